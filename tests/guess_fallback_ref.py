"""The degrade-to-initial-guess rule (nep_batch_guess_fallback) in plain numpy over abi.SOLUTION_DTYPE,
abi.GUESS_DTYPE and abi.TRAJ_REC_DTYPE arrays.  It shares no code with the library: the tests compare the kernels' bytes with it.

The reference: when both solves fail, pwp_out_ = pwp_init_ (solver_gurobi_poly.cpp:856-859) and Neptune::replanFull goes on with it
(neptune.cpp:1519-1527, the early return is commented out): the guess is sampled, judged by safetyCheckAfterReplan (:1644) and
published (:1661-1699)."""
import numpy as np

OK, RELAXED, FAILED, SKIPPED, GUESS = 0, 1, 2, 3, 4
FLEET_ACCEPTED = 4
MAX_POL, TRAJ_MAX_SEG = 8, 16


def publishable(sol, num_pol):
    """is this slot examined, and has it a guess to publish"""
    examined = int(sol["stats"]["status"]) == FAILED
    return examined, examined and 1 <= int(sol["K"]) <= num_pol


def record(left, sol, guess, agent, pb, drone_radius):
    """the record a published slot gets: `left` (what the replan left in the slot) with the fields the replan's writer gives a
    solved slot, for the trajectory in `sol` (the guess).  agent: the global 0-based index.  bend[1..] and pwp._pad stay `left`'s"""
    r = np.zeros(1, dtype=left.dtype); r[0] = left      # (a copy: a record taken out of an array is a view of it)
    K = int(sol["K"])
    r["id"] = agent + 1; r["is_agent"] = 1; r["n_bend"] = 1; r["valid"] = 1
    r["bbox"] = 2 * drone_radius
    r["pos"] = np.array(guess["coeff"])[:, 0, 3]
    r["bend"][0, 0] = np.asarray(pb, dtype=np.float64).reshape(-1, 2)[agent]
    r["pwp"]["n_seg"] = K
    r["pwp"]["times"][0] = 0.0; r["pwp"]["times"][0, : K + 1] = np.array(sol["times"])[: K + 1]
    r["pwp"]["coeff"][0] = 0.0; r["pwp"]["coeff"][0, :, :K, :] = np.array(sol["coeff"])[:, :K, :]
    r = r[0]
    return r


def fallback(sol, guess, commit, num_pol, pb, drone_radius, first_local=0, n_local=None, count=None):
    """one call over every slot -> (sol', commit', count') with count [n_scenes][4] added to ([0] examined, [1] published)"""
    sol = np.array(sol, copy=True); commit = np.array(commit, copy=True)
    n_local = len(sol) if n_local is None else n_local
    count = np.zeros((len(sol) // n_local, 4), dtype=np.int32) if count is None else np.array(count, copy=True)
    for slot in range(len(sol)):
        ex, pub = publishable(sol[slot], num_pol)
        if not ex:
            continue
        count[slot // n_local, 0] += 1
        if not pub:
            continue
        count[slot // n_local, 1] += 1
        commit[slot] = record(commit[slot], sol[slot], guess[slot], first_local + slot % n_local, pb, drone_radius)
        sol["stats"]["status"][slot] = GUESS
    return sol, commit, count


def tally(sol, outcome, n_local, count):
    """after the fleet's commit: [2] += published guesses that were accepted, [3] += the others"""
    count = np.array(count, copy=True)
    for slot in range(len(sol)):
        if int(sol[slot]["stats"]["status"]) == GUESS:
            count[slot // n_local, 2 if int(outcome[slot]) == FLEET_ACCEPTED else 3] += 1
    return count


def written_mask(itemsize, fields):
    """the bytes of a record the writer writes: everything but bend[1..] and pwp._pad -> bool [itemsize]"""
    m = np.ones(itemsize, dtype=bool)
    bend_dt, bend_off = fields["bend"][0], fields["bend"][1]
    m[bend_off + 16: bend_off + bend_dt.itemsize] = False
    pwp_dt, pwp_off = fields["pwp"][0], fields["pwp"][1]
    pad_off = pwp_off + pwp_dt.fields["_pad"][1]
    m[pad_off: pad_off + 4] = False
    return m


def infeasible_guess(g, x_max):
    """a guess whose start lies outside the world box: neither solve can hold the first control point's position rows"""
    g = g.copy()
    co = np.array(g["coeff"])
    co[0, :, 3] += (x_max + 5.0) - co[0, 0, 3]
    g["coeff"] = co
    return g


def fixture(scene_mod):
    """scene.make_scene(5, 3, seed=4) with guesses[1] shifted outside the world, guesses[3] the same bytes, guesses[2].K = 0"""
    sc = scene_mod.make_scene(5, 3, seed=4)
    gue = sc["guesses"].copy()
    gue[1] = infeasible_guess(gue[1], sc["par"].x_max)
    gue[3] = gue[1]
    gue[2]["K"] = 0
    return sc, gue
