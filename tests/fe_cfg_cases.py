"""The front-end settings sweep, stated once: the named nep_fe_cfg settings (overrides on scene.frontend_cfg's result), the scene
set-ups they are run on and the references' outcomes at them — shared by tests/test_fe_cfg_cases_cpu.py (the references alone: every
pair used on the device differs from the default setting and is not degenerate) and tests/test_gpu_fe_cfg_sweep.py (the kernels).
The set-ups are tests/test_gpu_frontend_entangle.py's (scene.tether_crossing_scene, scene.synthetic_entangle, every third search
starting with a crossing) and tests/astar_ent_cases.py's; nothing here generates a scene of its own."""
import functools

import numpy as np

import astar_ent_cases as cases
import helpers
from neptune_amd import abi, scene

# ---- the settings: scene.frontend_cfg gives voxel_size 0.2, bias 1.1, goal_size 0.2, cable_length = par.tether_length, num_samples 5, ent_samples 3
SETTINGS = {
    "default": {},
    "ent1": dict(ent_samples=1), "ent2": dict(ent_samples=2), "ent5": dict(ent_samples=5), "ent8": dict(ent_samples=8),
    "voxel0.1": dict(voxel_size=0.1), "voxel0.45": dict(voxel_size=0.45),
    "bias1.0": dict(bias=1.0), "bias2.5": dict(bias=2.5),
    "goal0.05": dict(goal_size=0.05), "goal0.6": dict(goal_size=0.6),
    "lattice2": dict(num_samples=2), "lattice4": dict(num_samples=4),
    "cable4": dict(cable_length=4.0),      # (the handle's tether_length stays at the scene's 200: a kernel reading that one instead shows)
    "combined": dict(ent_samples=5, voxel_size=0.3, bias=1.7, goal_size=0.4, num_samples=4),
}
ENT_SAMPLES = ("ent1", "ent2", "ent5", "ent8")
EVERY = tuple(k for k in SETTINGS if k != "default")
NO_CHECK = ("voxel0.1", "voxel0.45", "bias1.0", "bias2.5", "goal0.05", "goal0.6", "lattice2", "lattice4", "combined")      # the settings a search without the check reads

# ---- the beam's set-ups: name -> (agents, statics, seed, beam width, stride of the agents held to the oracle, bends: 0 none, 1: 2-4, 2: 5-8)
BEAM_SETUPS = {
    "8+6": (8, 6, 60, 16, 1, 0),
    "16+8 bends 2-4": (16, 8, 66, 16, 1, 1),
    "24+10 bends 2-4": (24, 10, 67, 32, 1, 1),
    "12+4 bends 5-8": (12, 4, 68, 16, 1, 2),
    "72+40": (72, 40, 63, 16, 6, 0),      # (more than one mask word of agents and of statics; every sixth agent, from BEAM_FIRST on)
    "16+8": (16, 8, 61, 16, 1, 0),        # (the big-record instantiation's scene)
    "5+0 wide": (5, 0, 64, 64, 1, 0),
    "8+6 wide": (8, 6, 60, 64, 1, 0), "12+4 bends 5-8 wide": (12, 4, 68, 64, 1, 2),      # (the widest beam where the 5-agent scene cannot tell a goal_size from the default)
}
BEAM_FIRST = {"72+40": 4}                 # (agents 4, 10, ..., 70: agent 46 is the one whose search tells every sample count from 3)
ASTAR_POPS = 150

# ---- what tests/test_gpu_fe_cfg_sweep.py runs.  On every pair of the *_PAIRS lists the reference tells the setting from the default
# one and is not degenerate (tests/test_fe_cfg_cases_cpu.py asserts it).  Where it cannot on the first set-up, the setting has moved to
# another of the same set-ups on which it can, and the first pair stays in the run as one of *_SAME: the device is held to the
# reference there as well, and the CPU file asserts that the reference's outcome there is the default setting's, so that nobody takes
# that run for a test of the setting.
BEAM_ENT_PAIRS = ([("8+6", s) for s in EVERY] + [(k, s) for k in ("16+8 bends 2-4", "12+4 bends 5-8", "72+40") for s in ENT_SAMPLES])
BEAM_BIG_PAIRS = [("16+8", "ent5"), ("16+8", "ent8")]
BEAM_TABLE_PAIRS = [(k, s) for k in ("16+8 bends 2-4", "24+10 bends 2-4", "12+4 bends 5-8") for s in ("ent1", "ent2", "ent8")]      # (CPU only: the three set-ups the sample counts were first tried on)
BEAM_PLAIN_SAME = [("8+6", "goal0.6"), ("5+0 wide", "goal0.05"), ("5+0 wide", "goal0.6")]
BEAM_PLAIN_PAIRS = ([(k, s) for k in ("8+6", "5+0 wide") for s in NO_CHECK if (k, s) not in BEAM_PLAIN_SAME] +
                    [("12+4 bends 5-8", "goal0.6"), ("8+6 wide", "goal0.05"), ("12+4 bends 5-8 wide", "goal0.6")])
ASTAR_PLAIN_PAIRS = [("plain", s) for s in NO_CHECK]
ASTAR_ENT_SAME = [("plain", "ent5"), ("plain", "ent8"), ("plain", "goal0.6")]      # (ent5 and ent8 are told apart on "bends")
ASTAR_ENT_PAIRS = ([("plain", s) for s in EVERY if ("plain", s) not in ASTAR_ENT_SAME] + [("bends", s) for s in ("ent1", "ent5", "ent8", "combined")] +
                   [("doubly", "goal0.6")])


def overrides(setting):
    return tuple(sorted(SETTINGS[setting].items()))


def fe_of(p, setting, beam_width=32, entangle=True, pad_hold=0):
    """the nep_fe_cfg of a setting: scene.frontend_cfg's with the setting's fields written over it"""
    fe = scene.frontend_cfg(p, beam_width=beam_width, pad_hold=pad_hold, entangle=entangle)
    for k, v in SETTINGS[setting].items():
        setattr(fe, k, v)
    return fe


def ent_of(sc, a, fe, init=None, t0=None, recs=None):
    """helpers.ent_inputs of agent a with the trajectories sampled at the setting's own count"""
    return helpers.ent_inputs(sc, a, num_samples=int(fe.ent_samples), init=init, recs=recs, t0=t0)


def lattice_order(fe):
    """the natural order of the setting's lattice, as nep_batch_set_fe_astar wants it spelled for a lattice other than 5 x 5"""
    return None if fe.num_samples == 5 else np.arange(fe.num_samples * fe.num_samples, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def beam_setup(key):
    """-> (scene, initial states [N]) as test_entangle_front_end_matches_the_oracle_bit_for_bit builds them"""
    N, M, seed, _, _, bends = BEAM_SETUPS[key]
    sc = scene.tether_crossing_scene(N, M, seed)
    if bends:
        scene.synthetic_entangle(sc, seed=900 + seed, frac=0.1, nb_range=(2, 5) if bends == 1 else (5, 9))
    return sc, cases.third_agent_inits(N, seed)


def beam_agents(key):
    N, _, _, _, stride, _ = BEAM_SETUPS[key]
    return range(BEAM_FIRST.get(key, 0), N, stride)


_BEAM = {}


def beam_want(oracle, key, setting, check=True):
    """{agent: (guess, result dict, case block or None)} of the C oracle's beam on set-up `key` at `setting`, for beam_agents(key);
    computed once per (set-up, setting, check) and never changed"""
    have = _BEAM.setdefault((key, setting, overrides(setting), check), {})
    if have:
        return have
    sc, inits = beam_setup(key)
    p = sc["par"]
    fe = fe_of(p, setting, beam_width=BEAM_SETUPS[key][3], entangle=check)
    starts = scene.frontend_starts(sc)
    for a in beam_agents(key):
        t0 = float(starts[a]["t_start"])
        hx, hn = oracle.hulls_of_scene(p, a + 1, sc["committed"], t0, sc["statics"])
        if check:
            have[a] = oracle.frontend_beam_ent(p, fe, a + 1, starts[a], hx, hn, sc["statics"], ent_of(sc, a, fe, init=inits[a], t0=t0))
        else:
            have[a] = oracle.frontend_beam(p, fe, a + 1, starts[a], hx, hn, sc["statics"]) + (None,)
    return have


_ASTAR = {}


def astar_plain_want(oracle, name, setting, max_pops=ASTAR_POPS):
    """{agent: (guess, result dict, None)} of the C oracle's best-first search (no check) on astar_ent_cases.setup(name) at `setting`"""
    have = _ASTAR.setdefault((name, setting, overrides(setting), max_pops), {})
    if have:
        return have
    sc = cases.setup(name)[0]
    p = sc["par"]
    fe = fe_of(p, setting, entangle=False)
    starts = cases.starts_of(name)
    for a in range(p.num_agents):
        hx, hn = oracle.hulls_of_scene(p, a + 1, sc["committed"], float(starts[a]["t_start"]), sc["statics"])
        have[a] = oracle.frontend_astar(p, fe, a + 1, starts[a], hx, hn, sc["statics"], order=lattice_order(fe), max_pops=max_pops) + (None,)
    return have


def astar_ent_want(oracle, name, setting, max_pops=ASTAR_POPS):
    """tests/astar_ent_ref.py with the check on at `setting`, through astar_ent_cases.want (whose cache key carries the setting)"""
    return cases.want(oracle, name, max_pops=max_pops, setting=overrides(setting))


# the C oracle's entangleCheckGivenPwp on recheck_inputs(scene.tether_crossing_scene(16, 8, 66)), per ent_samples: agent 12, who
# hovers while agent 15's new trajectory drags its tether past, comes out entangled only when the interval is sampled at three steps
# or more (tests/test_fe_cfg_cases_cpu.py recomputes them)
RECHECK_SCENE = (16, 8, 66)
RECHECK_VERDICTS = {k: [0, 1, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0, int(k >= 3), 1, 0, 0] for k in (1, 2, 3, 5, 8)}


def recheck_inputs(sc):
    """New trajectories and states at A on which the safety pass's entangle re-check has something to decide, from a
    scene.tether_crossing_scene: there agent a = (j + 3) % N passes the tether of every hovering (even) agent j at a knot of its
    guess — between the second and the sixth, never in the first interval, which is all entangleCheckGivenPwp looks at.  So a's new
    trajectory here is its guess from the segment before that knot on (re-timed to start at the guess's t_start), everybody else
    keeps the committed record, and a's state at A holds one crossing of j already: a second one is an entanglement.  Whether the
    first interval does cross depends on the hover point's scatter and on where the sampled steps fall.
    -> (records [N] TRAJ_REC_DTYPE, states [N] FE_ENT_STATE_DTYPE)"""
    p = sc["par"]; N = p.num_agents; T = p.T_span
    fresh = sc["committed"].copy()
    inits = np.zeros(N, dtype=abi.FE_ENT_STATE_DTYPE)
    for a in range(N):
        inits[a]["n_alpha"] = 1; inits[a]["id"][0] = (a + 3) % N + 1; inits[a]["cs"][0] = 1      # (test_safety_pass_entangle_recheck's states)
    for j in range(0, N, 2):
        a = (j + 3) % N
        g = sc["guesses"][a]; K = int(g["K"])
        co = np.array(g["coeff"])
        knots = np.stack([co[0, :K, 3], co[1, :K, 3]], axis=1)
        k = int(np.argmin(((knots - np.array(sc["committed"][j]["pos"])[:2]) ** 2).sum(axis=1)))
        s = max(k - 1, 0)
        r = fresh[a]
        r["pwp"]["coeff"][:] = 0; r["pwp"]["times"][:] = 0
        r["pwp"]["n_seg"] = K - s
        r["pwp"]["coeff"][:, :K - s, :] = co[:, s:K, :]
        r["pwp"]["times"][: K - s + 1] = float(g["t_start"]) + T * np.arange(K - s + 1)
        r["pos"] = co[:, s, 3]
        inits[a]["id"][0] = j + 1
    return fresh, inits


def differs(want, base, goal_only=False):
    """what separates a reference outcome from the default setting's on the same set-up -> the kinds of difference found.  A setting
    counts as told apart by guess bytes, case block or n_entangled; goal_size by K or the status"""
    kinds = set()
    for a in want:
        g, r = want[a][0], want[a][1]
        g0, r0 = base[a][0], base[a][1]
        if np.asarray(g).tobytes() != np.asarray(g0).tobytes():
            kinds.add("guess")
        if want[a][2] is not None and not np.array_equal(want[a][2], base[a][2]):
            kinds.add("case")
        if r["n_entangled"] != r0["n_entangled"]:
            kinds.add("n_entangled")
        if r["K"] != r0["K"]:
            kinds.add("K")
        if r["status"] != r0["status"]:
            kinds.add("status")
    return kinds & ({"K", "status"} if goal_only else {"guess", "case", "n_entangled"})


def outline(want):
    """(statuses seen, searches with K >= 1, summed n_entangled) of a reference outcome"""
    rs = [w[1] for w in want.values()]
    return sorted({r["status"] for r in rs}), sum(r["K"] >= 1 for r in rs), sum(r["n_entangled"] for r in rs)
