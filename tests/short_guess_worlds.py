"""The inputs of the short-guess tests (test_short_guess_worlds_cpu.py fixes by the oracle alone that they are not vacuous,
test_gpu_short_guess_paths.py flies them): 8-agent worlds at num_pol D in 5..8 whose slots replan with guesses of DIFFERENT lengths
K <= D — what the best-first front ends return without pad_hold, and what the goal gate and fly-the-guess then fly.  Host side, numpy
only, deterministic (a world depends on D, its seed and its shift alone).

A world is a dict like scene.make_scene's: par, statics, guesses [N], committed [N], plus case (None, or the entangle cases
[N][NEP_MAX_POL][N] of with_entangle) and name.  Nothing here is modified after it is returned: every function copies."""
import dataclasses
import functools

import numpy as np

import param_sets as PS
from neptune_amd import scene

N = 8
DS = (5, 6, 7, 8)

# Seeds per D, chosen by the oracle (test_short_guess_worlds_cpu.py asserts what they were chosen for).  truncated: over a D's seeds
# the statuses include OK, RELAXED and FAILED, a slot with K < D has an active line row, a slot has an active box row and no LP fails.
# at_rest: for every K in 3..D a slot ends OK with no active row at all.
TRUNCATED_SEEDS = {5: (5, 6, 8), 6: (5, 6), 7: (5, 8), 8: (5, 8)}
AT_REST_SEEDS = {5: (11, 12), 6: (11, 12), 7: (11, 12), 8: (11, 12)}
ENT_DS = (6, 8)          # the entangle variants: with_entangle(world, ent_seed(seed))


def ent_seed(seed):
    """scene.synthetic_entangle's draw per world seed (on these the oracle poses entangle LPs in slots with K < D)"""
    return 31 + seed

# with_misses(world, variant): the two slots whose front end found nothing (K = 0, coefficients zero) and the slot whose start lies
# outside the world box (fails both solves), agent D - 1 - variant: K = D and K = D - 1 at shift 0
MISSES = ((0, 3), (1, 7))


def guess_length(a, D, shift=0):
    """segments of agent a's guess: 1..D, cycling over the agents"""
    return ((a + shift) % D) + 1


def bad_agent(D, variant):
    return D - 1 - variant


def fast_long_params(D):
    """param_sets.SETS["fast_long"] at num_pol = D, 8 agents + 6 obstacles"""
    return scene.scaled_params(N, 6, num_pol=D, **PS.SETS["fast_long"])


def at_rest_params(D):
    return scene.scaled_params(N, 3, num_pol=D)


@functools.lru_cache(maxsize=None)
def _scene(kind, D, seed, K):
    if kind == "truncated":
        return scene.make_scene(N, 6, seed=seed, K=K, par=fast_long_params(D))
    return scene.make_scene(N, 3, seed=seed, K=K, par=at_rest_params(D))


def _world(sc, guesses, name):
    return dict(par=sc["par"], statics=[np.array(s) for s in sc["statics"]], guesses=guesses, committed=sc["committed"].copy(), case=None, name=name)


def truncated(D, seed, shift=0):
    """fast_long at num_pol = D: agent a keeps the first guess_length(a, D, shift) segments of its D-segment guess, the rest zeroed.
    Such a guess ends at speed: these replans iterate."""
    sc = _scene("truncated", D, seed, D)
    gue = sc["guesses"].copy()
    for a in range(N):
        K = guess_length(a, D, shift)
        gue["K"][a] = K
        gue["coeff"][a, :, K:, :] = 0.0
    return _world(sc, gue, "truncated D%d seed %d shift %d" % (D, seed, shift))


def at_rest(D, seed, shift=0):
    """the default parameter point at num_pol = D, 8 agents + 3 obstacles: agent a flies the guess the scene generator makes for it
    at K = guess_length(a, D, shift) segments (a roll-out that brakes to rest at its end); the committed records and the statics are
    the K = D scene's (the per-K scenes' are not byte-equal to each other)"""
    sc = _scene("at_rest", D, seed, D)
    gue = sc["guesses"].copy()
    for a in range(N):
        gue[a] = _scene("at_rest", D, seed, guess_length(a, D, shift))["guesses"][a]
    return _world(sc, gue, "at_rest D%d seed %d shift %d" % (D, seed, shift))


def full_length(D, seed):
    """at_rest's scene with every slot at K = D"""
    sc = _scene("at_rest", D, seed, D)
    return _world(sc, sc["guesses"].copy(), "at_rest D%d seed %d full length" % (D, seed))


def infeasible_guess(g, p):
    """start outside the world box: the position rows of the first control point cannot hold in either solve"""
    g = g.copy()
    co = np.array(g["coeff"])
    co[0, :, 3] += (p.x_max + 5.0) - co[0, 0, 3]
    g["coeff"] = co
    return g


def with_misses(w, variant=0):
    """two slots with K = 0 (front-end miss, coefficients zero) and one slot made infeasible"""
    D = w["par"].num_pol
    gue = w["guesses"].copy()
    for a in MISSES[variant]:
        gue["K"][a] = 0
        gue["coeff"][a] = 0.0
    b = bad_agent(D, variant)
    gue[b] = infeasible_guess(gue[b], w["par"])
    return dict(w, guesses=gue, name=w["name"] + " misses %d" % variant)


def with_overlong(w):
    """agent num_pol - 1 (a full-length guess at shift 0) claims a segment more than the handle plans for (K = num_pol + 1, the
    extra segment zero): the library reports NEP_FAILED with an empty solution for it, and the separators make lines for its first
    num_pol segments only — never compared with the oracle (which has no such case), only between the separator kernels"""
    gue = w["guesses"].copy()
    gue["K"][w["par"].num_pol - 1] = w["par"].num_pol + 1
    return dict(w, guesses=gue, name=w["name"] + " overlong")


def with_entangle(w, seed):
    """enable_entangle and scene.synthetic_entangle's cases and bend points (frac 0.3): with entangle candidates the packed
    separator keeps its ballots in LDS rather than in lanes"""
    tmp = dict(par=w["par"], guesses=w["guesses"], committed=w["committed"].copy())
    case = scene.synthetic_entangle(tmp, seed=seed, frac=0.3)
    return dict(w, par=dataclasses.replace(w["par"], enable_entangle=True), committed=tmp["committed"], case=case, name=w["name"] + " entangle")


def stack(worlds):
    """worlds of one parameter set as the scenes of one handle -> (par, statics per scene, guesses [S][N], committed [S][N],
    cases [S][N][NEP_MAX_POL][N] or None)"""
    p = worlds[0]["par"]
    gue = np.stack([w["guesses"] for w in worlds]); com = np.stack([w["committed"] for w in worlds])
    case = None if worlds[0]["case"] is None else np.ascontiguousarray(np.stack([w["case"] for w in worlds]))
    return p, [w["statics"] for w in worlds], np.ascontiguousarray(gue), np.ascontiguousarray(com), case


def oracle_results(oracle, w):
    """oracle.replan of every slot with a guess (None for K = 0: nothing to solve)"""
    out = []
    for a in range(N):
        g = w["guesses"][a]
        out.append(None if int(g["K"]) == 0 else oracle.replan(w["par"], a + 1, w["committed"], g, w["statics"],
                                                                case_id=None if w["case"] is None else w["case"][a]))
    return out


def active_rows(w, a, r):
    """(box rows, line rows) active at the oracle's optimum of slot a"""
    return scene.active_rows(w["par"], r["coeff"], int(w["guesses"][a]["K"]), r["line_seg"], r["line_nd"])
