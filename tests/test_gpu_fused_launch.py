"""GPU: the fused launch of the batched handle's geometry half.  When the eight-hulls-per-wave hull kernel (hull_group_kernel) runs
over one hull list per agent it also writes the hulls' boxes and zeroes the presolve's redo counters (fe_box_kernel is not
launched), and from the second replan on its block 0 makes the round's QP launch order and zeroes the polish counters (order_kernel
is not launched).  Here: the boxes against an exact host reference, the fused sequence against the unfused one slot for slot (the
headline's inputs, config-5 style inputs with the entangle rows, an active set), the launch order's contract, the counters of every
round, and the static polygons' boxes across uploads of new polygons between eager rounds, under a captured graph and before a
capture (the graph contract of nep_batch_set_scene_statics, include/neptune_backend.h).  Every test proves from
nep_batch_debug_launch_path that it ran the path it is about.  Last, the launch topology itself: the table of scripts/launch_paths.py
against the answers recorded before the launch plan existed (tests/golden/launch_paths.json)."""
import dataclasses
import importlib.util
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from neptune_amd import abi, scene
from gpu_util import COEF_TOL, COST_RTOL

pytestmark = pytest.mark.gpu

HEAD_N, HEAD_M, HEAD_S = 64, 20, 40          # the headline's scenes: 2 560 trajectories (the grouped hull kernel from 2 048 on)
C5_N, C5_M, C5_SEEDS, C5_S = 256, 100, (41, 42), 5      # config-5 style: two scenes repeated, 1 280 slots (the launch order from 1 024 on)
WORKERS = 16                                 # host processes making scenes, oracle threads


@pytest.fixture(scope="module")
def be():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from neptune_amd import backend
    return backend


@pytest.fixture(scope="module")
def head(be):
    return scene.make_scenes(HEAD_N, HEAD_M, range(HEAD_S), workers=WORKERS)


@pytest.fixture(scope="module")
def c5(be):
    scs = scene.make_scenes(C5_N, C5_M, C5_SEEDS, workers=len(C5_SEEDS))
    cases = [scene.synthetic_entangle(sc, seed=1041 + k, frac=0.1) for k, sc in enumerate(scs)]      # (bend points into the records)
    return scs, cases


def _handle(be, p, statics, mode=0, order=True, cull=None):
    """one handle over len(statics) scenes, each with its own polygons (the first per-scene upload included)"""
    bb = be.BatchBackend(p, statics[0], n_scenes=len(statics))
    for s, st in enumerate(statics):
        bb.set_scene_statics(s, st)
    if mode:
        bb.set_hull_kernel(mode)
    if not order:
        bb.set_launch_order(False)
    if cull is not None:
        bb.set_line_cull(cull)
    return bb


def _stack(scs):
    return np.stack([sc["committed"] for sc in scs]), np.stack([sc["guesses"] for sc in scs])


def _poly_box(xy):
    """(x0, x1, y0, y1) of a polygon; an empty one gets the box nothing meets"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    if len(xy) == 0:
        return np.array([np.inf, -np.inf, np.inf, -np.inf])
    return np.array([xy[:, 0].min(), xy[:, 0].max(), xy[:, 1].min(), xy[:, 1].max()])


def _box_mismatches(bb, statics):
    """scenes whose boxes (nep_batch_debug_boxes) differ from min / max over the hull vertices of the last replan (debug_hulls) and
    over the uploaded polygons: [(scene, first (entry, interval) pairs that differ)]"""
    bad = []
    for s in range(bb.n_scenes):
        box = bb.debug_boxes(s)
        hx, hn = bb.debug_hulls(s)
        want = np.empty_like(box)
        for j in range(bb.N):
            for i in range(bb.par.num_pol):
                want[j, i] = _poly_box(hx[j, i, :hn[j, i]])
        for k, poly in enumerate(statics[s]):
            want[bb.N + k, :] = _poly_box(poly)
        if not np.array_equal(box, want):
            bad.append((s, np.argwhere((box != want).any(axis=2))[:4].tolist()))
    return bad


def _outputs(bb, active=None):
    """what the last replan left: solutions, states, commits, the lines of every (active) slot, every scene's hulls, the redo and
    polish counters"""
    sol = bb.solutions()
    lines = [bb.debug_lines(k, cap=20000) if active is None or active[k] else None for k in range(bb.slots)]
    hulls = []
    for s in range(bb.n_scenes):
        hx, hn = bb.debug_hulls(s)
        hx[np.arange(abi.NEP_HULL_MAX_V)[None, None, :] >= hn[:, :, None]] = 0.0      # (vertex slots past the count are scratch)
        hulls.append(hx.tobytes() + hn.tobytes())
    n = bb.redo_count()
    redo = (n, bb.redo_reasons["parked_line_violated"], bb.redo_reasons["moved_beyond_radius"], tuple(sorted(bb.redo_list().tolist())))
    return dict(sol=sol, states=bb.states().tobytes(), com=bb.commits().tobytes(), lines=lines, hulls=hulls, redo=redo,
                polish=bb.polish_count())


def _same_lines(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes())


def _differences(got, want):
    """the fields in which two _outputs differ (every slot, byte for byte)"""
    d = []
    if got["sol"].tobytes() != want["sol"].tobytes():
        d.append(("solutions", np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got["sol"], want["sol"])])[:8].tolist()))
    for k in ("states", "com"):
        if got[k] != want[k]:
            d.append(k)
    bad = [k for k, (a, b) in enumerate(zip(got["lines"], want["lines"])) if not _same_lines(a, b)]
    if bad:
        d.append(("lines", len(bad), bad[:8]))
    bad = [s for s, (a, b) in enumerate(zip(got["hulls"], want["hulls"])) if a != b]
    if bad:
        d.append(("hulls", bad[:8]))
    if got["redo"] != want["redo"]:
        d.append(("redo", got["redo"][:3], want["redo"][:3]))
    if got["polish"] != want["polish"]:
        d.append(("polish", got["polish"], want["polish"]))
    return d


def _check_oracle(oracle, p, scs, out, slots, cases=None):
    """the default-path checks of gpu_util._check_scene on a sample of slots (slot = scene * N + agent): statuses, LP and line counts,
    lines a subset of the oracle's bit for bit, coefficients within COEF_TOL, cost within COST_RTOL"""
    N = p.num_agents

    def key(k):                  # (a repeated scene poses the same problems: one oracle solve each)
        return id(scs[k // N]), k % N

    def solve(k):
        s, a = divmod(k, N)
        sc = scs[s]
        return oracle.replan(p, a + 1, sc["committed"], sc["guesses"][a], sc["statics"], case_id=None if cases is None else cases[s][a])
    first = {}
    for k in slots:
        first.setdefault(key(k), k)
    oracle.lib()
    with ThreadPoolExecutor(WORKERS) as ex:
        refs = dict(zip(first, ex.map(solve, first.values())))
    sol = out["sol"]
    for k in slots:
        r = refs[key(k)]
        st = sol[k]["stats"]; K = int(sol[k]["K"])
        assert int(st["status"]) == r["status"] and int(st["n_lines"]) == r["n_lines"], k
        assert int(st["n_lp"]) == r["n_lp"] and int(st["n_lp_failed"]) == r["n_lp_failed"], k
        want = {(int(s_), l.tobytes()) for s_, l in zip(r["line_seg"], r["line_nd"])}
        seg, nd = out["lines"][k]
        assert all((int(s_), np.ascontiguousarray(l).tobytes()) in want for s_, l in zip(seg, nd)), k
        err = np.abs(np.array(sol[k]["coeff"])[:, :K, :] - r["coeff"]).max()
        assert err <= COEF_TOL, (k, err)
        if r["status"] != 2:
            assert abs(float(st["objective"]) - r["objective"]) <= COST_RTOL * (1 + abs(r["objective"])), k


def _sample(S, N, per_scene):
    """every agent of scene 0 and a spread over the other scenes"""
    return list(range(N)) + [s * N + (37 * s + 11 * t) % N for s in range(1, S) for t in range(per_scene)]


def _new_statics(statics):
    """every fourth scene gets other polygons of the same count, all box-edged: half of them another scene's set, half their own
    translated -> (the sets of every scene, the changed scenes)"""
    S = len(statics)
    new = list(statics)
    changed = list(range(0, S, 4))
    for n_, s in enumerate(changed):
        new[s] = statics[(s + S // 2 + 1) % S] if n_ % 2 == 0 else [np.ascontiguousarray(np.asarray(q) + np.array([1.75, -1.25])) for q in statics[s]]
    return new, changed


def _fused_against_unfused(be, oracle, p, scs, mode=0, mask=None, cases=None, per_scene=2):
    """three eager rounds of a handle on the fused path and of two references on the same inputs — hull kernel 1 (fe_box_kernel +
    order_kernel), and hull kernel 1 with the launch order off: every output of every slot equal in every round; the last round's
    sample against the oracle"""
    import torch
    S, N = len(scs), p.num_agents
    statics = [sc["statics"] for sc in scs]
    com, gue = _stack(scs)
    act = None if mask is None else mask.reshape(-1).astype(bool)
    hs = [_handle(be, p, statics, mode=mode), _handle(be, p, statics, mode=1), _handle(be, p, statics, mode=1, order=False)]
    dev = []
    for bb in hs:
        if cases is not None:
            for s in range(S):
                reps, longest = scene.static_reps(statics[s])
                bb.set_static_reps(reps, longest, scene=s)
        if mask is not None:
            bb.set_active(torch.from_numpy(mask).to(bb.device))
        d_ent = torch.from_numpy(np.ascontiguousarray(np.stack(cases)).reshape(-1)).to(bb.device) if cases is not None else None
        dev.append((bb.to_device(com), bb.to_device(gue), d_ent))
    first = None
    for r in range(3):
        outs, paths = [], []
        for bb, (d_c, d_g, d_e) in zip(hs, dev):
            bb.replan(d_c, d_g, d_e)
            bb.check()                                    # (no capacity flag: a capped hull's boxes legitimately differ)
            outs.append(_outputs(bb, act)); paths.append(bb.debug_launch_path())
        fused, ref1, ref2 = paths
        assert fused["grouped_hulls"] and fused["fused_boxes"] and not fused["box_kernel"], (r, fused)
        assert fused["fused_order"] == (r > 0) and fused["ordered_qp"] == (r > 0), (r, fused)
        assert not ref1["grouped_hulls"] and not ref1["fused_boxes"] and not ref1["fused_order"] and ref1["box_kernel"], (r, ref1)
        assert ref1["ordered_qp"] == (r > 0), (r, ref1)                       # (order_kernel)
        assert not ref2["fused_boxes"] and not ref2["fused_order"] and not ref2["ordered_qp"] and ref2["box_kernel"], (r, ref2)
        assert fused["presolve_kernel"] and ref1["presolve_kernel"] and fused["redo_pass"] and ref1["redo_pass"], (fused, ref1)
        assert not _differences(outs[0], outs[1]), (r, "hull kernel 1", _differences(outs[0], outs[1]))
        assert not _differences(outs[0], outs[2]), (r, "hull kernel 1, slot order", _differences(outs[0], outs[2]))
        if first is None:
            first = outs[0]
        else:
            assert not _differences(outs[0], first), (r, "round 1", _differences(outs[0], first))
    sample = [k for k in _sample(S, N, per_scene) if act is None or act[k]]
    assert len(sample) >= 64
    _check_oracle(oracle, p, scs, outs[0], sample, cases)
    if act is not None:
        assert (outs[0]["sol"]["stats"]["status"][~act] == abi.NEP_SKIPPED).all()
    for bb in hs:
        bb.close()


# ---- A. boxes ------------------------------------------------------------------------------------------------------------------

def test_boxes_equal_the_host_reference(be):
    """fe_box_kernel's boxes and the hull kernel's fused ones: min / max over the hull vertices and over the uploaded polygons, bit for
    bit (numpy float64 reproduces a min / max exactly).  Time-jittered scenes, short guesses, invalid records (an empty hull: the box
    nothing meets) and agents at rest (coinciding control points).  Eight hulls per wave: the fused boxes, then fe_box_kernel's on the
    same handle (hulls reused: no records, so no fused launch), then fused again; and one hull per wave (fe_box_kernel)."""
    scs = scene.make_scenes(HEAD_N, HEAD_M, [7, 8], workers=2, t_jitter=0.3) + scene.make_scenes(HEAD_N, HEAD_M, [9, 10], workers=2, K=3)
    p = scs[0]["par"]
    com, gue = _stack(scs)
    for j in (3, 17, 40):
        com[1, j]["valid"] = 0                                                  # invalid records
    for s, j in ((2, 5), (3, 0), (3, 63)):                                      # at rest: every control point of every interval the same
        n = int(com[s, j]["pwp"]["n_seg"])
        c = np.array(com[s, j]["pwp"]["coeff"])
        c[:, :n, :3] = 0.0
        c[:, :n, 3] = c[:, 0, 3][:, None]
        com[s, j]["pwp"]["coeff"][:, :n, :] = c[:, :n, :]
    statics = [sc["statics"] for sc in scs]
    got = {}
    for mode in (2, 1):
        bb = _handle(be, p, statics, mode=mode)
        d_com, d_gue = bb.to_device(com), bb.to_device(gue)
        rounds = ((d_com, "fused_boxes"), (None, "box_kernel"), (d_com, "fused_boxes")) if mode == 2 else ((d_com, "box_kernel"),)
        for r, (d_c, via) in enumerate(rounds):
            bb.replan(d_c, d_gue)
            bb.check()                                                          # the hull capacity flag stays clear
            path = bb.debug_launch_path()
            assert path[via] and path["grouped_hulls"] == (mode == 2 and d_c is not None), (mode, r, path)
            assert not (path["fused_boxes"] and path["box_kernel"]), (mode, r, path)
            assert not _box_mismatches(bb, statics), (mode, r, _box_mismatches(bb, statics))
        _, hn = bb.debug_hulls(1)
        assert (hn[[3, 17, 40]] == 0).all() and (bb.debug_boxes(1)[[3, 17, 40], :, 0] == np.inf).all()
        got[mode] = [bb.debug_boxes(s) for s in range(len(scs))]
        bb.close()
    for s in range(len(scs)):
        np.testing.assert_array_equal(got[1][s], got[2][s])


# ---- B. the fused sequence against the unfused one ------------------------------------------------------------------------------

def test_fused_launch_equals_unfused_on_the_headline_inputs(be, oracle, head):
    """(i) the headline's scenes with their own statics and the handle's default selection (2 560 trajectories: the grouped kernel)"""
    _fused_against_unfused(be, oracle, head[0]["par"], head)


def test_fused_launch_equals_unfused_with_the_entangle_rows(be, oracle, c5):
    """(ii) config-5 style: 256 agents, 100 statics, synthetic entangle cases and static representatives, eight hulls per wave forced;
    the grouped kernel's entangle outputs (uninflated hulls, bend points) feed the entangle rows"""
    scs, cases = c5
    scs5 = [scs[s % 2] for s in range(C5_S)]; cases5 = [cases[s % 2] for s in range(C5_S)]
    p = dataclasses.replace(scs[0]["par"], enable_entangle=True)
    _fused_against_unfused(be, oracle, p, scs5, mode=2, cases=cases5, per_scene=4)


def test_fused_launch_equals_unfused_under_an_active_set(be, oracle, head):
    """(iii) the headline's inputs with a quarter of the agents active (scene 0 whole: the oracle sample)"""
    mask = (np.random.default_rng(5).random((HEAD_S, HEAD_N)) < 0.25).astype(np.int32)
    mask[0, :] = 1
    _fused_against_unfused(be, oracle, head[0]["par"], head, mask=mask, per_scene=4)


# ---- C. the launch order ----------------------------------------------------------------------------------------------------------

def test_launch_order_sorts_by_the_previous_rounds_keys(be, head):
    """The order of round r + 1 is a permutation of the slots with keys[order] & 63 non-increasing, keys as round r left them: the hull
    kernel's block-0 counting sort (fused) and order_kernel.  (Within a bin the order depends on atomics: not compared across handles.)"""
    p = head[0]["par"]; statics = [sc["statics"] for sc in head]
    com, gue = _stack(head)
    for mode in (0, 1):
        bb = _handle(be, p, statics, mode=mode)
        d_com, d_gue = bb.to_device(com), bb.to_device(gue)
        bb.replan(d_com, d_gue)
        assert bb.launch_order() is None                                        # first replan: slot order
        for r in range(2):
            keys = bb.debug_order_keys()
            bb.replan(d_com, d_gue)
            path = bb.debug_launch_path()
            assert path["ordered_qp"] and path["fused_order"] == (mode == 0), (mode, path)
            order = bb.launch_order()
            assert order is not None and np.array_equal(np.sort(order), np.arange(bb.slots))
            k = keys[order] & 63
            assert (np.diff(k) <= 0).all(), (mode, r, np.flatnonzero(np.diff(k) > 0)[:8])
            assert k[0] > k[-1]                                                 # (the keys spread: the sort had something to do)
        bb.close()


# ---- D. counters ----------------------------------------------------------------------------------------------------------------

def test_counters_start_every_round_at_zero(be, head):
    """A 5 cm presolve radius lists many replans for the redo pass (the polish pass at its default, on).  The redo counts per reason,
    the redo list and the polish counts of the fused rounds 2 and 3 equal round 1's and those of hull kernel 1 (where fe_box_kernel
    and order_kernel zero them): counters that accumulated would differ."""
    p = head[0]["par"]; statics = [sc["statics"] for sc in head]
    com, gue = _stack(head)
    seen = []
    for mode in (0, 1):
        bb = _handle(be, p, statics, mode=mode, cull=0.05)
        d_com, d_gue = bb.to_device(com), bb.to_device(gue)
        for r in range(3):
            bb.replan(d_com, d_gue)
            path = bb.debug_launch_path()
            assert path["redo_pass"] and path["fused_boxes"] == (mode == 0) and path["fused_order"] == (mode == 0 and r > 0), (mode, r, path)
            n = bb.redo_count()
            seen.append(((n, bb.redo_reasons["parked_line_violated"], bb.redo_reasons["moved_beyond_radius"]), sorted(bb.redo_list().tolist()), bb.polish_count()))
        bb.close()
    assert seen[0][0][0] > 100, seen[0][0]
    for k, s in enumerate(seen[1:], 1):
        assert s == seen[0], (k, s[0], seen[0][0], s[2], seen[0][2])


# ---- E-G. static boxes across uploads --------------------------------------------------------------------------------------------

def _fresh(be, p, statics, com, gue):
    """one replan of a new handle built with these polygons"""
    bb = _handle(be, p, statics)
    bb.replan(bb.to_device(com), bb.to_device(gue))
    bb.check()
    out = _outputs(bb)
    bb.close()
    return out


def test_statics_upload_between_eager_rounds(be, head):
    """After two fused rounds a quarter of the scenes get new polygons of the same count: the next replan equals a fresh handle built
    with them, and the static boxes are the new polygons'.  The upload changes the problems of most slots of those scenes."""
    p = head[0]["par"]; statics = [sc["statics"] for sc in head]
    com, gue = _stack(head)
    new, changed = _new_statics(statics)
    bb = _handle(be, p, statics)
    d_com, d_gue = bb.to_device(com), bb.to_device(gue)
    for _ in range(2):
        bb.replan(d_com, d_gue)
    path = bb.debug_launch_path()
    assert path["fused_boxes"] and path["fused_order"], path
    before = _outputs(bb)
    for s in changed:
        bb.set_scene_statics(s, new[s])
    bb.replan(d_com, d_gue)
    bb.check()
    got = _outputs(bb)
    boxes = _box_mismatches(bb, new)
    diff = _differences(got, _fresh(be, p, new, com, gue))
    assert not boxes and not diff, (boxes, diff)
    slots = [s * HEAD_N + a for s in changed for a in range(HEAD_N)]
    moved = [k for k in slots if int(got["sol"][k]["stats"]["n_lp"]) != int(before["sol"][k]["stats"]["n_lp"])
             or not _same_lines(got["lines"][k], before["lines"][k])]
    assert len(moved) >= 0.5 * len(slots), (len(moved), len(slots))
    bb.close()


def test_graph_replayed_after_an_upload_reads_the_new_static_boxes(be, head):
    """Capture, upload, replay: a replan captured on the fused path (no fe_box_kernel node) after the first per-scene upload and two
    eager rounds replays as the eager round ran; after new polygons of the same count for several scenes its replay equals a fresh
    handle built with them, and the static boxes are the new polygons'."""
    import torch
    p = head[0]["par"]; statics = [sc["statics"] for sc in head]
    com, gue = _stack(head)
    new, changed = _new_statics(statics)
    bb = _handle(be, p, statics)
    d_com, d_gue = bb.to_device(com), bb.to_device(gue)
    cur = torch.cuda.current_stream(bb.device)
    s_ = torch.cuda.Stream(bb.device)
    s_.wait_stream(cur)
    with torch.cuda.stream(s_):
        for _ in range(2):
            bb.replan(d_com, d_gue)
    cur.wait_stream(s_)
    bb.check()
    eager = _outputs(bb)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bb.replan(d_com, d_gue)
    path = bb.debug_launch_path()
    assert path["fused_boxes"] and path["fused_order"] and not path["box_kernel"], path
    g.replay()
    bb.check()
    replayed = _outputs(bb)
    assert not _differences(replayed, eager), _differences(replayed, eager)
    for s in changed:
        bb.set_scene_statics(s, new[s])
    g.replay()
    bb.check()
    got = _outputs(bb)
    boxes = _box_mismatches(bb, new)
    diff = _differences(got, _fresh(be, p, new, com, gue))
    assert not boxes and not diff, (boxes, diff)
    del g
    bb.close()


def test_eager_replan_after_an_upload_and_a_capture_reads_the_new_static_boxes(be, head):
    """Upload, capture, eager: new polygons after two eager rounds, a replan captured and never replayed (none of it ran), then an
    eager replan: it equals a fresh handle built with the new polygons, and the static boxes are theirs."""
    import torch
    p = head[0]["par"]; statics = [sc["statics"] for sc in head]
    com, gue = _stack(head)
    new, changed = _new_statics(statics)
    bb = _handle(be, p, statics)
    d_com, d_gue = bb.to_device(com), bb.to_device(gue)
    for _ in range(2):
        bb.replan(d_com, d_gue)
    bb.check()
    for s in changed:
        bb.set_scene_statics(s, new[s])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bb.replan(d_com, d_gue)
    bb.replan(d_com, d_gue)
    bb.check()
    assert bb.debug_launch_path()["grouped_hulls"]
    got = _outputs(bb)
    boxes = _box_mismatches(bb, new)
    diff = _differences(got, _fresh(be, p, new, com, gue))
    assert not boxes and not diff, (boxes, diff)
    del g
    bb.close()


# ---- H. the launch topology against the recorded one ------------------------------------------------------------------------------

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(_ROOT, "tests", "golden", "launch_paths.json")) as _f:
    _RECORDED = json.load(_f)["cases"]


@pytest.fixture(scope="module")
def launch_paths(be):
    """scripts/launch_paths.py as a module, and its four base scenes (made once)"""
    spec = importlib.util.spec_from_file_location("launch_paths", os.path.join(_ROOT, "scripts", "launch_paths.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, scene.make_scenes(mod.N_AGENTS, mod.N_STATIC, mod.SEEDS, workers=1)


def test_launch_path_table_is_the_recorded_one(launch_paths):
    mod, _ = launch_paths
    assert [(n, s, v) for n, s, v in mod.cases()] == [(c["name"], c["scenes"], c["variant"]) for c in _RECORDED]


@pytest.mark.parametrize("case", _RECORDED, ids=["%s-%d" % (c["name"], c["scenes"]) for c in _RECORDED])
def test_launch_paths_equal_the_recorded_ones(be, launch_paths, case):
    """three replans of the case's handle: the launch-path bits, launch_order() is None, the polish counters seen armed and
    qp_kernel_name() of every call as recorded at the commit before Engine::run followed a plan (8 agents, 2 statics, 1 to 512 scenes:
    both sides of the 1 024-slot, 2 048-record and 4 096-slot thresholds)"""
    import torch
    mod, base = launch_paths
    got = mod.run_case(be, scene, torch, base, case["scenes"], case["variant"])
    assert len(got) == len(case["calls"]) == 3
    for r, (g, w) in enumerate(zip(got, case["calls"])):
        assert all(g[k] == w[k] for k in mod.ANSWERS), (r, g, w)
