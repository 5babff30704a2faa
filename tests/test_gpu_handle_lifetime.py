"""GPU: who owns the library's memory.  Every device buffer and page-locked arena of the two handle kinds and of the stand-alone
calls frees itself (DevBuf / PinnedArena in backend.hip), and nep_debug_live_bytes reports what the process holds right now.  Each
case reads it first and finds both numbers back at exactly that reading afterwards; the readings are relative because other tests'
fixtures may hold handles.  The shapes are the smallest that reach every owner: a 2 x 4 batched handle with static obstacles,
tethers, the fleet state, an active set, the audit and the profile counters; a per-agent handle with its arenas and the temporary
buffers of generatePwpOut; a create that fails after its first allocation; the three stand-alone calls.

The batched handle owns no page-locked memory (only the per-agent handle has arenas), so its case proves that the counter counts on
the device figure and holds the page-locked one at the baseline throughout; the per-agent case sees both above the baseline."""
import ctypes as C
import dataclasses
import functools
import gc

import numpy as np
import pytest

from neptune_amd import abi, scene
from neptune_amd._lib import BackendError, check, lib
from gpu_util import _solver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from neptune_amd import backend
    return backend


def live():
    """(device bytes, page-locked bytes) held now; handles nobody refers to any more are destroyed first"""
    gc.collect()
    d, p = C.c_int64(-1), C.c_int64(-1)
    check(lib().nep_debug_live_bytes(C.byref(d), C.byref(p)))
    return d.value, p.value


@functools.lru_cache(maxsize=None)
def _scene(seed):
    return scene.make_scene(4, 2, seed=seed)


def test_batched_handle(be):
    """2 scenes x 4 agents, 2 static polygons, enable_entangle: the profile counters re-sized with the scratch, both
    replicate-and-swap paths of the per-scene statics, the active set, the fleet state and its tethers, the audit's partials, one
    eager tethered round of the fleet loop and one nep_batch_track_ent; then close()"""
    import torch
    base = live()
    scenes = [_scene(1), _scene(2)]
    p = dataclasses.replace(scenes[0]["par"], enable_entangle=True)
    S, N = 2, p.num_agents
    bb = be.BatchBackend(p, scenes[0]["statics"], n_scenes=S)
    dev = bb.device
    bb.debug_option("qp_profile", 1)
    bb.set_line_capacity(-1)
    reps = [scene.static_reps(sc["statics"]) for sc in scenes]
    bb.set_static_reps(*reps[0])
    for s, sc in enumerate(scenes):
        bb.set_scene_statics(s, sc["statics"])
    for s in range(S):
        bb.set_static_reps(*reps[s], scene=s)
    mask = torch.ones((S, N), dtype=torch.int32, device=dev)
    bb.set_active(mask)
    fe = scene.frontend_cfg(p, beam_width=8, pad_hold=1, entangle=True, ent_samples=3)
    lo = 6.5 * p.dc
    cfg = abi.nep_fleet_cfg(p.dc, p.T_span, lo, lo, 0.0, 1.0, 6, 5, 5, 0, fe.goal_size, 0.0)
    state0 = np.zeros((S, N, 12)); goals = np.zeros((S, N, 3))
    for s, sc in enumerate(scenes):
        state0[s, :, :2] = np.asarray(sc["starts"], dtype=np.float64)[:, :2]
        goals[s] = np.asarray(scene.reachable_goals(sc), dtype=np.float64).reshape(N, 3)
    state0[:, :, 2] = p.goal_height
    bb.fleet_init(cfg, torch.from_numpy(state0.reshape(-1)).to(dev), torch.from_numpy(goals.reshape(-1)).to(dev))
    bb.fleet_init_ent()
    n = S * N
    zeros = lambda size, t=torch.uint8: torch.zeros(size, dtype=t, device=dev)      # noqa: E731
    d_rec, d_final = zeros(n * abi.TRAJ_REC_DTYPE.itemsize), zeros(n * abi.TRAJ_REC_DTYPE.itemsize)
    d_start = zeros(n * abi.FE_START_DTYPE.itemsize)
    d_guess, d_res = zeros(n * abi.GUESS_DTYPE.itemsize), zeros(n * abi.FE_RESULT_DTYPE.itemsize)
    d_ent_a, d_ent = zeros(n * abi.FE_ENT_STATE_DTYPE.itemsize), zeros(n * abi.FE_ENT_STATE_DTYPE.itemsize)
    d_case = zeros(n * abi.NEP_MAX_POL * N, torch.int32)
    d_acc, d_flags = zeros(n, torch.int32), zeros(n, torch.int32)
    d_audit = bb.new_audit()
    bb.audit(d_rec, d_start, p.dc, 0, d_audit)
    # one eager round of the tethered fleet loop (neptune_amd.loop.DeviceFleetLoop._round_ops)
    bb.fleet_select(d_start, d_rec)
    bb.fleet_predict_ent(d_start, d_rec, d_ent_a)
    bb.frontend_ent(fe, d_rec, d_start, d_guess, d_res, d_case, d_ent_init=d_ent_a)
    bb.replan(None, d_guess, d_ent=d_case)
    bb.safety_commit_ent(d_rec, bb.d_commit, d_guess, d_final, d_acc, d_ent_init=d_ent_a)
    bb.fleet_commit(d_res, d_acc)
    bb.fleet_track_ent(d_rec, d_flags)
    bb.fleet_tick()
    bb.track_ent(d_rec, d_final, d_guess, d_ent)
    bb.check()
    held = live()
    print("batched handle: %d device bytes, %d page-locked" % (held[0] - base[0], held[1] - base[1]))
    assert held[0] > base[0] and held[1] == base[1], (base, held)
    bb.close()
    assert live() == base


def test_per_agent_handle(be):
    """PolySolver with 4 agents: one optimize(), generatePwpOut at the schedule's dc and at another one (the temporary buffers);
    both counts are above the baseline while the handle lives and back at it after close()"""
    base = live()
    sc = _scene(1)
    p = sc["par"]
    aid = 2
    hx, hn, h0, n0 = be.hulls_batch(sc["committed"], 0.0, p.num_pol, p.T_span, p.drone_radius)
    assert live() == base
    s = _solver(be, p, aid)
    s.setStaticObstVert(sc["statics"])
    g = sc["guesses"][aid - 1]; K = int(g["K"])
    s.setInitTrajectory(np.arange(K + 1) * p.T_span, np.array(g["coeff"])[:, :K, :])
    s.setHulls([[hx[j, i, :hn[j, i]] for i in range(p.num_pol)] for j in range(4) if j != aid - 1])
    s.optimize()
    _, _, traj = s.generatePwpOut(0.0, p.dc)
    _, _, traj2 = s.generatePwpOut(0.0, 0.7 * p.dc)
    assert len(traj) > 0 and len(traj2) > len(traj)
    held = live()
    print("per-agent handle: %d device bytes, %d page-locked" % (held[0] - base[0], held[1] - base[1]))
    assert held[0] > base[0] and held[1] > base[1], (base, held)
    s.close()
    assert live() == base


def test_failed_create(be):
    """nep_batch_create with a static polygon that is not convex returns NULL after its first allocations: nothing stays behind"""
    base = live()
    sc = _scene(1)
    dart = np.array([[20.0, 20.0], [22.0, 20.0], [20.5, 20.5], [20.0, 22.0]])
    with pytest.raises(BackendError, match="not convex"):
        be.BatchBackend(sc["par"], [sc["statics"][0], dart], n_scenes=2)
    assert live() == base


def test_stand_alone_calls(be):
    """separator_batch, gjk_batch and hulls_batch on three or four problems each"""
    base = live()
    sq = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    ok, _ = be.separator_batch([sq, sq + 5.0, sq[:3]], [sq + [3.0, 0.0], sq + [5.5, 5.5], sq + [0.0, 4.0]])
    assert ok.tolist() == [True, False, True]
    assert live() == base
    hit = be.gjk_batch([sq, sq + 5.0, sq[:3]], np.stack([sq + [3.0, 0.0], sq + [5.5, 5.5], sq + [0.0, 4.0]]))
    assert hit.tolist() == [False, True, False]
    assert live() == base
    sc = _scene(1)
    p = sc["par"]
    _, hn, _, _ = be.hulls_batch(sc["committed"], 0.0, p.num_pol, p.T_span, p.drone_radius)
    assert hn.max() >= 3
    assert live() == base
