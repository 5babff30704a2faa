"""GPU: the post-solve safety pass (safety_conflict_kernel, safety_resolve_kernel, launch_safety) against the oracle beyond the one
shape the other tests compare it at (two scenes of 8 agents): several staging rounds and a partial last one, waves without an
agent, the ballot with idle lanes (num_pol 5 and 6), two, three and nine words per conflict row (the accepted set in LDS from
N > 256), both hull kernels under it, records that are invalid, no agents or short, scenes on their own clocks, active masks —
and gjk::collision on touching sets, equal centroids and hulls or quads that are points or segments.  The cases and what they
reach: safety_cases.py, test_safety_cases_cpu.py.  Verdicts are compared bit for bit; the expected values are the oracle's alone
(never the device's own conflict matrix)."""
import numpy as np
import pytest

import safety_cases as SC
from neptune_amd import abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from neptune_amd import backend
    return backend


def _handle(be, scs):
    """one handle of three scenes, each on its own clock: (handle, prev [S][N], fresh [S][N], d_prev, d_guess)"""
    p = scs[0]["par"]; S, N = len(scs), p.num_agents
    bb = be.BatchBackend(p, [], n_scenes=S)
    prev = np.stack([sc["prev"] for sc in scs]); fresh = np.stack([sc["fresh"] for sc in scs])
    gue = np.zeros((S, N), dtype=abi.GUESS_DTYPE)
    gue["K"] = p.num_pol
    for k, sc in enumerate(scs):
        gue[k]["t_start"] = sc["t_start"]
    return bb, prev, fresh, bb.to_device(prev), bb.to_device(gue)


def _commit(bb, d_prev, d_new, d_gue):
    """one safety_commit from sentinel-filled outputs -> (accept [S][N], final records [S][N])"""
    torch = bb.torch
    d_fin = torch.full_like(d_prev, 0x5A); d_acc = torch.full((bb.n_scenes * bb.N,), -7, dtype=torch.int32, device=bb.device)
    bb.safety_commit(d_prev, d_new, d_gue, d_fin, d_acc)
    bb.check()
    return d_acc.cpu().numpy().reshape(bb.n_scenes, bb.N), d_fin.cpu().numpy().view(abi.TRAJ_REC_DTYPE).reshape(bb.n_scenes, bb.N)


def _records_equal(got, want, what):
    g = got.view(np.uint8).reshape(len(got), -1); w = np.ascontiguousarray(want).view(np.uint8).reshape(len(want), -1)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert len(bad) == 0, (what, "agents", bad[:8].tolist())


@pytest.mark.parametrize("mode", [1, 2], ids=["hull_per_wave", "hulls_grouped"])
@pytest.mark.parametrize("key", list(SC.CONFIGS))
def test_conflicts_and_resolution_at_sizes(be, key, mode):
    """Three scenes per handle (other seeds, clocks 0, 1.5 and 3 intervals after their records'), the plain pass and the one with
    the previous-record check: both conflict matrices, the accept flags and every byte of the final records against the oracle.
    mode 2 is the eight-hulls-per-wave kernel the benchmark's sizes get (more than 2 048 records a launch).  Nothing the handle
    exposes tells which hull kernel a safety pass launched — nep_batch_debug_launch_path describes the last replan — so that it
    is in force rests on launch_safety reading the same hull_mode set_hull_kernel writes."""
    scs = SC.config(key)                                   # (the oracle's answers: once per configuration, not per hull kernel)
    bb, prev, fresh, d_prev, d_gue = _handle(be, scs)
    bb.set_hull_kernel(mode)
    d_new = bb.to_device(fresh)
    for check_prev in (False, True):
        bb.set_safety_check_prev(check_prev)
        acc, fin = _commit(bb, d_prev, d_new, d_gue)
        for k, sc in enumerate(scs):
            what = (key, mode, "check_prev" if check_prev else "plain", "scene %d" % k)
            np.testing.assert_array_equal(bb.debug_conflicts(k), sc["C"], err_msg=str(what))
            if check_prev:
                np.testing.assert_array_equal(bb.debug_conflicts_prev(k), sc["Cp"], err_msg=str(what))
            want = sc["accept_prev"] if check_prev else sc["accept"]
            np.testing.assert_array_equal(acc[k], want, err_msg=str(what))
            rec = prev[k].copy(); rec[want == 1] = fresh[k][want == 1]
            _records_equal(fin[k], rec, what)
    bb.close()


@pytest.mark.parametrize("key", list(SC.MASKED))
def test_resolution_with_active_masks_at_sizes(be, key):
    """nep_batch_set_active over more than one row word: scene 0 all active, scene 1 a random half, scene 2 the first 40 agents
    inactive (accepted-first bits in words 0 and 1; at N = 37 that is everybody).  Expected: the header's rule (safety_cases.resolve)
    on the oracle's matrices of the records the header defines — the previous record where inactive; the inactive agents' new
    records on the device are random bytes."""
    import torch
    scs, mcs = SC.config(key), SC.masked_config(key)
    bb, prev, fresh, d_prev, d_gue = _handle(be, scs)
    S, N = prev.shape
    mask = np.stack([mc["mask"] for mc in mcs])
    new = fresh.copy().view(np.uint8).reshape(S, N, -1)
    ina = mask == 0
    new[ina] = np.random.default_rng(1).integers(0, 256, new[ina].shape, dtype=np.uint8)
    d_new = bb.to_device(new.reshape(-1))
    d_mask = torch.from_numpy(mask).to(bb.device)
    bb.set_active(d_mask)
    for check_prev in (False, True):
        bb.set_safety_check_prev(check_prev)
        acc, fin = _commit(bb, d_prev, d_new, d_gue)
        for k, mc in enumerate(mcs):
            what = (key, "check_prev" if check_prev else "plain", "scene %d" % k)
            want = SC.resolve(mc["C"], mc["Cp"] if check_prev else None, mc["mask"])
            np.testing.assert_array_equal(bb.debug_conflicts(k), mc["C"], err_msg=str(what))
            if check_prev:
                np.testing.assert_array_equal(bb.debug_conflicts_prev(k), mc["Cp"], err_msg=str(what))
            np.testing.assert_array_equal(acc[k], want, err_msg=str(what))
            rec = prev[k].copy(); rec[want == 1] = mc["judged"][want == 1]
            _records_equal(fin[k], rec, what)
    bb.set_active(None)
    bb.close()


def test_gjk_degenerate_inputs(be, oracle):
    """gjk::collision on the 1/8 grid: shared vertices and edges, quads that are a point or a segment, equal centroids, boxes a grid
    step apart, touching and into each other, hulls of one to three vertices — the oracle's verdict on every case, and the exact
    integer verdict wherever intersecting and overlapping are the same answer."""
    polys, quads, verdict, decisive = SC.gjk_grid_cases(0)
    got = be.gjk_batch(polys, quads)
    want = np.array([oracle.gjk_collision(P, Q) for P, Q in zip(polys, quads)])
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[decisive], verdict[decisive])
