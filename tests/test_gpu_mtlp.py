"""GPU: the MTLP comparator (include/neptune_mtlp.h) on the device against its host form, on every byte — the directed worlds and the
seeded family of tests/mtlp_worlds.py (which tests/test_mtlp_cpu.py holds to the Python restatement of the reference), launches of
1, 5, 64 and 257 runs mixed over the worlds, eager and in a captured graph replayed twice, guard bytes round every output buffer, a
run whose robots mix the three outcomes, and the exact predicates' near-degenerate inputs through the debug entry point; then the
wide worlds (five robots on the benchmark's grid, 16 and 64 robots, one robot, pools of thousands of nodes), one handle across
launches that grow and shrink, and the predicates over the whole stated domain."""
import numpy as np
import pytest
import torch

import mtlp_worlds as W
from neptune_amd import _lib, abi, mtlp

pytestmark = pytest.mark.gpu

GUARD = 0x5A


def _mixed(n):
    """n runs of two robots under one configuration: the two-robot directed worlds in turn (reached, budget and empty-list outcomes,
    coplanar lines, touches, the collinear triangle), each shifted by a multiple of 1/16 per round so that no two runs are the same"""
    base = [c for c in W.directed() if c["cfg"]["n_robots"] == 2]
    cfgd = W.cfg(max_pops=40, max_nodes=256, radius=0.25)
    b = np.zeros((n, 2, 3)); s = np.zeros((n, 2, 2, 3))
    for k in range(n):
        c = base[k % len(base)]
        shift = np.array([0.0625 * ((k // len(base)) % 5), 0.0625 * ((k // (5 * len(base))) % 5), 0.0])
        b[k] = np.array(c["bases"]) + shift; s[k] = np.array(c["sg"]) + shift
    return cfgd, b, s


@pytest.mark.parametrize("cases", [W.directed(), W.family()], ids=["directed", "family"])
def test_device_equals_host_on_every_world(cases):
    for cfgd, g in W.groups(cases):
        m = W.make_handle(cfgd)
        b, s = W.pack(g)
        want = m.solve(b, s, device=False)
        got = m.solve(b, s, device=True)
        diff = W.same_bytes(got, want)
        assert diff is None, ([c["name"] for c in g], diff)
        m.close()


@pytest.mark.parametrize("n", [1, 5, 64, 257])
def test_launch_sizes_eager_and_captured(n):
    cfgd, b, s = _mixed(n)
    m = W.make_handle(cfgd)
    want = m.solve(b, s, device=False)
    if n >= 64:
        assert {-1, 0, 1} <= set(want["result"]["status"].ravel().tolist())
    d_b, d_s = torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda()
    out = m.solve_device(d_b, d_s)      # eager: allocates
    torch.cuda.synchronize()
    assert W.same_bytes(m.from_device(out), want) is None
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            m.solve_device(d_b, d_s, out=out, stream=side.cuda_stream)
    for _ in range(2):
        out["result"].zero_(); out["path"].fill_(7.0); out["graph"].fill_(9); out["run_status"].fill_(9)
        graph.replay()
        torch.cuda.synchronize()
        diff = W.same_bytes(m.from_device(out), want)
        assert diff is None, diff
    m.close()


def _guarded(shape, dtype, pad=64):
    """a tensor of `shape` inside a buffer with `pad` guard bytes on either side"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 2 * pad,), GUARD, dtype=torch.uint8, device="cuda")
    return buf, buf[pad:pad + n].view(dtype).view(*shape)


def test_mixed_outcomes_and_flags_with_guard_bytes():
    d = {c["name"]: c for c in W.directed()}
    for name in ("mixed_outcomes", "path_cap", "rule6_pool_fills"):
        c = d[name]
        n, r = c["cfg"]["n_robots"], 3
        m = W.make_handle(c["cfg"])
        b, s = W.pack([c] * r)
        if name == "path_cap":
            s[2, 0, 0, 0] = np.nan      # ... and a run outside the domain
        want = m.solve(b, s, device=False)
        if name == "mixed_outcomes":
            assert set(want["result"]["status"][0].tolist()) == {-1, 0, 1}
        bufs, outs = zip(*[_guarded((r, n, n), torch.int32), _guarded((r,), torch.int32), _guarded((r * n * abi.MTLP_RESULT_DTYPE.itemsize,), torch.uint8),
                           _guarded((r, n, c["cfg"]["path_cap"], 3), torch.float64)])
        out = dict(graph=outs[0], run_status=outs[1], result=outs[2], path=outs[3])
        m.solve_device(b, s, out=out)
        torch.cuda.synchronize()
        diff = W.same_bytes(m.from_device(out), want)
        assert diff is None, (name, diff)
        for buf in bufs:
            assert (buf[:64] == GUARD).all() and (buf[-64:] == GUARD).all(), name
        if name == "path_cap":
            assert want["run_status"][2] == -2 and want["result"]["flags"][0, 0] & abi.NEP_MTLP_FLAG_PATH
            with pytest.raises(_lib.BackendError):
                m.check()
        assert m.check() == 0
        m.close()


def test_predicates_on_the_device_equal_the_host():
    which, rec = W.predicate_records()
    for w in (0, 1, 2):
        r = rec[which == w]
        vh, eh = mtlp.predicates(w, r, device=False)
        vd, ed = mtlp.predicates(w, r, device=True)
        assert (vh == vd).all() and (eh == ed).all(), w
        assert (eh > 0).sum() > len(r) // 4


# ---- past four robots and over the whole domain (W.wide(), W.predicate_records_wide(); tests/test_mtlp_wide_cpu.py holds the host
# form to the restatement on them) ---------------------------------------------------------------------------------------------------------
def _lattice64_runs():
    """lattice64 and two copies shifted by 1/16 and 2/16 in x: a graph launch of 12 288 entries (runs r > 0 at n = 64), 192 searches
    of up to 63 cable lines (27 passes of the wave per expansion)"""
    c = W.wide_case("lattice64")
    return c["cfg"], [c, W.shifted(c, 0.0625), W.shifted(c, 0.125)]


def test_device_equals_host_on_wide_worlds():
    for cfgd, g in W.groups(W.wide()):
        if g[0]["name"] == "lattice64":
            cfgd, g = _lattice64_runs()
        m = W.make_handle(cfgd)
        b, s = W.pack(g)
        want = m.solve(b, s, device=False)
        got = m.solve(b, s, device=True)
        diff = W.same_bytes(got, want)
        assert diff is None, ([c["name"] for c in g], diff)
        m.close()


def test_many_lines_with_guard_bytes():
    for name in ("lattice64", "one_robot_pool"):
        cfgd, g = _lattice64_runs() if name == "lattice64" else (W.wide_case(name)["cfg"], [W.wide_case(name)] * 3)
        n, r = cfgd["n_robots"], len(g)
        m = W.make_handle(cfgd)
        b, s = W.pack(g)
        want = m.solve(b, s, device=False)
        if name == "lattice64":
            assert set(want["result"]["status"].ravel().tolist()) == {-1, 0, 1} and (want["graph"][1] != want["graph"][1].T).any()
        else:
            assert (want["result"]["status"] == -1).all() and (want["result"]["nodes_used"] == 3000).all() and (want["result"]["pops"] == 3000).all()
        bufs, outs = zip(*[_guarded((r, n, n), torch.int32), _guarded((r,), torch.int32), _guarded((r * n * abi.MTLP_RESULT_DTYPE.itemsize,), torch.uint8),
                           _guarded((r, n, cfgd["path_cap"], 3), torch.float64)])
        out = dict(graph=outs[0], run_status=outs[1], result=outs[2], path=outs[3])
        m.solve_device(b, s, out=out)
        torch.cuda.synchronize()
        diff = W.same_bytes(m.from_device(out), want)
        assert diff is None, (name, diff)
        for buf in bufs:
            assert (buf[:64] == GUARD).all() and (buf[-64:] == GUARD).all(), name
        assert m.check() == 0
        m.close()


def test_one_handle_grows_and_shrinks():
    """one handle through launches of 3, 70 and 5 runs (its workspace grows once and is then reused by a smaller launch, over what
    other runs left in it), then the 70 again, captured — nothing is left to allocate — and replayed"""
    cfgd, b70, s70 = _mixed(70)
    m = W.make_handle(cfgd)
    want70 = m.solve(b70, s70, device=False)
    assert {-1, 0, 1} <= set(want70["result"]["status"].ravel().tolist())
    d_b, d_s = torch.from_numpy(b70).cuda(), torch.from_numpy(s70).cuda()
    out70 = None
    for lo, hi in ((20, 23), (0, 70), (10, 15)):
        out = m.solve_device(d_b[lo:hi].contiguous(), d_s[lo:hi].contiguous())
        torch.cuda.synchronize()
        got = m.from_device(out)
        diff = W.same_bytes(got, {k: v[lo:hi] for k, v in want70.items()})
        assert diff is None, (lo, hi, diff)
        if hi - lo == 70:
            out70 = out
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            m.solve_device(d_b, d_s, out=out70, stream=side.cuda_stream)
    out70["result"].zero_(); out70["path"].fill_(7.0); out70["graph"].fill_(9); out70["run_status"].fill_(9)
    graph.replay()
    torch.cuda.synchronize()
    diff = W.same_bytes(m.from_device(out70), want70)
    assert diff is None, diff
    m.close()


def test_predicates_wide_on_the_device_equal_the_host():
    which, rec, _ = W.predicate_records_wide()
    for w in (0, 1, 2):
        r = rec[which == w]
        vh, eh = mtlp.predicates(w, r, device=False)
        vd, ed = mtlp.predicates(w, r, device=True)
        assert (vh == vd).all() and (eh == ed).all(), (w, int((vh != vd).sum()), int((eh != ed).sum()))
        assert 4 * (eh > 0).sum() >= len(r)
