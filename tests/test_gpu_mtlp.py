"""GPU: the MTLP comparator (include/neptune_mtlp.h) on the device against its host form, on every byte — the directed worlds and the
seeded family of tests/mtlp_worlds.py (which tests/test_mtlp_cpu.py holds to the Python restatement of the reference), launches of
1, 5, 64 and 257 runs mixed over the worlds, eager and in a captured graph replayed twice, guard bytes round every output buffer, a
run whose robots mix the three outcomes, and the exact predicates' near-degenerate inputs through the debug entry point."""
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
