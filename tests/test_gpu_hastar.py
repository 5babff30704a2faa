"""GPU: the homotopic grid A* (include/neptune_hastar.h) on the device against its host form, on every byte — the directed worlds and
the seeded family of tests/hastar_worlds.py (which tests/test_hastar_cpu.py holds to the Python restatement of the reference),
launches of 1, 5, 64 and 257 searches mixed across 3 scenes, eager and in a captured graph replayed twice, two chained searches that
stay on the device, and the capacity flags with guard words around every output buffer."""
import numpy as np
import pytest
import torch

import hastar_worlds as W
from neptune_amd import _lib, abi

pytestmark = pytest.mark.gpu

GUARD = 0x5A


def _mixed(n):
    """n searches over 3 scenes (one obstacle, three obstacles, 34 reps) with the default configuration: the directed cases' starts
    and goals, nudged per search so that no two are the same"""
    d = {c["name"]: c for c in W.directed()}
    base = [(0, d["obstacle_above"]), (1, d["inplace_update"]), (2, d["power_int_wraps"]), (0, d["cancel"]), (0, d["obstacle_below"])]
    worlds = [d["obstacle_above"]["world"], d["inplace_update"]["world"], d["power_int_wraps"]["world"]]
    cases, scenes = [], []
    for k in range(n):
        s, c = base[k % len(base)]
        dx, dy = 0.05 * ((k // 5) % 7), 0.04 * ((k // 35) % 9)
        cases.append(dict(c, start=(c["start"][0] + dx, c["start"][1] + dy), goal=(c["goal"][0] - dx, c["goal"][1] + dy),
                          cont0=[(c["start"][0] + dx, c["start"][1] + dy)]))
        scenes.append(s)
    return W.cfg(), worlds, cases, np.array(scenes, dtype=np.int32)


@pytest.mark.parametrize("cases", [W.directed(), W.family()], ids=["directed", "family"])
def test_device_equals_host_on_every_case(cases):
    for cfgd, g in W.groups(cases):
        ha = W.make_handle(cfgd, [c["world"] for c in g])
        start, goal, st = W.pack_inputs(ha, g)
        scene = np.arange(len(g), dtype=np.int32)
        want = ha.search(scene, start, goal, state=st, device=False)
        got = ha.search(scene, start, goal, state=st, device=True)
        diff = W.same_bytes(got, want)
        assert diff is None, ([c["name"] for c in g], diff)
        ha.close()


@pytest.mark.parametrize("n", [1, 5, 64, 257])
def test_launch_sizes_eager_and_captured(n):
    cfgd, worlds, cases, scene = _mixed(n)
    ha = W.make_handle(cfgd, worlds)
    start, goal, st = W.pack_inputs(ha, cases)
    want = ha.search(scene, start, goal, state=st, device=False)
    assert (want[0]["status"] == 1).sum() > 0.7 * n
    d_state = ha.to_device_state(st)
    d_scene, d_start, d_goal = torch.from_numpy(scene).cuda(), torch.from_numpy(start).cuda(), torch.from_numpy(goal).cuda()
    out = ha.search_device(d_scene, d_start, d_goal, d_state)      # eager: allocates and uploads
    torch.cuda.synchronize()
    assert W.same_bytes(ha.from_device(out), want) is None
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            ha.search_device(d_scene, d_start, d_goal, d_state, out=out, stream=side.cuda_stream)
    for _ in range(2):
        out["result"].zero_(); out["path"].fill_(7.0)
        for t in out["state"]:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        diff = W.same_bytes(ha.from_device(out), want)
        assert diff is None, diff
    assert ha.check() == 0
    ha.close()


def test_two_chained_searches_stay_on_the_device():
    cfgd, worlds, cases, scene = _mixed(64)
    ha = W.make_handle(cfgd, worlds)
    start, goal, st = W.pack_inputs(ha, cases)
    goal2 = np.ascontiguousarray(start + [0.1, -0.05])
    # host: the second search starts where the first path ends, from the first terminal state
    r1, p1, s1 = ha.search(scene, start, goal, state=st, device=False)
    ok = r1["status"] == 1
    assert ok.sum() > 40
    start2 = np.where(ok[:, None], p1[np.arange(64), np.maximum(r1["n_path"], 1) - 1], start)
    want = ha.search(scene, start2, goal2, state=s1, device=False)
    # device: nothing comes back in between
    d_scene = torch.from_numpy(scene).cuda()
    o1 = ha.search_device(d_scene, torch.from_numpy(start).cuda(), torch.from_numpy(goal).cuda(), ha.to_device_state(st))
    res = o1["result"].view(torch.int32).view(64, -1)
    last = (res[:, 1].clamp(min=1) - 1).long()
    d_start2 = torch.where((res[:, 0] == 1)[:, None], o1["path"][torch.arange(64, device="cuda"), last], torch.from_numpy(start).cuda()).contiguous()
    o2 = ha.search_device(d_scene, d_start2, torch.from_numpy(goal2).cuda(), o1["state"])
    torch.cuda.synchronize()
    diff = W.same_bytes(ha.from_device(o2), want)
    assert diff is None, diff
    assert (want[0]["status"] == 1).sum() > 40
    # ... and in place: the terminal state written over the initial one
    o3 = ha.search_device(d_scene, d_start2, torch.from_numpy(goal2).cuda(), o1["state"], d_state_out=o1["state"])
    torch.cuda.synchronize()
    assert W.same_bytes(ha.from_device(o3), want) is None
    ha.close()


def _guarded(shape, dtype, pad=64):
    """a tensor of `shape` inside a buffer with `pad` guard bytes on either side"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 2 * pad,), GUARD, dtype=torch.uint8, device="cuda")
    return buf, buf[pad:pad + n].view(dtype).view(*shape)


def test_caps_are_flagged_and_nothing_is_written_past_a_buffer():
    d = {c["name"]: c for c in W.directed()}
    for name, flag in (("cap_hsig", abi.NEP_HASTAR_FLAG_HSIG), ("cap_cont", abi.NEP_HASTAR_FLAG_CONT), ("cap_path", abi.NEP_HASTAR_FLAG_PATH),
                       ("cap_pool", abi.NEP_HASTAR_FLAG_POOL)):
        c = d[name]
        cases = [c, c, c]
        ha = W.make_handle(c["cfg"], [c["world"]])
        start, goal, st = W.pack_inputs(ha, cases)
        scene = np.zeros(3, dtype=np.int32)
        want = ha.search(scene, start, goal, state=st, device=False)
        with pytest.raises(_lib.BackendError):
            ha.check()      # the host form's flags
        d_state = ha.to_device_state(st)
        bufs, state = zip(*[_guarded(t.shape, t.dtype) for t in d_state])
        rbuf, result = _guarded((3 * abi.HASTAR_RESULT_DTYPE.itemsize,), torch.uint8)
        pbuf, path = _guarded((3, ha.cfg.path_cap, 2), torch.float64)
        out = dict(result=result, path=path, state=list(state))
        ha.search_device(scene, start, goal, d_state, out=out)
        torch.cuda.synchronize()
        got = ha.from_device(out)
        diff = W.same_bytes(got, want)
        assert diff is None, (name, diff)
        assert (got[0]["flags"] & flag).all(), name
        for b in list(bufs) + [rbuf, pbuf]:
            assert (b[:64] == GUARD).all() and (b[-64:] == GUARD).all(), name
        with pytest.raises(_lib.BackendError, match="capacity"):
            ha.check()
        assert ha.check() == 0
        ha.close()
