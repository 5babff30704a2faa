"""GPU: the span audit (nep_batch_audit_span) equals its host form (nep_span_audit_records) byte for byte — the
whole record, over accumulated calls, windows of 1, 5 and 37 ticks (37 ticks cross more knots than a record's staged pieces hold),
scenes with their own statics and clocks and more partners than a wave has lanes; captured and replayed it equals the eager call; it
runs inside DeviceFleetLoop's and TetherLoop's rounds without disturbing the flight or the tick audit, and the loops' buffers equal the
host chain over every round's records; and the handle contract."""
import dataclasses

import numpy as np
import pytest

from neptune_amd import abi, audit, scene
from neptune_amd._lib import BackendError

from span_audit_cases import RADIUS, TICK, big_scene, cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def first_difference(got, want):
    bad = [(a, f) for a in range(len(want)) for f in abi.SPAN_AUDIT_DTYPE.names if got[a][f].tobytes() != want[a][f].tobytes()]
    a, f = bad[0]
    return "%d fields differ, first agent %d %s device %r host %r" % (len(bad), a, f, got[a][f], want[a][f])


def device_equals_host(torch, par, recs, statics, clocks, tick, tick_counts, calls=2):
    """recs [S][N], statics [S] lists of polygons, clocks [S]: for every n_ticks of tick_counts, `calls` accumulated device calls (the
    clocks advanced by n_ticks*tick in between) against the same chain on the host"""
    from neptune_amd.backend import BatchBackend
    S, N = recs.shape
    be = BatchBackend(par, statics[0], n_scenes=S)
    for s in range(S):
        be.set_scene_statics(s, statics[s])
    d_rec = be.to_device(recs.reshape(-1))
    for n_ticks in tick_counts:
        d_span = be.new_span_audit()
        want = [audit.new_span_audit(N) for _ in range(S)]
        start = np.zeros((S, N), dtype=abi.FE_START_DTYPE)
        for c in range(calls):
            for s in range(S):
                start[s]["t_start"] = clocks[s] + c * n_ticks * tick
                start[s, 1:]["t_start"] += 100.0      # (a scene's clock is its FIRST slot's)
                audit.span_audit_records(recs[s], statics[s], par.drone_radius, float(start[s, 0]["t_start"]), tick, n_ticks, out=want[s])
            be.audit_span(d_rec, be.to_device(start.reshape(-1)), tick, n_ticks, d_span)
            be.check()
            got = d_span.cpu().numpy().view(abi.SPAN_AUDIT_DTYPE).reshape(S, N)
            for s in range(S):
                if got[s].tobytes() != want[s].tobytes():
                    pytest.fail("n_ticks %d call %d scene %d: %s" % (n_ticks, c, s, first_difference(got[s], want[s])))
        seen = got["n_spans"] > 0
        assert seen.any() and (got["n_spans"][seen] == calls).all()
    be.close()


def hand_par(n, n_static, radius):
    return dataclasses.replace(scene.scaled_params(n, n_static), drone_radius=radius)


def test_device_equals_host_directed_scene(torch):
    """the directed cases side by side in one scene, 40 m apart, with all their polygons: every rule at once, each pair still alone"""
    recs, statics = [], []
    for k, c in enumerate(cases()):
        shift = np.array([40.0 * (k % 4) - 60.0, 40.0 * (k // 4) - 40.0])
        for r in c["recs"]:
            r = r.copy()
            r["pwp"]["coeff"][0, :, 3] += shift[0]; r["pwp"]["coeff"][1, :, 3] += shift[1]
            r["id"] = len(recs) + 1
            recs.append(r)
        statics += [np.asarray(q, dtype=np.float64) + shift for q in c["statics"]]
    recs = np.stack(recs)
    device_equals_host(torch, hand_par(len(recs), len(statics), RADIUS), recs[None], [statics], [0.0], TICK, (1, 5, 37))


def test_device_equals_host_16_agents_own_statics_and_clocks(torch):
    scenes = [scene.make_scene(16, 4, seed=40 + s) for s in range(2)]
    p = scenes[0]["par"]
    recs = np.stack([sc["committed"] for sc in scenes])
    device_equals_host(torch, p, recs, [sc["statics"] for sc in scenes], [0.0, 0.33], p.dc, (1, 5, 37))


def test_device_equals_host_65_agents(torch):
    """more partners than a wave has lanes: 65 agents on the random splines of the config-5-size scene's generator"""
    recs, statics, radius, dc = big_scene(seed=3, n_agents=65, n_static=6)
    device_equals_host(torch, hand_par(65, len(statics), radius), recs[None], [statics], [0.1], dc, (1, 5, 37))


def test_device_equals_host_520_agents(torch):
    """more items than a wave sorts into kept and skipped (512: nobody is skipped then) and more than 64 KB of LDS (the launch's
    attribute, set by the first call)"""
    recs, statics, radius, dc = big_scene(seed=5, n_agents=520, n_static=4)
    device_equals_host(torch, hand_par(520, len(statics), radius), recs[None], [statics], [0.0], dc, (5,), calls=2)


def test_graph_equals_eager(torch):
    from neptune_amd.backend import BatchBackend
    sc = scene.make_scene(16, 4, seed=41)
    p = sc["par"]
    start = np.zeros(16, dtype=abi.FE_START_DTYPE)
    start["t_start"] = 0.2
    be = BatchBackend(p, sc["statics"])
    d_rec, d_start = be.to_device(sc["committed"]), be.to_device(start)
    d_eager, d_graph = be.new_span_audit(), be.new_span_audit()
    be.audit_span(d_rec, d_start, p.dc, 0, d_eager)      # the first call, with n_ticks = 0: nothing happens
    assert d_eager.cpu().numpy().tobytes() == audit.new_span_audit(16).tobytes()
    be.audit_span(d_rec, d_start, p.dc, 10, d_eager)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(be.device)
    s.wait_stream(torch.cuda.current_stream(be.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        be.audit_span(d_rec, d_start, p.dc, 10, d_graph, stream=s)
        g.capture_end()
    torch.cuda.current_stream(be.device).wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert d_graph.cpu().numpy().tobytes() == d_eager.cpu().numpy().tobytes()
    assert d_eager.cpu().numpy().tobytes() == audit.span_audit_records(sc["committed"], sc["statics"], p.drone_radius, 0.2, p.dc, 10).tobytes()
    be.close()


def test_span_audit_inside_the_device_fleet_loop(torch):
    from neptune_amd.loop import DeviceFleetLoop
    scenes = [scene.make_scene(8, 4, seed=50 + s) for s in range(2)]
    rounds = 10

    def fly(span):
        lp = DeviceFleetLoop(scenes, beam_width=16, audit=True, span_audit=span)
        chain = [audit.new_span_audit(lp.N) for _ in scenes] if span else None

        def host_chain(lp):      # between the commit and the tick of an eager round: the records and the clock the audits read
            rec = lp.d_rec.cpu().numpy().view(abi.TRAJ_REC_DTYPE).reshape(lp.S, lp.N)
            clock = lp.d_clock.cpu().numpy().view(abi.FE_START_DTYPE).reshape(lp.S, lp.N)["t_start"][:, 0]
            for s, sc in enumerate(scenes):
                audit.span_audit_records(rec[s], sc["statics"], lp.p.drone_radius, float(clock[s]), lp.p.dc, lp.replan_every, out=chain[s])
        if span:
            lp.after_commit = host_chain
        for _ in range(rounds):
            lp.round()
        torch.cuda.synchronize()
        st = lp.be.fleet_state(pwp=False)
        out = dict(state=st["state"].tobytes(), rec=lp.d_rec.cpu().numpy().tobytes(), audit=lp.audit_records().copy(),
                   span=lp.span_audit_records().copy() if span else None, chain=chain, report=lp.report())
        lp.close()
        return out

    on, off = fly(True), fly(False)
    for k in ("state", "rec"):
        assert on[k] == off[k], k
    assert on["audit"].tobytes() == off["audit"].tobytes()
    for s in range(len(scenes)):
        if on["span"][s].tobytes() != on["chain"][s].tobytes():
            pytest.fail("scene %d: %s" % (s, first_difference(on["span"][s], on["chain"][s])))
    assert (on["span"]["n_spans"] == rounds).all()
    for fv in ("min_center_dist", "min_box_clear", "min_static_dist"):      # over the same flight the span minima cannot lie above the ticks'
        assert (on["span"][fv] <= on["audit"][fv]).all(), fv
    assert "span_audit" in on["report"][0] and "span_audit" not in off["report"][0]
    with pytest.raises(ValueError):
        DeviceFleetLoop(scenes, span_audit=True)
    print(audit.format_span_summary([r["span_audit"] for r in on["report"]]))


def test_span_audit_inside_the_device_fleet_loop_graph(torch):
    """the same flight with the round captured (no hook): the replayed graph fills the buffer the eager chain fills"""
    from neptune_amd.loop import DeviceFleetLoop
    scenes = [scene.make_scene(8, 4, seed=50 + s) for s in range(2)]
    out = []
    for graph in (True, False):
        lp = DeviceFleetLoop(scenes, beam_width=16, audit=True, span_audit=True, graph=graph)
        for _ in range(10):
            lp.round()
        torch.cuda.synchronize()
        out.append((lp.span_audit_records().copy(), lp.audit_records().copy()))
        lp.close()
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()


def test_span_audit_inside_the_tether_loop(torch):
    from neptune_amd.loop import TetherLoop
    scenes = [scene.tether_crossing_scene(8, 4, 58)]
    rounds = 5

    def fly(span, graph):
        lp = TetherLoop(scenes, beam_width=8, audit=True, span_audit=span, graph=graph)
        chain = [audit.new_span_audit(lp.N) for _ in scenes] if span and not graph else None
        for _ in range(rounds):
            t = lp.d_start.cpu().numpy().view(abi.FE_START_DTYPE).reshape(lp.S, lp.N)["t_start"][:, 0].copy()
            lp.round()
            if chain is not None:
                rec = lp.d_rec.cpu().numpy().view(abi.TRAJ_REC_DTYPE).reshape(lp.S, lp.N)
                for s, sc in enumerate(scenes):
                    audit.span_audit_records(rec[s], sc["statics"], lp.p.drone_radius, float(t[s]), lp.p.dc, lp.audit_ticks, out=chain[s])
        torch.cuda.synchronize()
        out = dict(ent=lp.d_ent.cpu().numpy().tobytes(), rec=lp.d_rec.cpu().numpy().tobytes(), start=lp.d_start.cpu().numpy().tobytes(),
                   audit=lp.audit_records().copy(), span=lp.span_audit_records().copy() if span else None, chain=chain, report=lp.report())
        lp.close()
        return out

    g, e, plain = fly(True, True), fly(True, False), fly(False, True)
    for k in ("ent", "rec", "start"):
        assert g[k] == plain[k] and e[k] == plain[k], k
    assert g["audit"].tobytes() == plain["audit"].tobytes() and e["audit"].tobytes() == plain["audit"].tobytes()
    assert g["span"].tobytes() == e["span"].tobytes()
    assert e["span"].tobytes() == np.stack(e["chain"]).tobytes()
    assert (g["span"]["n_spans"] == rounds).all()
    for fv in ("min_center_dist", "min_box_clear", "min_static_dist"):
        assert (g["span"][fv] <= g["audit"][fv]).all(), fv
    assert "span_audit" in g["report"] and "span_audit" not in plain["report"]
    with pytest.raises(ValueError):
        TetherLoop(scenes, span_audit=True)


def test_handle_contract(torch):
    from neptune_amd.backend import BatchBackend
    sc = scene.make_scene(8, 4, seed=2)
    p = sc["par"]
    start = np.zeros(8, dtype=abi.FE_START_DTYPE)
    sharded = BatchBackend(p, sc["statics"], first_local=0, n_local=4)
    d_rec = sharded.to_device(sc["committed"])
    with pytest.raises(BackendError, match="-2"):      # NEP_E_STATE
        sharded.audit_span(d_rec, sharded.to_device(start), p.dc, 5, sharded.to_device(audit.new_span_audit(8)))
    sharded.close()
    be = BatchBackend(p, sc["statics"])
    d_rec, d_start = be.to_device(sc["committed"]), be.to_device(start)
    d_span = be.new_span_audit()
    with pytest.raises(BackendError):                  # NEP_E_ARG: a tick must be a finite number >= 0
        be.audit_span(d_rec, d_start, float("inf"), 5, d_span)
    with pytest.raises(BackendError):
        be.audit_span(d_rec, d_start, -p.dc, 5, d_span)
    be.audit_span(d_rec, d_start, p.dc, 0, d_span)     # the first call
    torch.cuda.synchronize()
    s = torch.cuda.Stream(be.device)
    s.wait_stream(torch.cuda.current_stream(be.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        be.audit_span(d_rec, d_start, p.dc, 40, d_span, stream=s)      # a second call under capture: nothing is allocated
        g.capture_end()
    torch.cuda.current_stream(be.device).wait_stream(s)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    want = audit.span_audit_records(sc["committed"], sc["statics"], p.drone_radius, 0.0, p.dc, 40)
    audit.span_audit_records(sc["committed"], sc["statics"], p.drone_radius, 0.0, p.dc, 40, out=want)
    assert d_span.cpu().numpy().tobytes() == want.tobytes()
    be.close()
