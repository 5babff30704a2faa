"""GPU: the fleet recorder (include/neptune_fleet.h "recorder", neptune_amd.loop.DeviceFleetLoop's recorder=, rewind, checkpoints).
A flight restored from a snapshot continues byte for byte like the flight the snapshot was taken from — plain, with timers,
tethered in both forms, with missions in both modes; one scene of a batch flown alone from the recorder's ring equals its part of
the batch, drawn goals and log included; the ring inside the captured round neither disturbs the flight nor records anything but
the state before the round; sizes that are no multiple of 16 bytes; and the calls' contracts."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from neptune_amd import abi, mission, scene
from neptune_amd._lib import BackendError

pytestmark = pytest.mark.gpu

BEAM, EVERY = 32, 5


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@functools.lru_cache(maxsize=None)
def _scene(n, m, seed, K=8):
    return scene.make_scene(n, m, seed=seed, K=K)


def _scenes():
    return [_scene(6, 3, 41), _scene(6, 3, 42), _scene(6, 3, 43)]


# short timeouts and a log of two records: a leg (a run) ends in every 0.25 s round, so the log has wrapped before round 5
AGENT = mission.MissionSpec("agent", goals=20, seed=3, min_interval=0.0, timeout=0.2, rest_v=100.0, rest_a=100.0, min_dist_self=3.0, log_cap=2)
RUNS = mission.MissionSpec("runs", goals=20, seed=3, timeout=0.2, log_cap=2)
KINDS = dict(plain=dict(), timers=dict(periods=3, phases=np.tile(np.arange(6, dtype=np.int32) % 3, (3, 1))), tethers=dict(tethers=True),
             lists=dict(tethers=True, ent_cap=48), agent=dict(missions=AGENT), runs=dict(missions=RUNS), agent_tethers=dict(missions=AGENT, tethers=True))


def _loop(kind, scenes=None, **kw):
    from neptune_amd.loop import DeviceFleetLoop
    o = dict(beam_width=BEAM, replan_every=EVERY, graph=False)
    o.update(KINDS[kind]); o.update(kw)
    return DeviceFleetLoop(_scenes() if scenes is None else scenes, **o)


def fingerprint(lp, scene_i=None):
    """the fleet state the readers give, and the round's outputs, as bytes per name; scene_i: that scene's part alone"""
    be, S, N = lp.be, lp.S, lp.N
    sl = (lambda a, per: a.reshape((S, per) + a.shape[1:])[scene_i]) if scene_i is not None else (lambda a, per: a)
    fs = be.fleet_state(pwp=True)
    cnt, t_now, rnd = be.fleet_counters()
    out = {"fleet_" + k: sl(v, N).tobytes() for k, v in fs.items()}
    plans = be.fleet_plans()
    out["plans"] = b"".join(p.tobytes() for p in (plans if scene_i is None else plans[scene_i * N:(scene_i + 1) * N]))
    out.update(counters=sl(cnt, 1).tobytes(), t_now=sl(t_now, 1).tobytes(), rounds=sl(rnd, 1).tobytes())
    if lp.tethers:
        es = be.fleet_ent_state(states=lp.ent_cap is None)
        out.update({"ent_" + k: sl(v, N).tobytes() for k, v in es.items() if v is not None})
        if lp.ent_cap is not None:
            lists, held = be.fleet_ent_lists(lp.ent_cap)
            out["held"] = sl(held, N).tobytes()
            for k in ("n_alpha", "n_bend", "id", "cs", "beta", "bend"):
                a = getattr(lists, k)
                out["lists_" + k] = sl(a.reshape(S * N, -1), N).tobytes()
    if lp.missions is not None:
        ms = be.fleet_mission_state()
        out.update({"mis_" + k: sl(v, 1 if k in ("scene", "t_run") else N).tobytes() for k, v in ms.items()})
        log, n = be.fleet_mission_log(ordered=False)
        per = N if lp.mission_cfg.mode == abi.NEP_MISSION_PER_AGENT else 1
        out.update(log=sl(log, per).tobytes(), log_n=sl(n, per).tobytes())
    # the round's outputs
    out["outcome"] = sl(lp.d_outcome.cpu().numpy(), N).tobytes()
    out["fe_result"] = sl(lp.d_res.cpu().numpy().view(abi.FE_RESULT_DTYPE), N).tobytes()
    out["solution"] = sl(be.solutions(), N).tobytes()
    return out


def same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k] == want[k], (what, k)


def fly(lp, rounds, scene_i=None):
    """`rounds` rounds, the fingerprint after each"""
    out = []
    for _ in range(rounds):
        lp.round()
        out.append(fingerprint(lp, scene_i))
    return out


@functools.lru_cache(maxsize=None)
def straight(kind):
    lp = _loop(kind)
    try:
        return fly(lp, 12)
    finally:
        lp.close()


# ---- 1. resume equals straight flight -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,graph", [("plain", False), ("timers", False), ("tethers", True), ("lists", False), ("agent", False), ("runs", False)])
def test_resume_equals_straight_flight(torch, kind, graph):
    want = straight(kind)
    if kind in ("agent", "runs"):      # legs (runs) ended and the log wrapped before the cut
        n = np.frombuffer(want[4]["log_n"], dtype=np.int32)
        assert (n > 2).all(), n
    lp = _loop(kind)
    try:
        first = fly(lp, 5)
        for r in range(5):
            same(first[r], want[r], (kind, "before the cut", r))
        blob = lp.be.fleet_snapshot()
        assert blob.numel() == lp.be.fleet_snapshot_bytes()
        host = blob.cpu().numpy().copy()
    finally:
        lp.close()
    del blob
    lp = _loop(kind, graph=graph)
    try:
        lp.be.fleet_restore(host)
        lp.rounds = 5
        for r in range(5, 12):
            lp.round()
            same(fingerprint(lp), want[r], (kind, "after the restore", r))
        assert lp._g is not None or not graph
    finally:
        lp.close()


# ---- 2. one scene alone -----------------------------------------------------------------------------------------------------------
def test_one_scene_alone(torch):
    lp = _loop("agent_tethers", recorder=4)
    try:
        batch = fly(lp, 9, scene_i=1)
        with pytest.raises(ValueError):
            lp.rewind(1, 2)       # overwritten
        with pytest.raises(ValueError):
            lp.rewind(1, 10)      # not flown yet
        with pytest.raises(ValueError):
            lp.rewind(1, 9)
        one = lp.rewind(1, 6)
        try:
            assert one.S == 1 and one.trace == [] and not one.graph and one.rounds == 6
            for r in range(6, 9):
                one.round()
                same(fingerprint(one), batch[r], ("scene 1 alone", r))
            assert len(one.trace) == 3
            log, n = one.be.fleet_mission_log()
            who = sorted({int(rec["who"]) for recs in log for rec in recs})
            assert who and who[0] >= lp.N and who[-1] < 2 * lp.N, who      # the batch's global slots, not the one-scene handle's
        finally:
            one.close()
    finally:
        lp.close()


# ---- 3. the recorder does not disturb the flight and records the right thing ------------------------------------------------------
def test_recorder_in_the_graph(torch):
    twin = _loop("agent", graph=False)
    snaps, want = {}, []
    try:
        for r in range(8):
            if r >= 5:
                snaps[r] = twin.be.fleet_snapshot().cpu().numpy().tobytes()
            twin.round()
            want.append(fingerprint(twin))
    finally:
        twin.close()
    lp = _loop("agent", graph=True, recorder=3)
    try:
        for r in range(8):
            lp.round()
            same(fingerprint(lp), want[r], ("recorder=3, graph", r))
        assert lp._g is not None
        be = lp.be
        stamps = be.snapshot_ring_stamps(lp.d_ring, 3)
        assert stamps["used"].all() and sorted(stamps["round"][:, 0].tolist()) == [5, 6, 7]
        for r in (5, 6, 7):
            assert (stamps["round"][r % 3] == r).all() and (stamps["origin"][r % 3] == np.arange(3)).all()
            assert be.snapshot_ring_entry(lp.d_ring, 3, r % 3).cpu().numpy().tobytes() == snaps[r], ("ring entry of round", r)
    finally:
        lp.close()


# ---- 4. shapes that can break the copy --------------------------------------------------------------------------------------------
def _round_trip(lp, check_layout):
    """two rounds, a snapshot; a third round moves the state; restored from device and from host memory it is the snapshot's again;
    then one block into the other scene"""
    be, S = lp.be, lp.S
    lp.round(); lp.round()
    blob = be.fleet_snapshot()
    host = blob.cpu().numpy().copy()
    info = check_layout(host)
    body = host[abi.NEP_SNAPSHOT_HDR_BYTES:].reshape(S, -1)
    for i, name in enumerate(abi.SNAPSHOT_SECTIONS):      # padding is zero
        b, at = info.bytes[i], info.offset[i]
        assert not body[:, at + b:at + (b + 15) // 16 * 16].any(), name
    assert (body[:, info.offset[0]:info.offset[0] + 4].view(np.int32).ravel() == np.arange(S)).all()      # origins
    assert (body[:, info.offset[1]:info.offset[1] + 4].view(np.int32).ravel() == 2).all()                 # round counters
    fp = fingerprint(lp)
    lp.round()
    moved = fingerprint(lp)
    print("N = %d, ring_cap %d: counters after 3 rounds" % (lp.N, be.fleet_ring_cap), be.fleet_counters()[0].tolist())
    assert moved["t_now"] != fp["t_now"] and moved["rounds"] != fp["rounds"] and moved["counters"] != fp["counters"]
    be.fleet_restore(blob)
    after_dev = be.fleet_snapshot().cpu().numpy()
    lp.round()
    be.fleet_restore(host)
    after_host = be.fleet_snapshot().cpu().numpy()
    assert after_dev.tobytes() == host.tobytes() and after_host.tobytes() == host.tobytes()
    got = fingerprint(lp)
    for k in fp:
        if k not in ("outcome", "fe_result", "solution"):      # (the round's outputs are the caller's buffers, not state)
            assert got[k] == fp[k], k
    # one block into another scene: scene 1 becomes what scene 0 was, the others stay
    be.fleet_restore(host, 0, 1)
    both = be.fleet_snapshot().cpu().numpy()[abi.NEP_SNAPSHOT_HDR_BYTES:].reshape(S, -1)
    assert both[1].tobytes() == body[0].tobytes()
    for s in range(S):
        if s != 1:
            assert both[s].tobytes() == body[s].tobytes()
    return fp, moved


def _describe(host):
    from neptune_amd._lib import lib
    info = abi.nep_fleet_snapshot_info()
    assert lib().nep_fleet_snapshot_describe(host.ctypes.data, host.size, C.byref(info)) == 0
    assert info.hdr.scene_bytes % 16 == 0 and abi.NEP_SNAPSHOT_HDR_BYTES + info.hdr.n_scenes * info.hdr.scene_bytes == host.size
    return info


def test_odd_sizes_round_trip(torch):
    """N = 70 (the per-slot int sections are 280 bytes: the 4-byte path, with padding; more than one wave of slots), timers, a
    tethered mission flight, two scenes; restore from host and from device memory"""
    sc = _scene(70, 2, 5, K=2)
    lp = _loop("agent_tethers", scenes=[sc, sc], periods=2, phases=np.tile(np.arange(70, dtype=np.int32) % 2, (2, 1)))
    try:
        def layout(host):
            info = _describe(host)
            assert info.hdr.N == 70 and info.hdr.n_scenes == 2 and info.hdr.timers == 1 and info.hdr.tether_form == 1 and info.hdr.mission_mode == abi.NEP_MISSION_PER_AGENT
            assert info.bytes[abi.SNAPSHOT_SECTIONS.index("head")] == 280 and info.bytes[abi.SNAPSHOT_SECTIONS.index("period")] == 280
            return info
        fp, moved = _round_trip(lp, layout)
        assert moved["plans"] != fp["plans"] and moved["fleet_pwp"] != fp["fleet_pwp"]      # plans were accepted: the rings and trajectories are in use
    finally:
        lp.close()


def test_small_ring_round_trip(torch):
    """ring_cap below the default (the capacity path raises sticky flags, which are state), the list form of the tethers with 41
    entries (the sign lists are 246 bytes a scene: the byte path; the ids 492: the 4-byte path), fleet-wide runs"""
    lp = _loop("lists", missions=RUNS, ring_cap=20, ent_cap=41)
    try:
        def layout(host):
            info = _describe(host)
            assert info.hdr.ring_cap == 20 == lp.be.fleet_ring_cap and info.hdr.tether_form == 2 and info.hdr.tether_cap == 41 and info.hdr.timers == 0
            assert info.bytes[abi.SNAPSHOT_SECTIONS.index("l_cs")] == 246 and info.bytes[abi.SNAPSHOT_SECTIONS.index("l_id")] == 492 and info.bytes[abi.SNAPSHOT_SECTIONS.index("log_n")] == 4
            return info
        _round_trip(lp, layout)
    finally:
        lp.close()


# ---- 5. contract ------------------------------------------------------------------------------------------------------------------
def test_before_init_and_sharded(torch):
    from neptune_amd._lib import lib
    from neptune_amd.backend import BatchBackend
    L = lib()
    sc = _scene(6, 3, 41)
    z = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    be = BatchBackend(sc["par"], sc["statics"])
    try:
        assert L.nep_batch_fleet_snapshot_bytes(be._h) == -2 and L.nep_batch_fleet_snapshot_ring_bytes(be._h, 2) == -2
        assert L.nep_batch_fleet_snapshot(be._h, z.data_ptr(), None) == -2 and b"nep_batch_fleet_init" in L.nep_last_error()
        assert L.nep_batch_fleet_snapshot_ring(be._h, z.data_ptr(), 2, None) == -2
        assert L.nep_batch_fleet_restore(be._h, z.data_ptr(), z.numel(), -1, -1) == -2
    finally:
        be.close()
    sh = BatchBackend(sc["par"], sc["statics"], first_local=0, n_local=3)
    try:
        assert L.nep_batch_fleet_snapshot(sh._h, z.data_ptr(), None) == -2 and b"unsharded" in L.nep_last_error()
        assert L.nep_batch_fleet_snapshot_bytes(sh._h) == -2
    finally:
        sh.close()


def _other_dc():
    return [dict(sc, par=dataclasses.replace(sc["par"], dc=0.04)) for sc in _scenes()]


MISMATCH = dict(other_N=("plain", {}, "plain", dict(scenes=[_scene(5, 3, 44)] * 3)),
                other_ring_cap=("plain", {}, "plain", dict(ring_cap=20)),
                other_tether_form=("plain", {}, "tethers", {}),
                lists_for_record=("tethers", {}, "lists", {}),
                other_capacity=("lists", {}, "lists", dict(ent_cap=56)),
                other_mission_mode=("agent", {}, "runs", {}),
                missions_for_none=("plain", {}, "agent", {}),
                other_dc=("plain", {}, "plain", dict(scenes=None)))


@pytest.mark.parametrize("case", sorted(MISMATCH))
def test_restore_refuses_another_state(torch, case):
    kind, kw, kind2, kw2 = MISMATCH[case]
    if case == "other_dc":
        kw2 = dict(scenes=_other_dc())
    src = _loop(kind2, **kw2)
    try:
        blob = src.be.fleet_snapshot().cpu().numpy().copy()
    finally:
        src.close()
    lp = _loop(kind, **kw)
    try:
        lp.round()
        before = lp.be.fleet_snapshot().cpu().numpy().tobytes()
        with pytest.raises(BackendError, match="error -1"):
            lp.be.fleet_restore(blob)
        with pytest.raises(BackendError, match="error -1"):
            lp.be.fleet_restore(blob, 0, 0)
        assert lp.be.fleet_snapshot().cpu().numpy().tobytes() == before
        good = np.frombuffer(before, dtype=np.uint8)
        for bad in (good[:-1], good[:abi.NEP_SNAPSHOT_HDR_BYTES]):      # truncated
            with pytest.raises(BackendError, match="error -1"):
                lp.be.fleet_restore(bad.copy())
        with pytest.raises(BackendError, match="error -1"):
            lp.be.fleet_restore(good, 3, 0)      # no such block
        with pytest.raises(BackendError, match="error -1"):
            lp.be.fleet_restore(good, 0, -1)
        assert lp.be.fleet_snapshot().cpu().numpy().tobytes() == before
    finally:
        lp.close()


def test_captured_ring_call_replays_and_restore_refuses_a_capture(torch):
    lp = _loop("plain")
    try:
        be = lp.be
        lp.round()
        ring = be.new_snapshot_ring(2)
        blob = be.fleet_snapshot()
        be.fleet_snapshot_ring(ring, 2)      # (the first call, eager)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            be.fleet_snapshot_ring(ring, 2)
            with pytest.raises(BackendError, match="error -2"):
                be.fleet_restore(blob)
        lp.round()
        want = be.fleet_snapshot().cpu().numpy().tobytes()
        g.replay()
        torch.cuda.synchronize()
        st = be.snapshot_ring_stamps(ring, 2)
        assert st["used"].all() and (st["round"][0] == 2).all() and (st["round"][1] == 1).all()
        assert be.snapshot_ring_entry(ring, 2, 0).cpu().numpy().tobytes() == want
        assert be.snapshot_ring_entry(ring, 2, 1).cpu().numpy().tobytes() == blob.cpu().numpy().tobytes()
        be.fleet_restore(blob)      # and outside a capture it goes through
        assert be.fleet_snapshot().cpu().numpy().tobytes() == blob.cpu().numpy().tobytes()
    finally:
        lp.close()


def test_checkpoint_file(torch, tmp_path):
    """save_checkpoint / resume: the audit buffer travels, the report at the end equals the uninterrupted flight's, and a file
    flown with other options is refused"""
    from neptune_amd.loop import DeviceFleetLoop
    path = str(tmp_path / "flight.npz")
    whole = _loop("agent", audit=True)
    try:
        for _ in range(8):
            whole.round()
        want = whole.report()
    finally:
        whole.close()
    lp = _loop("agent", audit=True)
    try:
        for _ in range(4):
            lp.round()
        lp.save_checkpoint(path)
    finally:
        lp.close()
    with pytest.raises(ValueError):
        DeviceFleetLoop.resume(path, _scenes(), replan_every=EVERY + 1)
    with pytest.raises(ValueError):
        DeviceFleetLoop.resume(path, [_scene(5, 3, 44)] * 3)
    lp = DeviceFleetLoop.resume(path, _scenes(), graph=False)
    try:
        assert lp.rounds == 4
        for _ in range(4):
            lp.round()
        assert lp.report() == want
    finally:
        lp.close()
