"""GPU: the list form of the tracked tether state (nep_ent_lists; include/neptune_frontend.h, include/neptune_fleet.h).
Between rounds (nep_batch_track_ent_lists) and in the device fleet loop (nep_batch_fleet_init_ent_lists, the list-form instantiation
of the step kernel behind nep_batch_fleet_track_ent / _predict_ent, the publish kernels) the device equals the host chain of
nep_ent_track_step / nep_ent_predict_a with state->cap = cap byte for byte, on lists of more than NEP_FE_ENT_CAP entries; a state at
point A that does not fit the fixed record holds its slot for the round.  The seeds come from tests/ent_lists_seeds.py (its
conditions are asserted in tests/test_ent_lists_cpu.py)."""
import dataclasses
import functools

import numpy as np
import pytest

import ent_lists_seeds as seeds
from neptune_amd import abi, entangle, scene
from neptune_amd._lib import BackendError
from neptune_amd.loop import ent_state_record
from test_gpu_fleet_loop import _np
from test_gpu_fleet_tether import TetherChain, _swap_goals
from test_gpu_tether_track import _bends, host_round

pytestmark = pytest.mark.gpu

CAP = seeds.CAP
HELD = abi.NEP_ENT_TRACK_HELD


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _empty_states(scenes, cap):
    return [[entangle.State(sc["par"].num_agents + len(seeds.reps_of(sc)[0]), cap=cap) for _ in range(sc["par"].num_agents)] for sc in scenes]


def run_rounds(torch, scenes, states, cap, n_iv, rounds, ns=3, absent=(), absent_from=0, proof=None):
    """run_rounds of tests/test_gpu_tether_track.py on the list form: `rounds` rounds of nep_batch_track_ent_lists against host_round on
    `states` (host states of capacity cap, updated), the nine-argument perturbation of d_prev as there"""
    from neptune_amd import dist as ndist
    from neptune_amd._lib import lib
    from neptune_amd.backend import BatchBackend
    p = dataclasses.replace(scenes[0]["par"], enable_entangle=True)
    S_, N = len(scenes), p.num_agents
    be = BatchBackend(p, scenes[0]["statics"], n_scenes=S_)
    if proof is not None:
        be.debug_option("fleet_ent_proof", proof)
    reps, longs = [], []
    for s, sc in enumerate(scenes):
        be.set_scene_statics(s, sc["statics"])
        r, l = seeds.reps_of(sc)
        be.set_static_reps(r, l, scene=s)
        reps.append(r); longs.append(l)
    com, gue = ndist.stack_scenes(scenes)
    recs = com.reshape(S_, N).copy(); prev = recs.copy()
    gue = gue.reshape(S_, N).copy()
    lists = be.new_ent_lists(cap, seeds.to_lists(states, cap))
    d_fl = torch.zeros(S_ * N, dtype=torch.int32, device=be.device)
    out = []
    rng = np.random.default_rng(7)
    for r in range(rounds):
        if r == absent_from:
            for s, a in absent:
                recs[s][a]["valid"] = 0
        changed = 0
        for s in range(S_):      # the previous check saw some tethers with a bend point more or less: the nine-argument form
            for j in range(N):
                nb = int(prev[s][j]["n_bend"])
                if rng.uniform() < 0.3 and len(reps[s]):
                    if nb > 1 and rng.uniform() < 0.5:
                        prev[s][j]["n_bend"] = nb - 1
                    elif 1 <= nb < abi.NEP_MAX_BEND:
                        prev[s][j]["bend"][nb] = reps[s][int(rng.integers(len(reps[s])))][int(rng.integers(2))]
                        prev[s][j]["n_bend"] = nb + 1
                changed += len(_bends(prev[s][j])) != len(_bends(recs[s][j]))
        d_prev = be.to_device(prev.reshape(-1)); d_rec = be.to_device(recs.reshape(-1)); d_g = be.to_device(gue.reshape(-1))
        be.track_ent_lists(d_prev, d_rec, d_g, lists, d_fl, n_intervals=n_iv, ent_samples=ns)
        rc = lib().nep_batch_check(be._h, torch.cuda.current_stream(be.device).cuda_stream)
        dev = lists.to_host()
        dev_rec = d_rec.cpu().numpy().view(abi.TRAJ_REC_DTYPE).reshape(S_, N)
        dev_fl = d_fl.cpu().numpy().reshape(S_, N)
        new_prev = recs.copy()
        host_fl = np.zeros((S_, N), dtype=np.int32)
        for s in range(S_):
            t0 = float(gue[s][0]["t_start"])
            host_fl[s] = host_round(p, reps[s], longs[s], prev[s], recs[s], t0, states[s], n_iv, ns, p.tether_length)
            for a in range(N):
                seeds.assert_lists_equal(dev, s * N + a, states[s][a], (r, s, a))
            assert np.array_equal(dev_fl[s], host_fl[s]), (r, s, dev_fl[s], host_fl[s])
            assert dev_rec[s].tobytes() == recs[s].tobytes(), (r, s)      # the published bend points, and nothing else in the record changed
        assert rc == (-4 if (dev_fl & abi.NEP_ENT_TRACK_CAP).any() else 0), (r, rc)      # (a capacity is raised through nep_batch_check too)
        out.append(dict(changed=changed, flags=dev_fl.copy(), host_flags=host_fl, n_alpha=dev.n_alpha.reshape(S_, N).copy(),
                        n_bend=dev.n_bend.reshape(S_, N).copy(), bytes=dev.tobytes() + dev_rec.tobytes() + dev_fl.tobytes()))
        prev = new_prev
        for s in range(S_):
            for a in range(N):
                gue[s][a]["t_start"] += n_iv * p.T_span
    be.close()
    return out


@pytest.mark.parametrize("n_iv", [1, 2])
def test_lists_above_the_fixed_record_equal_the_host_chain(torch, n_iv):
    """two seeded (20, 8) scenes, cap 112, 6 rounds: states, flags, published records and nep_batch_check against the host chain; some
    slot carries more than NEP_FE_ENT_CAP entries in every round (without the list form there is no such state on the device)"""
    scenes, states, kinds = seeds.seeded_scenes(cap=CAP)
    out = run_rounds(torch, scenes, states, CAP, n_iv, rounds=6)
    print("largest list per round", [int(o["n_alpha"].max()) for o in out], "changed", [o["changed"] for o in out])
    assert sum(o["changed"] for o in out) > 0
    above = np.all([o["n_alpha"] > abi.NEP_FE_ENT_CAP for o in out], axis=0)
    assert above.any(), "no slot stayed above NEP_FE_ENT_CAP entries"
    assert not any((o["flags"] & abi.NEP_ENT_TRACK_CAP).any() for o in out)


def test_the_capacity_itself(torch):
    """cap = the largest seeded count + 1: the host chain drops a move at the capacity (NEP_ENT_TRACK_CAP), the device drops the same
    moves and leaves the same states (run_rounds compares every state after every round)"""
    _, st0, _ = seeds.seeded_scenes(cap=CAP)
    cap = max(st.c.n_alpha for row in st0 for st in row) + 1
    scenes, states, _ = seeds.seeded_scenes(cap=cap)
    out = run_rounds(torch, scenes, states, cap, 1, rounds=6)
    n_cap = sum(int(((o["host_flags"] & abi.NEP_ENT_TRACK_CAP) != 0).sum()) for o in out)
    print("cap", cap, "moves dropped on the host, per round", [int(((o["host_flags"] & abi.NEP_ENT_TRACK_CAP) != 0).sum()) for o in out])
    assert n_cap >= 1, "the host chain never reached the capacity"
    assert max(int(o["n_alpha"].max()) for o in out) <= cap


@pytest.mark.parametrize("n,m", [(72, 8), (5, 0)])
def test_lane_edges(torch, n, m):
    """72 agents: two ballot words, the second one partial; 5 agents and no statics: one partial word, an empty statics mask"""
    scenes = [scene.tether_crossing_scene(n, m, 61)]
    out = run_rounds(torch, scenes, _empty_states(scenes, CAP), CAP, 2, rounds=3)
    assert sum(int((o["n_alpha"] > 0).sum()) for o in out) > 0, "no crossing was tracked"


def test_slot_without_a_trajectory(torch):
    """a seeded long slot stops publishing a trajectory after the first round: flags 0, lists and record as they are"""
    scenes, states, kinds = seeds.seeded_scenes(cap=CAP)
    a = kinds[0].index("long")
    out = run_rounds(torch, scenes, states, CAP, 2, rounds=3, absent=[(0, a)], absent_from=1)
    assert out[0]["n_alpha"][0, a] > abi.NEP_FE_ENT_CAP
    for o in out[1:]:
        assert o["flags"][0, a] == 0 and o["n_alpha"][0, a] == out[0]["n_alpha"][0, a] and o["n_bend"][0, a] == out[0]["n_bend"][0, a]


def test_proofs_on_equal_proofs_off(torch):
    res = []
    for proof in (1, 0):
        scenes, states, _ = seeds.seeded_scenes(cap=CAP)
        res.append([o["bytes"] for o in run_rounds(torch, scenes, states, CAP, 2, rounds=3, proof=proof)])
    assert res[0] == res[1]


# ---- the bulk-synchronous loop -----------------------------------------------------------------------------------------------------
def _tether_loop(graph, **kw):
    from neptune_amd.loop import TetherLoop
    scenes, states, kinds = seeds.seeded_scenes(cap=CAP)
    lp = TetherLoop(scenes, beam_width=8, n_intervals=2, graph=graph, ent_cap=CAP, ent_lists0=seeds.to_lists(states, CAP), **kw)
    return lp, scenes, states


def test_tether_loop_holds_what_does_not_fit_and_tracks_everybody(torch):
    """TetherLoop(ent_cap=112) on the seeded scenes, every second agent inactive by the caller's mask: each round the state at A is
    the list where it fits and zeros where it does not, the handle's mask is the caller's and the fit, a held slot comes out
    NEP_FE_SKIPPED, and the tracking of what the loop flew equals the host chain for every slot, held ones included"""
    N = 20
    active = (torch.arange(2 * N, device="cuda") % 2 == 0).to(torch.int32).reshape(2, N).contiguous()
    lp, scenes, states = _tether_loop(False, active=active)
    p = lp.p
    reps = [seeds.reps_of(sc) for sc in scenes]
    seen = {}
    orig = lp.be.track_ent_lists

    def spy(d_prev, d_records, d_guess, lists, *a, **k):
        seen.update(prev=d_prev.clone(), recs=d_records.clone(), guess=d_guess.clone())
        return orig(d_prev, d_records, d_guess, lists, *a, **k)
    lp.be.track_ent_lists = spy
    held_total = np.zeros(2 * N, dtype=np.int32)
    held_and_long = 0
    for r in range(5):
        n_before = np.array([st.c.n_alpha for row in states for st in row])
        lp.round()
        held = n_before > abi.NEP_FE_ENT_CAP
        held_total += held
        at_a = lp.d_ent.cpu().numpy().view(abi.FE_ENT_STATE_DTYPE)
        flat = [st for row in states for st in row]
        # (at_a was written before the tracking of this round: it shows the states as they were before host_round below)
        for i in range(2 * N):
            exp = np.zeros(1, dtype=abi.FE_ENT_STATE_DTYPE)[0] if held[i] else ent_state_record(flat[i])
            assert at_a[i].tobytes() == exp.tobytes(), ("state at A", r, i)
        assert (_np(lp.d_flags_a) == np.where(held, HELD, 0)).all(), r
        assert (_np(lp.d_mask).reshape(-1) == (_np(active).reshape(-1) != 0) & ~held).all(), r
        assert (_np(lp.d_held) == held_total).all(), r
        status = _np(lp.d_res, abi.FE_RESULT_DTYPE)["status"]
        assert (status[held] == 4).all() and (status[(_np(active).reshape(-1) != 0) & ~held] != 4).all(), r      # NEP_FE_SKIPPED
        held_and_long += int(held.sum())
        prev = seen["prev"].cpu().numpy().view(abi.TRAJ_REC_DTYPE).reshape(2, N).copy()
        recs = seen["recs"].cpu().numpy().view(abi.TRAJ_REC_DTYPE).reshape(2, N).copy()
        gue = seen["guess"].cpu().numpy().view(abi.GUESS_DTYPE).reshape(2, N)
        dev = lp.lists.to_host()
        for s in range(2):
            fl = host_round(p, reps[s][0], reps[s][1], prev[s], recs[s], float(gue[s][0]["t_start"]), states[s], 2, 3, p.tether_length)
            for a in range(N):
                seeds.assert_lists_equal(dev, s * N + a, states[s][a], (r, s, a))
            assert np.array_equal(_np(lp.d_flags).reshape(2, N)[s], fl), (r, s)
        assert lp.d_rec.cpu().numpy().tobytes() == recs.tobytes(), r      # the flown records with the published bend points
    rep = lp.report()
    assert held_and_long > 0 and sum(rep["held"]) == int(held_total.sum()) and max(rep["max_list"]) == max(st.c.n_alpha for row in states for st in row)
    lp.close()


def test_tether_loop_lists_graph_equals_eager(torch):
    res = []
    for graph in (True, False):
        lp, _, _ = _tether_loop(graph)
        rep = lp.run(8)
        res.append((rep, lp.lists.to_host().tobytes(), lp.d_rec.cpu().numpy().tobytes(), lp.d_ent.cpu().numpy().tobytes(), lp.d_flags.cpu().numpy().tobytes(),
                    lp.d_mask.cpu().numpy().tobytes(), lp.d_held.cpu().numpy().tobytes(), lp.d_start.cpu().numpy().tobytes()))
        assert sum(rep["held"]) > 0
        lp.close()
    assert res[0] == res[1]


# ---- the fleet ---------------------------------------------------------------------------------------------------------------------
class ListChain(TetherChain):
    """TetherChain with every tether's state in a host eu::ent_state of capacity `cap`, and the hold rule restated: a state at A of
    more than NEP_FE_ENT_CAP crossings gives a zeroed record, NEP_ENT_TRACK_HELD, one more held round and a cleared mask entry"""

    def __init__(self, loop, states):
        super().__init__(loop)
        self.ent = [st for row in states for st in row]
        self.held = np.zeros(self.S * self.N, dtype=np.int32)
        self.held_rounds = []

    def predict(self, m):
        lp, S, N, p = self.loop, self.S, self.N, self.loop.p
        got = _np(lp.d_ent_a, abi.FE_ENT_STATE_DTYPE); got_fl = _np(lp.d_flags_a)
        present = np.ones(N, dtype=np.int32)
        mask = np.ones((S, N), dtype=bool) if m is None else m.copy()
        zero = np.zeros(1, dtype=abi.FE_ENT_STATE_DTYPE)[0]
        held_now = np.zeros(S * N, dtype=bool)
        for s in range(S):
            sl = slice(s * N, (s + 1) * N)
            t0 = float(self.starts[s * N]["t_start"])
            pik = self.state[sl, :2].copy()
            pik1 = np.stack([entangle.sample_points(self.rec[s * N + j]["pwp"], t0, t0 + p.num_pol * p.T_span, p.num_pol, lp.ent_samples)[0, 0] for j in range(N)])
            for a in range(N):
                i = s * N + a
                out, fl = self.chk[i].predict_a(self.ent[i], pik[a], self.starts[i]["pos"][:2], pik, pik1, present, self.bends[sl])
                if out.c.n_alpha > abi.NEP_FE_ENT_CAP:
                    exp, fl = zero, fl | HELD
                    self.held[i] += 1; mask[s, a] = False; held_now[i] = True
                else:
                    exp = ent_state_record(out)
                assert got[i].tobytes() == exp.tobytes(), ("state at A", self.round, i, got[i]["n_alpha"], out.c.n_alpha)
                assert got_fl[i] == fl, ("flags at A", self.round, i, got_fl[i], fl)
        dev_mask = _np(lp.d_active if lp.masked else lp.d_hold).reshape(S, N)
        assert (dev_mask == mask.astype(np.int32)).all(), ("mask", self.round)
        self.held_rounds.append(held_now)
        self.compare_ent("predict")
        return mask

    def compare_ent(self, where):
        be = self.loop.be
        lists, held = be.fleet_ent_lists(self.loop.ent_cap)
        es = be.fleet_ent_state()
        for i in range(self.S * self.N):
            seeds.assert_lists_equal(lists, i, self.ent[i], (where, self.round, i))
            if self.ent[i].c.n_alpha <= abi.NEP_FE_ENT_CAP:
                assert es["state"][i].tobytes() == ent_state_record(self.ent[i]).tobytes(), (where, self.round, i)
            else:
                assert es["state"][i]["n_alpha"] == -1 and not es["state"][i].tobytes()[4:].strip(b"\0"), (where, self.round, i)
        assert (held == self.held).all(), (where, self.round, "held rounds")
        assert (es["ever"] == self.ever).all(), (where, self.round, "sticky flags")
        if where == "tick":
            assert (es["flags"] == self.flags_round).all(), (where, self.round, "round flags")


def _fleet_loop(scenes, **kw):
    from neptune_amd.loop import DeviceFleetLoop
    kw.setdefault("beam_width", 16)
    return DeviceFleetLoop(scenes, goals=_swap_goals(scenes), tethers=True, replan_every=5, **kw)


def _flight_bytes(loop, rounds):
    out = []
    for _ in range(rounds):
        loop.round()
        es = loop.be.fleet_ent_state()
        row = [es["state"].tobytes(), es["flags"].tobytes(), es["ever"].tobytes(), _np(loop.d_ent_a).tobytes(), _np(loop.d_flags_a).tobytes(), _np(loop.d_rec).tobytes()]
        if loop.ent_cap is not None:
            lists, held = loop.be.fleet_ent_lists(loop.ent_cap)
            row += [lists.tobytes(), held.tobytes()]
        out.append(row)
    st = loop.be.fleet_state()
    out.append([st["state"].tobytes(), st["pwp"].tobytes(), b"".join(p.tobytes() for p in loop.be.fleet_plans()), loop.be.fleet_counters()[0].tobytes()])
    return out


def test_fleet_flight_equals_the_host_chain_with_the_hold_rule(torch):
    """two seeded (20, 8) scenes, 10 eager rounds: after every predict, commit and track the lists, the states at A, both flag sets,
    the held counts, the mask, the published records and the counters equal the host chain's.  Then a re-seed with the short lists
    alone: nobody is held in the next round."""
    scenes, states, kinds = seeds.seeded_scenes(cap=CAP)
    loop = _fleet_loop(scenes, graph=False, ent_cap=CAP, ent_lists0=seeds.to_lists(states, CAP))
    host = ListChain(loop, states)
    state = {}

    def after_select(lp):
        state["m"] = host.predict(host.select())
    loop.after_select = after_select
    loop.after_commit = lambda lp: host.commit(state["m"])
    outcomes = []
    for _ in range(10):
        loop.round()
        outcomes.append(host.outcome.copy())
        host.tick()
    h0 = host.held_rounds[0]
    print("held per round", [int(h.sum()) for h in host.held_rounds], "largest list", host.seen["n_alpha"])
    assert h0.any() and not h0.all(), "round 0 needs held and planning slots"
    assert (outcomes[0][h0] == abi.NEP_FLEET_SKIPPED).all() and (outcomes[0][~h0] != abi.NEP_FLEET_SKIPPED).any()
    rep = loop.report()
    assert sum(r["held"] for r in rep) == int(host.held.sum()) and max(r["max_list"] for r in rep) == max(st.c.n_alpha for st in host.ent)
    loop.be.check()      # (a hold is no capacity)
    # re-seed with the short lists: nobody is held
    loop.after_select = loop.after_commit = None
    _, short, _ = seeds.seeded_scenes(cap=CAP, short_only=True)
    loop.be.fleet_init_ent_lists(CAP, host=seeds.to_lists(short, CAP))
    loop.round()
    assert not (_np(loop.d_flags_a) & HELD).any()
    assert (_np(loop.d_hold) == 1).all()
    assert not loop.be.fleet_ent_lists(CAP)[1].any()
    host.close(); loop.close()


def test_fleet_graph_equals_eager(torch):
    out = []
    for graph in (False, True):
        scenes, states, _ = seeds.seeded_scenes(cap=CAP)
        loop = _fleet_loop(scenes, graph=graph, ent_cap=CAP, ent_lists0=seeds.to_lists(states, CAP))
        out.append(_flight_bytes(loop, 10))
        assert (loop._g is not None) == graph
        assert loop.be.fleet_ent_lists(CAP)[1].any(), "nobody was ever held"
        loop.close()
    assert out[0] == out[1]


@functools.lru_cache(maxsize=None)
def _scene(n, m, seed):
    return scene.make_scene(n, m, seed=seed)


def test_no_drift_for_fleets_that_fit(torch):
    """four (16, 8) circle swaps, 10 rounds, empty seeds: ent_cap=112 leaves the bytes of ent_cap=None — the states as fixed records,
    the states at A, the flags, the records, the plan state and the counters — and holds nobody"""
    out = []
    for cap in (None, CAP):
        loop = _fleet_loop([_scene(16, 8, s) for s in (1, 2, 3, 4)], graph=False, ent_cap=cap)
        out.append([row[:6] for row in _flight_bytes(loop, 10)])
        if cap is not None:
            lists, held = loop.be.fleet_ent_lists(cap)
            assert not held.any() and lists.n_alpha.max() <= abi.NEP_FE_ENT_CAP
            assert all(r["held"] == 0 for r in loop.report())
        loop.close()
    assert out[0] == out[1]


def test_misuse(torch):
    from neptune_amd._lib import lib
    from neptune_amd.backend import BatchBackend
    L = lib()
    sc = scene.tether_crossing_scene(8, 6, 60)
    p = sc["par"]
    be = BatchBackend(p, sc["statics"])
    be.set_static_reps(*scene.static_reps(sc["statics"]))
    d_rec = be.to_device(sc["committed"]); d_g = be.to_device(sc["guesses"])
    import ctypes as C

    def track(b, lists):
        return L.nep_batch_track_ent_lists(b._h, d_rec.data_ptr(), d_rec.data_ptr(), d_g.data_ptr(), 1, 3, 10.0, C.byref(lists.c), None, None)
    good = be.new_ent_lists(CAP)
    for cap in (abi.NEP_FE_ENT_CAP, abi.NEP_ENT_LISTS_MAX_CAP + 1):      # cap out of range: NEP_E_CAP
        bad = be.new_ent_lists(CAP); bad.c.cap = cap
        assert track(be, bad) == -4
    assert L.nep_batch_track_ent_lists(be._h, d_rec.data_ptr(), d_rec.data_ptr(), d_g.data_ptr(), 0, 3, 10.0, C.byref(good.c), None, None) == -1
    assert track(be, good) == 0
    d_ent = torch.zeros(8 * abi.FE_ENT_STATE_DTYPE.itemsize, dtype=torch.uint8, device=be.device)
    d_mask = torch.zeros(8, dtype=torch.int32, device=be.device)

    def at_a(b, lists):
        return L.nep_batch_ent_lists_at_a(b._h, C.byref(lists.c), d_ent.data_ptr(), None, None, d_mask.data_ptr(), None, None)
    assert at_a(be, good) == 0 and (d_mask.cpu().numpy() == 1).all()
    bad = be.new_ent_lists(CAP); bad.c.cap = abi.NEP_FE_ENT_CAP
    assert at_a(be, bad) == -4
    assert L.nep_batch_ent_lists_at_a(be._h, C.byref(good.c), d_ent.data_ptr(), None, None, None, None, None) == -1
    big = be.new_ent_lists(abi.NEP_ENT_LISTS_MAX_CAP)      # the largest cap: 45 KB of LDS per slot
    assert track(be, big) == 0
    torch.cuda.synchronize()
    assert L.nep_batch_fleet_ent_lists(be._h, None, None) == -2      # the reader before any init
    be.close()
    be2 = BatchBackend(dataclasses.replace(p, enable_entangle=False), sc["statics"])
    assert track(be2, good) == -2 and at_a(be2, good) == -2
    be2.close()
    be3 = BatchBackend(p, sc["statics"], first_local=0, n_local=4)
    assert track(be3, good) == -2 and at_a(be3, good) == -2
    assert L.nep_batch_fleet_init_ent_lists(be3._h, 10.0, C.byref(abi.nep_ent_lists(CAP)), None) == -2
    be3.close()
    # the fleet: init on a handle without enable_entangle, cap out of range, the reader on a fixed-record handle, prediction without a mask
    from neptune_amd.loop import DeviceFleetLoop
    plain = DeviceFleetLoop([_scene(5, 0, 1)], tethers=False, graph=False)
    assert L.nep_batch_fleet_init_ent_lists(plain.be._h, 10.0, C.byref(abi.nep_ent_lists(CAP)), None) == -2
    plain.close()
    loop = DeviceFleetLoop([_scene(5, 0, 1)], tethers=True, graph=False)
    assert L.nep_batch_fleet_ent_lists(loop.be._h, None, None) == -2      # (on the fixed record)
    for cap in (abi.NEP_FE_ENT_CAP, abi.NEP_ENT_LISTS_MAX_CAP + 1):
        assert L.nep_batch_fleet_init_ent_lists(loop.be._h, 10.0, C.byref(abi.nep_ent_lists(cap)), None) == -4
    loop.be.fleet_init_ent_lists(CAP)
    loop.be.fleet_select(loop.d_start, loop.d_rec)
    with pytest.raises(BackendError):      # no mask registered: NEP_E_STATE
        loop.be.fleet_predict_ent(loop.d_start, loop.d_rec, loop.d_ent_a, loop.d_flags_a)
    loop.be.fleet_init_ent()              # back on the fixed record: the prediction needs no mask
    loop.be.fleet_predict_ent(loop.d_start, loop.d_rec, loop.d_ent_a, loop.d_flags_a)
    assert L.nep_batch_fleet_ent_lists(loop.be._h, None, None) == -2
    torch.cuda.synchronize()
    loop.close()
