"""GPU: the writers of what a replan leaves behind (csrc/qp_outputs.h) — trajectory, sampled states, published record — one case per
kernel tail that calls them.  Every slot is checked by gpu_util.check_slot_outputs against the handle's own nep_solution, and every
case first proves that the tail it names wrote at least one slot.

Shapes: 2 scenes x 8 agents (slot / n_local and the scene stride of the previous records matter), as one handle over all agents and
as a shard with first_local = 4, n_local = 4 (own != slot); guesses of 3, 5 and 8 segments (the zero padding beyond K); a handle
created with max_states = 60 (the states buffer's rows per slot; scene.Params derives 83 by default), below the 81 samples that the
schedule of K = 8 holds at dc = 0.05 (the clamp) and above the 30 and 51 of K = 3 and 5."""
import dataclasses

import numpy as np
import pytest

import helpers  # noqa: F401
from neptune_amd import abi, scene
from gpu_util import check_slot_outputs
from test_gpu_robustness import _infeasible_guess

pytestmark = pytest.mark.gpu

S, N = 2, 8
KS = (8, 3, 5)                                   # agent a replans with KS[a % 3] segments
SHARDS = {"all": (0, 8), "shard": (4, 4)}        # first_local, n_local
MARK = 7.25                                      # z of the previous records' pos: no new record carries it


@dataclasses.dataclass
class _CappedParams(scene.Params):
    """scene.Params with a states buffer of 60 rows per slot instead of the derived ceil(num_pol T / dc) + 3"""
    max_states = 60


@pytest.fixture(scope="module")
def be():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from neptune_amd import backend
    return backend


@pytest.fixture(scope="module")
def world():
    """-> (params, statics per scene, guesses [S][N], previous records [S][N]); never modified by a case"""
    p = _CappedParams(**dataclasses.asdict(scene.scaled_params(N, 3)))
    scs = [scene.make_scene(N, 3, seed=11 + s, par=p) for s in range(S)]
    gue = np.stack([sc["guesses"] for sc in scs])
    for a in range(N):                           # the first K segments of the 8-segment guess
        K = KS[a % 3]
        gue["K"][:, a] = K
        gue["coeff"][:, a, :, K:, :] = 0.0
    prev = np.stack([sc["committed"] for sc in scs])
    prev["pos"][:, :, 2] = MARK
    return p, [sc["statics"] for sc in scs], gue, prev


def _handle(be, world, shard):
    p, statics, _, _ = world
    first, nl = SHARDS[shard]
    bb = be.BatchBackend(p, statics[0], first_local=first, n_local=nl, n_scenes=S)
    for s in range(1, S):
        bb.set_scene_statics(s, statics[s])
    return bb


def _replan_and_check(oracle, bb, gue, prev):
    """one replan of the handle's slots on gue [S][N] with prev [S][N] as d_committed, every slot through the shared checker
    -> (solutions [S][n_local], own index per local slot)"""
    own = np.arange(bb.first_local, bb.first_local + bb.n_local)
    bb.replan(bb.to_device(prev), bb.to_device(gue[:, own]))
    sol, states, com = bb.solutions().reshape(S, bb.n_local), bb.states().reshape(S, bb.n_local, bb.par.max_states, -1), bb.commits().reshape(S, bb.n_local)
    for s in range(S):
        for a, o in enumerate(own):
            check_slot_outputs(oracle, bb.par, int(o), gue[s, o], sol[s, a], states[s, a], com[s, a], prev=prev[s, o])
    assert (sol["n_states"][sol["K"] == 8] == 60).all() and set(np.unique(sol["K"])) - {0} == {3, 5, 8}      # (the clamp and the three K were there; 0: a skipped slot)
    return sol, own


@pytest.mark.parametrize("shard", list(SHARDS))
def test_presolved_slots_are_written_by_the_register_kernels_first_lines(be, oracle, world, shard):
    """the default handle: qp_presolve_kernel writes the trajectory of the replans it certifies (write_trajectory), qp_reg_kernel's
    first lines their states and record (write_states, write_commit)"""
    bb = _handle(be, world, shard)
    sol, _ = _replan_and_check(oracle, bb, world[2], world[3])
    assert bb.debug_launch_path()["presolve_kernel"] and bb.qp_kernel_name() == "qp_reg_kernel"
    assert ((sol["stats"]["status"] == abi.NEP_OK) & (sol["stats"]["iters"] == 0)).sum() >= 1
    bb.close()


@pytest.mark.parametrize("shard", list(SHARDS))
def test_register_kernel_tail_under_the_presolve(be, oracle, world, shard):
    """without the presolve kernel every slot goes through qp_reg_kernel<true>'s main tail"""
    bb = _handle(be, world, shard)
    bb.debug_option("presolve_kernel", 0)
    sol, _ = _replan_and_check(oracle, bb, world[2], world[3])
    assert not bb.debug_launch_path()["presolve_kernel"] and bb.qp_kernel_name() == "qp_reg_kernel" and bb.line_cull() == 4.0
    assert (sol["stats"]["status"] != abi.NEP_FAILED).sum() >= 1
    bb.close()


@pytest.mark.parametrize("shard", list(SHARDS))
def test_register_kernel_tail_with_every_row(be, oracle, world, shard):
    """line presolve off: qp_reg_kernel<false>"""
    bb = _handle(be, world, shard)
    bb.set_line_cull(0.0)
    sol, _ = _replan_and_check(oracle, bb, world[2], world[3])
    assert not bb.debug_launch_path()["presolve_kernel"] and bb.qp_kernel_name() == "qp_reg_kernel"
    assert (sol["stats"]["status"] != abi.NEP_FAILED).sum() >= 1
    bb.close()


@pytest.mark.parametrize("cull", [0.0, 4.0])
@pytest.mark.parametrize("shard", list(SHARDS))
def test_lds_kernel_tail(be, oracle, world, shard, cull):
    """qp_kernel<false> and qp_kernel<true>"""
    bb = _handle(be, world, shard)
    bb.debug_option("qp_kernel", 2)
    bb.set_line_cull(cull)
    sol, _ = _replan_and_check(oracle, bb, world[2], world[3])
    assert bb.qp_kernel_name() == "qp_kernel" and bb.line_cull() == cull and not bb.debug_launch_path()["presolve_kernel"]
    assert (sol["stats"]["status"] != abi.NEP_FAILED).sum() >= 1
    bb.close()


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("shard", list(SHARDS))
def test_failed_replan_keeps_the_previous_record(be, oracle, world, shard, kernel):
    """a start outside the world box fails both solves, on the register kernel (1) and the LDS kernel (2): the slot's record is the
    previous record of its (scene, agent), the solution returns the guess"""
    p, _, gue, prev = world
    gue = gue.copy()
    bad = [(0, 6), (1, 5)]                       # (scene, own): K = 8 and K = 5, both inside the shard
    for s, o in bad:
        gue[s, o] = _infeasible_guess(gue[s, o], p)
    bb = _handle(be, world, shard)
    bb.debug_option("qp_kernel", kernel)
    sol, own = _replan_and_check(oracle, bb, gue, prev)
    assert bb.qp_kernel_name() == ("qp_reg_kernel" if kernel == 1 else "qp_kernel")
    com = bb.commits().reshape(S, bb.n_local)
    for s, o in bad:
        a = int(o - own[0])
        assert int(sol[s, a]["stats"]["status"]) == abi.NEP_FAILED
        assert com[s, a].tobytes() == prev[s, o].tobytes() and com[s, a]["pos"][2] == MARK
        K = int(gue[s, o]["K"])
        np.testing.assert_array_equal(np.array(sol[s, a]["coeff"])[:, :K, :], np.array(gue[s, o]["coeff"])[:, :K, :])
    assert (sol["stats"]["status"] == abi.NEP_FAILED).sum() == len(bad)
    bb.close()


@pytest.mark.parametrize("shard", list(SHARDS))
def test_inactive_slots_keep_the_previous_record(be, oracle, world, shard):
    """an active set with inactive slots in both scenes: skipped_replan_kernel writes their outputs"""
    import torch
    mask = np.ones((S, N), dtype=np.int32)
    mask[0, [1, 5, 6]] = 0; mask[1, [4, 7]] = 0
    bb = _handle(be, world, shard)
    bb.set_active(torch.from_numpy(mask).to(bb.device))
    sol, own = _replan_and_check(oracle, bb, world[2], world[3])
    np.testing.assert_array_equal(sol["stats"]["status"] == abi.NEP_SKIPPED, mask[:, own] == 0)
    assert (sol["stats"]["status"] == abi.NEP_SKIPPED).sum() >= 2
    bb.close()


def test_polished_slots(be, oracle):
    """the polish pass's own tail: the slots it certified (bit 0x100 of their flag word), on the front-end guesses of
    test_gpu_presolve_polish.py's scenes, every row through the interior point"""
    from neptune_amd import dist as ndist
    Sp, Np = 4, 64
    scs = [scene.make_scene(Np, 20, seed=200 + s) for s in range(Sp)]
    p = scs[0]["par"]
    com, gue = ndist.stack_scenes(scs)
    prev = np.asarray(com).reshape(Sp, Np)
    bb = be.BatchBackend(p, scs[0]["statics"], n_scenes=Sp)
    for s in range(1, Sp):
        bb.set_scene_statics(s, scs[s]["statics"])
    d_com = bb.to_device(com); d_g = bb.to_device(gue)
    bb.frontend(scene.frontend_cfg(p, beam_width=32), d_com, bb.to_device(np.stack([scene.frontend_starts(s) for s in scs])), d_g, None)
    g = d_g.cpu().numpy().view(abi.GUESS_DTYPE).reshape(Sp, Np)
    bb.set_line_cull(0.0)
    bb.replan(d_com, d_g)
    assert bb.polish_count()[1] >= 1
    certified = np.flatnonzero(bb.polish_flags() & 0x100)
    assert len(certified) >= 1
    sol, states, rec = bb.solutions(), bb.states(), bb.commits()
    for slot in certified:
        s, a = divmod(int(slot), Np)
        assert int(sol[slot]["stats"]["status"]) in (abi.NEP_OK, abi.NEP_RELAXED)
        check_slot_outputs(oracle, p, a, g[s, a], sol[slot], states[slot], rec[slot], prev=prev[s, a])
    bb.close()
