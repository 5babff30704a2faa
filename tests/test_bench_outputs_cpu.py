"""bench.py --dump-outputs (bench_legs/outputs.py) without a GPU: the arrays of the handles' last replan, float64, one row per slot in
scene-chunk order; above the byte limit the states of a fixed seeded sample of slots, the same every time, and every other array whole."""
import numpy as np

from bench_legs import outputs
from neptune_amd import abi

MAX_STATES = 83


class _Handle:
    """what snapshot() reads of a BatchBackend: its output buffers as the host copies solutions() / states() / commits() return"""

    def __init__(self, slots, seed):
        rng = np.random.default_rng(seed)
        self.sol = np.zeros(slots, dtype=abi.SOLUTION_DTYPE)
        self.sol["coeff"] = rng.standard_normal(self.sol["coeff"].shape)
        self.sol["times"] = rng.standard_normal(self.sol["times"].shape)
        self.sol["K"] = 8
        self.sol["stats"]["status"] = rng.integers(0, 3, slots)
        self.sol["stats"]["objective"] = rng.standard_normal(slots)
        self.st = rng.standard_normal((slots, MAX_STATES, abi.NEP_STATE_DOUBLES))
        self.com = np.zeros(slots, dtype=abi.TRAJ_REC_DTYPE)
        self.com["pos"] = rng.standard_normal((slots, 3))

    def solutions(self):
        return self.sol.copy()

    def states(self):
        return self.st.copy()

    def commits(self):
        return self.com.copy()


def test_snapshot_is_every_slot_in_order_as_float64(tmp_path):
    hs = [_Handle(5, 1), _Handle(3, 2)]
    a = outputs.snapshot(hs)
    assert all(v.dtype == np.float64 and v.shape[0] == 8 for v in a.values())
    np.testing.assert_array_equal(a["states_slot"], np.arange(8))
    np.testing.assert_array_equal(a["coeff"], np.concatenate([h.sol["coeff"] for h in hs]))
    np.testing.assert_array_equal(a["status"], np.concatenate([h.sol["stats"]["status"] for h in hs]))
    np.testing.assert_array_equal(a["states"], np.concatenate([h.st for h in hs]))
    np.testing.assert_array_equal(a["commit_pos"], np.concatenate([h.com["pos"] for h in hs]))
    outputs.write(str(tmp_path / "d"), a)
    for k, v in a.items():
        b = np.load(tmp_path / "d" / (k + ".npy"))
        assert b.dtype == np.float64
        np.testing.assert_array_equal(b, v)


def test_snapshot_above_the_limit_samples_the_states_only(monkeypatch):
    monkeypatch.setattr(outputs, "LIMIT", 4 << 20)
    hs = [_Handle(400, 3), _Handle(400, 4)]
    a, b = outputs.snapshot(hs), outputs.snapshot(hs)
    n = len(a["states_slot"])
    assert 0 < n < 800 and len(a["states"]) == n and sum(v.nbytes for v in a.values()) <= 4 << 20
    assert np.all(np.diff(a["states_slot"]) > 0)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
        if k not in ("states", "states_slot"):
            assert a[k].shape[0] == 800, k
    np.testing.assert_array_equal(a["coeff"], np.concatenate([h.sol["coeff"] for h in hs]))
    full = np.concatenate([h.st for h in hs])
    np.testing.assert_array_equal(a["states"], full[a["states_slot"].astype(int)])
