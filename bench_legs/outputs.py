"""--dump-outputs DIR: what the timed path handed back in its last timed step, as DIR/<name>.npy (float64), so that two builds
can be compared output for output.  The scenes are seeded, so the same arguments give the same inputs from run to run.

The arrays come from the handles' own output buffers, one row per replan slot of this process (scene-major, then local agent;
with --gpus N > 1 rank 0 writes its own agents' slots): the nep_solution records (coefficients, segment times, objective, status
and counts), the committed records' positions, and the sampled states.  The states are most of the bytes (83 x 12 doubles per
slot at the default sizes): when writing all of them would pass LIMIT, a fixed seeded sample of slots is written instead, and
`states_slot` holds the slot index of every row of `states`."""
import os

import numpy as np

LIMIT = 48 << 20          # bytes written at most (the headline's 8 192 slots carry ~73 MB, 65 MB of them sampled states)


def snapshot(bes):
    """the handles' outputs of their last replan, concatenated in scene-chunk order -> {name: float64 array}"""
    sol = np.concatenate([b.solutions() for b in bes])
    states = np.ascontiguousarray(np.concatenate([b.states() for b in bes]), dtype=np.float64)
    com = np.concatenate([b.commits() for b in bes])
    st = sol["stats"]
    arrays = {"coeff": sol["coeff"], "times": sol["times"], "objective": st["objective"], "status": st["status"], "iters": st["iters"],
              "n_lines": st["n_lines"], "n_rows": st["n_rows"], "K": sol["K"], "n_states": sol["n_states"], "commit_pos": com["pos"]}
    arrays = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
    slots = len(sol)
    idx = np.arange(slots)
    room = LIMIT - sum(v.nbytes for v in arrays.values()) - 8 * slots
    per_slot = states[0].nbytes + 8 if slots else 8
    if per_slot * slots > room:
        idx = np.sort(np.random.default_rng(0).choice(slots, size=max(room, 0) // per_slot, replace=False))
    arrays["states"] = states[idx]
    arrays["states_slot"] = idx.astype(np.float64)
    return arrays


def write(dirname, arrays):
    if not arrays:
        raise SystemExit("--dump-outputs: this run has no timed path whose outputs could be written")
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)
