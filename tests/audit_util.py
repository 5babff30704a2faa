"""Inputs of the flight-audit tests (tests/test_flight_audit_cpu.py, tests/test_gpu_flight_audit.py): a hand-made scene whose
every record meets one rule of include/neptune_frontend.h's nep_audit."""
import numpy as np

from neptune_amd import abi

HAND_RADIUS = 0.3
HAND_T0, HAND_TICK, HAND_TICKS = 0.0, 0.125, 49      # ticks at 0, 0.125 .. 6.0: dyadic, so every tick time is exact


def _rec(rid, segs, t0=0.0, bbox=(0.6, 0.6, 0.6), valid=1, is_agent=1):
    """segs: list of (duration, coeff [2][4]) with coeff in descending powers of u = t - knot"""
    r = np.zeros((), dtype=abi.TRAJ_REC_DTYPE)
    r["id"] = rid; r["is_agent"] = is_agent; r["valid"] = valid; r["n_bend"] = 1
    r["bbox"] = bbox
    r["pwp"]["n_seg"] = len(segs)
    t = t0
    r["pwp"]["times"][0] = t
    for i, (dur, co) in enumerate(segs):
        t += dur
        r["pwp"]["times"][i + 1] = t
        r["pwp"]["coeff"][0, i] = co[0]
        r["pwp"]["coeff"][1, i] = co[1]
        r["pwp"]["coeff"][2, i] = [0, 0, 0, 1.0]
    r["pos"] = [segs[0][1][0][3], segs[0][1][1][3], 1.0]
    return r


def _line(p, v):
    return [[0, 0, v[0], p[0]], [0, 0, v[1], p[1]]]


def _hover(p):
    return [(1000.0, _line(p, (0, 0)))]


def hand_scene():
    """-> (records [10] TRAJ_REC_DTYPE, statics (list of polygons), drone_radius).  Ids are 1-based positions.
      1, 2   straight lines that meet at (0, 0) at t = 4, a tick: box clearance -(0.3 + 0.3) there; 1 has two segments, the second
             one a true cubic in y
      3      invalid record hovering at the meeting point; 4: is_agent = 0 next to it — both ignored, both ways
      5      starts at t = 1 (u clamped before the first knot) and ends at t = 3, inside the window: rests at (10, 8)
      6      flies through polygon 0 (a square): centre at (-7, 6) at t = 3, signed distance -1
      7      hovers at (6, -6) between 8 at (5, -6) and 9 at (7, -6): two partners at exactly distance 1, the lower id wins
      8, 9   bbox 0.4 x 0.4 and 2.0 x 1.0: 7 is 0.5 outside 8's inflated box and 0.3 inside 9's, while 9 is 0.4 outside 7's
      10     hovers next to polygon 1, a clockwise triangle (the handle turns it counter-clockwise), and polygon 2 has five vertices"""
    recs = [
        _rec(1, [(4.0, _line((-4, 0), (1, 0))), (4.0, [[0, 0, 1, 0], [0.01, 0, 0, 0]])]),
        _rec(2, [(8.0, _line((0, -4), (0, 1)))]),
        _rec(3, _hover((0, 0)), valid=0),
        _rec(4, _hover((0.125, 0.125)), is_agent=0),
        _rec(5, [(2.0, [[-0.5, 1.5, 0, 8], [0, 0, 0, 8]])], t0=1.0),
        _rec(6, [(8.0, _line((-10, 6), (1, 0)))]),
        _rec(7, _hover((6, -6))),
        _rec(8, _hover((5, -6)), bbox=(0.4, 0.4, 0.4)),
        _rec(9, _hover((7, -6)), bbox=(2.0, 1.0, 0.6)),
        _rec(10, _hover((12, -11.5))),
    ]
    statics = [np.array([[-8.0, 5.0], [-6.0, 5.0], [-6.0, 7.0], [-8.0, 7.0]]),
               np.array([[11.0, -13.0], [12.0, -12.0], [13.0, -13.0]]),
               np.array([[-12.0, -12.0], [-10.0, -12.5], [-9.0, -11.0], [-10.5, -9.5], [-12.5, -10.5]])]
    return np.stack(recs), statics, HAND_RADIUS
