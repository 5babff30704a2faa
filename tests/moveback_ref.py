"""Reference of the move-back rule (include/neptune_fleet.h: nep_batch_fleet_moveback / nep_moveback_step) in Python floats and
ints — it shares no code with neptune_amd/csrc/moveback_common.h.  The reference's rule (neptune_ros.cpp:1626-1636, 1291-1305): a
vehicle with a new goal plans towards (pb.x, pb.y, goal z) until it is strictly within the radius of its base or strictly older
than the timeout."""
import math

WAY_BACK = 16


def step(radius, timeout, state, pb, t_issue, t_first, t_now, flags, goals):
    """one call for n slots.  state [n][>= 2], pb [n][2], t_issue [n] or None, flags [n] ints, goals [n][3] (the goals the search
    was given by the select) -> (new flags, new goals, events): events[i] is a set out of {"set", "radius", "timeout"} — the bit was
    raised by this call, the radius test released it, the timer test released it"""
    out_f, out_g, events = [], [], []
    for i in range(len(flags)):
        t_iss = float(t_first) if t_issue is None else float(t_issue[i])
        f = int(flags[i]); ev = set()
        g = [float(goals[i][0]), float(goals[i][1]), float(goals[i][2])]
        if t_iss == float(t_now):
            f |= WAY_BACK; ev.add("set")
        if f & WAY_BACK:
            dx = float(state[i][0]) - float(pb[i][0]); dy = float(state[i][1]) - float(pb[i][1])
            d = math.sqrt(dx * dx + dy * dy)
            if d < float(radius):
                ev.add("radius")
            if float(t_now) - t_iss > float(timeout):
                ev.add("timeout")
            if ev & {"radius", "timeout"}:
                f &= ~WAY_BACK
        if f & WAY_BACK:
            g[0], g[1] = float(pb[i][0]), float(pb[i][1])
        out_f.append(f); out_g.append(g); events.append(ev)
    return out_f, out_g, events
