// mission_common.h — the arithmetic of the fleet's mission controller (include/neptune_fleet.h: nep_batch_fleet_mission), shared by
// its host form (mission_host.cpp) and its device form (fleet_mission_kernels.hip).  Both are built -ffp-contract=off, sqrt is the
// only library call, and every expression below is written once.  Nothing here depends on the order in which lanes run: a draw is
// "the accepted candidate of lowest k", which a serial rejection loop and a ballot over 64 candidates at a time both give.
#ifndef NEP_MISSION_COMMON_H_
#define NEP_MISSION_COMMON_H_

#include <math.h>
#include <stdint.h>

#include "../../include/neptune_fleet.h"

#ifndef NEP_MISSION_FN
#define NEP_MISSION_FN static inline
#endif

namespace nep_mission_impl {

// indices of a slot's counts and of a scene's integers
constexpr int kIssued = 0, kReached = 1, kTimedOut = 2, kNoGoal = 3;
constexpr int kRun = 0, kRunsOk = 1, kRunsFailed = 2, kFinished = 3;

NEP_MISSION_FN uint64_t mission_sm(uint64_t x) {      // the splitmix64 finaliser
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
NEP_MISSION_FN uint64_t mission_h1(uint64_t seed, uint64_t global_slot, uint64_t goal_index) {
  return mission_sm(mission_sm(seed ^ mission_sm(global_slot)) + goal_index);
}
NEP_MISSION_FN double mission_unit(uint64_t bits) { return (double)(bits >> 11) * 0x1.0p-53; }
// candidate k of a draw
NEP_MISSION_FN void mission_candidate(const nep_mission_cfg& c, uint64_t h1, int k, double& x, double& y) {
  const double ux = mission_unit(mission_sm(h1 + 2ull * (uint64_t)k)), uy = mission_unit(mission_sm(h1 + 2ull * (uint64_t)k + 1ull));
  x = c.lo[0] + (c.hi[0] - c.lo[0]) * ux;
  y = c.lo[1] + (c.hi[1] - c.lo[1]) * uy;
}

NEP_MISSION_FN double mission_norm2(double dx, double dy) { return sqrt(dx * dx + dy * dy); }
NEP_MISSION_FN double mission_norm3(double dx, double dy, double dz) { return sqrt((dx * dx + dy * dy) + dz * dz); }
NEP_MISSION_FN double mission_dist3(const double* a, const double* b) { return mission_norm3(a[0] - b[0], a[1] - b[1], a[2] - b[2]); }

// the end clock: round_ticks repeated additions, as nep_batch_fleet_tick advances it
NEP_MISSION_FN double mission_t_end(double t_now, double dc, int round_ticks) {
  double t = t_now;
  for (int k = 0; k < round_ticks; k++) t += dc;
  return t;
}

// mode FLEET_TOGETHER's test (auto_commands_together.py:160-164): inside the square of half side arrive_radius around the goal, x-y only
NEP_MISSION_FN bool mission_in_box(const nep_mission_cfg& c, const double* p, const double* goal) {
  const double dx = p[0] - goal[0], dy = p[1] - goal[1], rr = c.arrive_radius * c.arrive_radius;
  return dx * dx < rr && dy * dy < rr;
}

// one tick of one slot: the leg grows while the agent is not arrived; mode FLEET_RUNS re-evaluates `completed` (both directions),
// mode FLEET_TOGETHER only sets it
NEP_MISSION_FN void mission_tick(const nep_mission_cfg& c, const double* p_prev, const double* p, const double* goal, double& length, int& completed) {
  const double d = mission_dist3(p, goal), step = mission_dist3(p, p_prev);
  if (c.mode == NEP_MISSION_PER_AGENT) {
    if (d > c.arrive_radius) length = length + step;
  } else if (c.mode == NEP_MISSION_FLEET_RUNS) {
    if (!completed) length = length + step;
    completed = d < c.arrive_radius ? 1 : 0;
  } else {
    if (!completed) length = length + step;
    if (mission_in_box(c, p, goal)) completed = 1;
  }
}

// scripted goals: the row of a slot's table for the goal it is issued now (`issued` before the increment: the generator's goal index)
NEP_MISSION_FN int mission_script_row(int issued, int n_goals) { return (issued - 1) % n_goals; }
// the candidates a draw has examined, as a leg record states them: none without a draw and for a scripted goal
NEP_MISSION_FN int mission_attempts(const nep_mission_cfg& c, bool draws, bool scripted, int k_win) {
  return !draws || scripted ? 0 : (k_win >= 0 ? k_win + 1 : c.max_attempts);
}

// autoCMD's trigger on the end state (neptune_ros.cpp:1055-1066): 0 nothing, else NEP_MISSION_REACHED / NEP_MISSION_TIMED_OUT
NEP_MISSION_FN int mission_agent_trigger(const nep_mission_cfg& c, const double* s_end, const double* goal, double el) {
  if (el < c.min_interval) return 0;
  const double v_xy = mission_norm2(s_end[3], s_end[4]), a_xy = mission_norm2(s_end[6], s_end[7]);
  if ((el < c.timeout && v_xy > c.rest_v) || a_xy > c.rest_a) return 0;
  if (mission_dist3(s_end, goal) < c.arrive_radius) return NEP_MISSION_REACHED;
  if (el > c.timeout) return NEP_MISSION_TIMED_OUT;
  return 0;
}

// test 3: on or inside a counter-clockwise convex polygon of nv vertices
NEP_MISSION_FN bool mission_in_polygon(double x, double y, const double* xy, int nv) {
  bool inside = nv >= 1;
  for (int v = 0; v < nv; v++) {
    const int w = v + 1 == nv ? 0 : v + 1;
    const double ex = xy[2 * w] - xy[2 * v], ey = xy[2 * w + 1] - xy[2 * v + 1], wx = x - xy[2 * v], wy = y - xy[2 * v + 1];
    if (!(ex * wy - ey * wx >= 0.0)) inside = false;
  }
  return inside;
}

// The five tests on a candidate of agent a.  end_pos [N][3]: every agent's s_end position; new_goal [N][3] and got_new [N]: the
// goals drawn earlier in this call (got_new[j] == kGotNew; 0: nothing to do, NEP_MISSION_REACHED / _TIMED_OUT: a leg that ended
// and is not dealt with yet, kNoNew: dealt with, no new goal).
constexpr int kGotNew = 3, kNoNew = 4;
NEP_MISSION_FN bool mission_accept(const nep_mission_cfg& c, double x, double y, int a, int N, const double* end_pos, const double* pb,
                                   int n_poly, const int* poly_off, const double* poly_xy, const double* new_goal, const int* got_new) {
  bool ok = true;
  if (c.min_dist_self != 0.0) ok = ok && mission_norm2(x - end_pos[3 * a], y - end_pos[3 * a + 1]) >= c.min_dist_self;
  if (c.tether_max != 0.0) ok = ok && mission_norm2(x - pb[2 * a], y - pb[2 * a + 1]) <= c.tether_max;
  if (!ok) return false;
  for (int j = 0; j < n_poly; j++)
    if (mission_in_polygon(x, y, poly_xy + 2 * poly_off[j], poly_off[j + 1] - poly_off[j])) return false;
  if (c.close_pos != 0.0)
    for (int j = 0; j < N; j++)
      if (!(mission_norm3(x - end_pos[3 * j], y - end_pos[3 * j + 1], c.goal_z - end_pos[3 * j + 2]) >= c.close_pos)) return false;
  if (c.close_goal != 0.0)
    for (int j = 0; j < a; j++)
      if (got_new[j] == kGotNew && !(mission_norm3(x - new_goal[3 * j], y - new_goal[3 * j + 1], c.goal_z - new_goal[3 * j + 2]) >= c.close_goal)) return false;
  return true;
}

NEP_MISSION_FN bool mission_cfg_ok(const nep_mission_cfg& c) {
  if (c.mode != NEP_MISSION_PER_AGENT && c.mode != NEP_MISSION_FLEET_RUNS && c.mode != NEP_MISSION_FLEET_TOGETHER) return false;
  if (c.max_goals < 1 || c.log_cap < 0 || c.max_attempts < 64 || c.max_attempts > 4096 || c.max_attempts % 64 != 0) return false;
  if (!(c.hi[0] > c.lo[0]) || !(c.hi[1] > c.lo[1]) || !(c.arrive_radius > 0.0) || !(c.timeout > 0.0)) return false;
  if (!(c.min_interval >= 0.0) || !(c.rest_v >= 0.0) || !(c.rest_a >= 0.0)) return false;
  if (!(c.min_dist_self >= 0.0) || !(c.tether_max >= 0.0) || !(c.close_pos >= 0.0) || !(c.close_goal >= 0.0) || !(c.goal_z == c.goal_z)) return false;
  return true;
}

// a record into an owner's log: record i sits at i mod log_cap, the count runs on
NEP_MISSION_FN void mission_log(const nep_mission_cfg& c, nep_mission_leg* log, int* log_n, int who, int index, int outcome, int attempts,
                                double t_issue, double t_end, double length, double gx, double gy, double gz) {
  const int n = *log_n;
  if (c.log_cap > 0) {
    nep_mission_leg* r = log + n % c.log_cap;
    r->who = who; r->index = index; r->outcome = outcome; r->attempts = attempts;
    r->t_issue = t_issue; r->t_end = t_end; r->length = length; r->goal[0] = gx; r->goal[1] = gy; r->goal[2] = gz;
  }
  *log_n = n + 1;
}

// A slot's state behind pointers (host arrays or the handle's device buffers): what one thread updates when a leg ends.
struct MissionSlot { double* goal; int* done; int* flags; double* t_issue; double* length; int* completed; int* counts; double* sums; };

NEP_MISSION_FN bool mission_quota_used(const nep_mission_cfg& c, const int* counts) { return counts[kReached] + counts[kTimedOut] >= c.max_goals; }
// mode PER_AGENT: does the leg that ends now leave room for another one (is a goal drawn)?
NEP_MISSION_FN bool mission_agent_draws(const nep_mission_cfg& c, const int* counts) { return counts[kReached] + counts[kTimedOut] + 1 < c.max_goals; }

// the new leg of a slot: the goal drawn or scripted (k_win >= 0; gz: cfg.goal_z, or the table's) or, without one, the goal it has;
// returns true on the no-goal path
NEP_MISSION_FN bool mission_issue(const nep_mission_cfg& c, const MissionSlot& s, double t_end, int k_win, double gx, double gy, double gz) {
  const bool none = k_win < 0;
  if (none) { s.counts[kNoGoal] = s.counts[kNoGoal] + 1; *s.flags = *s.flags | NEP_FLEET_FLAG_GOAL; }
  else { s.goal[0] = gx; s.goal[1] = gy; s.goal[2] = gz; }
  s.counts[kIssued] = s.counts[kIssued] + 1;
  *s.t_issue = t_end; *s.length = 0.0; *s.completed = 0; *s.done = 0;
  return none;
}

// mode PER_AGENT: the leg of a slot ends with `outcome`; `draws`, k_win, (gx, gy, gz): the draw that followed, or (scripted, k_win = 0)
// the table's row.  Returns true on the no-goal path (the caller raises the handle's flag).
NEP_MISSION_FN bool mission_end_leg(const nep_mission_cfg& c, const MissionSlot& s, nep_mission_leg* log, int* log_n, int gslot, int outcome,
                                    double t_end, bool draws, bool scripted, int k_win, double gx, double gy, double gz) {
  const double el = t_end - *s.t_issue;
  const int index = s.counts[kIssued] - 1;
  const int which = outcome == NEP_MISSION_REACHED ? kReached : kTimedOut;
  s.counts[which] = s.counts[which] + 1;
  s.sums[0] = s.sums[0] + el; s.sums[1] = s.sums[1] + *s.length;
  const int attempts = mission_attempts(c, draws, scripted, k_win);
  mission_log(c, log, log_n, gslot, index, outcome, attempts, *s.t_issue, t_end, *s.length, s.goal[0], s.goal[1], s.goal[2]);
  if (!draws) return false;
  if (k_win < 0) mission_log(c, log, log_n, gslot, index + 1, NEP_MISSION_NO_GOAL, c.max_attempts, t_end, t_end, 0.0, s.goal[0], s.goal[1], s.goal[2]);
  return mission_issue(c, s, t_end, k_win, gx, gy, gz);
}

// modes FLEET_RUNS and FLEET_TOGETHER: a slot at the end of a run that took `el`
NEP_MISSION_FN bool mission_end_run_slot(const nep_mission_cfg& c, const MissionSlot& s, double el, double t_end, bool draws, int k_win, double gx, double gy, double gz) {
  const int which = *s.completed ? kReached : kTimedOut;
  s.counts[which] = s.counts[which] + 1;
  s.sums[0] = s.sums[0] + el; s.sums[1] = s.sums[1] + *s.length;
  if (!draws) return false;
  return mission_issue(c, s, t_end, k_win, gx, gy, gz);
}
// modes FLEET_RUNS and FLEET_TOGETHER: is the run over (all_completed: every slot's flag after the call's ticks)?
NEP_MISSION_FN bool mission_run_over(const nep_mission_cfg& c, bool all_completed, double el) { return all_completed || el > c.timeout; }
NEP_MISSION_FN bool mission_run_draws(const nep_mission_cfg& c, const int* scene_i) { return scene_i[kRun] + 1 < c.max_goals; }
// modes FLEET_RUNS and FLEET_TOGETHER: the scene's record and counters (length_sum: the slots' leg lengths summed in agent order)
NEP_MISSION_FN void mission_end_run(const nep_mission_cfg& c, int* scene_i, double* t_run, nep_mission_leg* log, int* log_n, int scene, bool success,
                                    double t_end, double length_sum, int N, int attempts) {
  mission_log(c, log, log_n, scene, scene_i[kRun], success ? NEP_MISSION_REACHED : NEP_MISSION_TIMED_OUT, attempts, *t_run, t_end,
              length_sum / (double)N, 0.0, 0.0, 0.0);
  scene_i[success ? kRunsOk : kRunsFailed] = scene_i[success ? kRunsOk : kRunsFailed] + 1;
  scene_i[kRun] = scene_i[kRun] + 1;
  if (scene_i[kRun] >= c.max_goals) scene_i[kFinished] = 1;
  *t_run = t_end;
}

}  // namespace nep_mission_impl
#endif  // NEP_MISSION_COMMON_H_
