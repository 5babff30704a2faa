// mission_host.cpp — host form of the fleet's mission controller (include/neptune_fleet.h: nep_mission_step, nep_mission_step_script).  No HIP call; built
// like plan_host.cpp (-O2 -ffp-contract=off).  A serial walk: agents in order, ticks in order, candidates k = 0, 1, 2, ... until one
// passes; the arithmetic is mission_common.h's, which the device form (fleet_mission_kernels.hip) shares, and the device equals a
// chain of these calls byte for byte.
#include <string>
#include <vector>

#include "mission_common.h"

namespace nep { void set_last_error(const std::string& msg); }

using namespace nep_mission_impl;

namespace {

MissionSlot slot_of(nep_mission_scene* sc, int a) {
  return MissionSlot{sc->goal + 3 * a, sc->done + a, sc->flags + a, sc->t_issue + a, sc->length + a, sc->completed + a, sc->counts + 4 * a, sc->sums + 2 * a};
}

// the serial rejection loop: the accepted candidate of lowest k, or -1
int draw(const nep_mission_cfg& c, const nep_mission_scene* sc, int a, const double* end_pos, const double* new_goal, const int* got, double& gx, double& gy) {
  const uint64_t h1 = mission_h1(c.seed, (uint64_t)((int64_t)sc->scene * sc->n_agents + a), (uint64_t)sc->counts[4 * a + kIssued]);
  for (int k = 0; k < c.max_attempts; k++) {
    double x, y;
    mission_candidate(c, h1, k, x, y);
    if (mission_accept(c, x, y, a, sc->n_agents, end_pos, sc->pb, sc->n_poly, sc->poly_off, sc->poly_xy, new_goal, got)) { gx = x; gy = y; return k; }
  }
  return -1;
}

// a scripted goal of agent a: row (issued - 1) mod n_goals of its table (k = 0: found)
int scripted(const nep_mission_scene* sc, int a, int n_goals, const double* script, double& gx, double& gy, double& gz) {
  const double* g = script + ((size_t)a * n_goals + mission_script_row(sc->counts[4 * a + kIssued], n_goals)) * 3;
  gx = g[0]; gy = g[1]; gz = g[2];
  return 0;
}

}  // namespace

extern "C" int nep_mission_step_script(const nep_mission_cfg* cfg, nep_mission_scene* sc, int32_t n_goals, const double* script) {
  if (!cfg || !sc) { nep::set_last_error("null argument"); return NEP_E_ARG; }
  const nep_mission_cfg& c = *cfg;
  if (!mission_cfg_ok(c)) { nep::set_last_error("bad mission configuration"); return NEP_E_ARG; }
  if (n_goals < 0 || (n_goals > 0 && !script)) { nep::set_last_error("bad script (n_goals >= 0, a table when n_goals > 0)"); return NEP_E_ARG; }
  const int N = sc->n_agents, T = sc->round_ticks;
  const bool scr = n_goals > 0;
  if (scr && N >= 1)
    for (size_t i = 0; i < (size_t)N * n_goals * 3; i++)
      if (!(script[i] - script[i] == 0.0)) { nep::set_last_error("a scripted goal is not finite"); return NEP_E_ARG; }
  if (N < 1 || T < 1 || sc->n_poly < 0 || !sc->pos || !sc->s_end || !sc->pb || (sc->n_poly > 0 && (!sc->poly_off || !sc->poly_xy)) || !sc->goal || !sc->done ||
      !sc->flags || !sc->t_issue || !sc->length || !sc->completed || !sc->counts || !sc->sums || !sc->scene_i || !sc->t_run || !sc->log_n || (c.log_cap > 0 && !sc->log)) {
    nep::set_last_error("bad mission scene"); return NEP_E_ARG;
  }
  if (sc->scene_i[kFinished]) return 0;
  const double t_end = mission_t_end(sc->t_now, sc->dc, T);
  std::vector<double> end_pos(3 * (size_t)N), new_goal(3 * (size_t)N, 0.0);
  std::vector<int> got(N, 0);
  const bool per_agent = c.mode == NEP_MISSION_PER_AGENT;
  // the ticks, and (mode PER_AGENT) the triggers
  bool all_completed = true;
  for (int a = 0; a < N; a++) {
    for (int i = 0; i < 3; i++) end_pos[3 * a + i] = sc->s_end[12 * a + i];
    if (per_agent && mission_quota_used(c, sc->counts + 4 * a)) continue;
    const double* p = sc->pos + (size_t)a * (T + 1) * 3;
    double len = sc->length[a]; int comp = sc->completed[a];
    for (int q = 1; q <= T; q++) mission_tick(c, p + 3 * (q - 1), p + 3 * q, sc->goal + 3 * a, len, comp);
    sc->length[a] = len; sc->completed[a] = comp;
    all_completed = all_completed && comp != 0;
    if (per_agent) got[a] = mission_agent_trigger(c, sc->s_end + 12 * a, sc->goal + 3 * a, t_end - sc->t_issue[a]);
  }
  if (per_agent) {
    bool fin = true;
    for (int a = 0; a < N; a++) {
      if (got[a] == NEP_MISSION_REACHED || got[a] == NEP_MISSION_TIMED_OUT) {
        const bool draws = mission_agent_draws(c, sc->counts + 4 * a);
        double gx = 0.0, gy = 0.0, gz = c.goal_z;
        const int k = !draws ? -1 : scr ? scripted(sc, a, n_goals, script, gx, gy, gz) : draw(c, sc, a, end_pos.data(), new_goal.data(), got.data(), gx, gy);
        mission_end_leg(c, slot_of(sc, a), c.log_cap > 0 ? sc->log + (size_t)a * c.log_cap : nullptr, sc->log_n + a, sc->scene * N + a, got[a], t_end, draws, scr, k, gx, gy, gz);
        got[a] = kNoNew;
        if (draws && k >= 0) { got[a] = kGotNew; new_goal[3 * a] = gx; new_goal[3 * a + 1] = gy; new_goal[3 * a + 2] = gz; }
      }
      fin = fin && mission_quota_used(c, sc->counts + 4 * a);
    }
    if (fin) sc->scene_i[kFinished] = 1;
    return 0;
  }
  const double el = t_end - *sc->t_run;
  if (!mission_run_over(c, all_completed, el)) return 0;
  double sum = 0.0;
  for (int a = 0; a < N; a++) sum = sum + sc->length[a];
  const bool draws = mission_run_draws(c, sc->scene_i);
  int attempts = 0;
  for (int a = 0; a < N; a++) {
    double gx = 0.0, gy = 0.0, gz = c.goal_z;
    const int k = !draws ? -1 : scr ? scripted(sc, a, n_goals, script, gx, gy, gz) : draw(c, sc, a, end_pos.data(), new_goal.data(), got.data(), gx, gy);
    attempts += mission_attempts(c, draws, scr, k);
    mission_end_run_slot(c, slot_of(sc, a), el, t_end, draws, k, gx, gy, gz);
    if (draws && k >= 0) { got[a] = kGotNew; new_goal[3 * a] = gx; new_goal[3 * a + 1] = gy; new_goal[3 * a + 2] = gz; }
  }
  mission_end_run(c, sc->scene_i, sc->t_run, sc->log, sc->log_n, sc->scene, all_completed, t_end, sum, N, attempts);
  return 0;
}

extern "C" int nep_mission_step(const nep_mission_cfg* cfg, nep_mission_scene* sc) {
  if (cfg && cfg->mode == NEP_MISSION_FLEET_TOGETHER) { nep::set_last_error("bad mission configuration (mode NEP_MISSION_FLEET_TOGETHER goes through nep_mission_step_script)"); return NEP_E_ARG; }
  return nep_mission_step_script(cfg, sc, 0, nullptr);
}
