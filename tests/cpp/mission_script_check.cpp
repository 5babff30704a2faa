// mission_script_check.cpp — stand-alone driver of the host forms nep_mission_step_script (neptune_amd/csrc/mission_host.cpp) and
// nep_effort_step (neptune_amd/csrc/effort_host.cpp), for a sanitizer build (tests/test_mission_script_cpu.py compiles the three
// with -fsanitize=address,undefined).  Seeded walks in the three modes with tables of 1 to 3 rows and a quota beyond them, and
// rings of every head and size, with every array sized exactly, so that a read or write past one is caught.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "neptune_fleet.h"

namespace nep { void set_last_error(const std::string&) {} }

namespace {
uint64_t g_s = 0x7654321ull;
double rnd() { g_s = g_s * 6364136223846793005ull + 1442695040888963407ull; return (double)(g_s >> 11) * (1.0 / 9007199254740992.0); }
double uni(double a, double b) { return a + (b - a) * rnd(); }

int walk(int mode, int S, int N, int T, int G, int calls) {
  nep_mission_cfg c{};
  c.mode = mode; c.max_goals = G + 3; c.max_attempts = 128; c.log_cap = 2; c.seed = 9;
  c.lo[0] = c.lo[1] = -9.0; c.hi[0] = c.hi[1] = 9.0; c.goal_z = 1.0; c.arrive_radius = 0.5;
  c.min_interval = mode == NEP_MISSION_PER_AGENT ? 0.5 : 0.0; c.timeout = 2.0; c.rest_v = 0.1; c.rest_a = 0.1;
  c.min_dist_self = mode == NEP_MISSION_PER_AGENT ? 3.0 : 0.0; c.tether_max = 14.0;
  const int n = S * N, owners = mode == NEP_MISSION_PER_AGENT ? n : S;
  std::vector<double> pb(2 * N, 0.0), goal(3 * n), t_issue(n, 0.0), length(n, 0.0), sums(2 * n, 0.0), t_run(S, 0.0), p(3 * n), script((size_t)n * G * 3);
  std::vector<int32_t> done(n, 1), flags(n, 0), completed(n, 0), counts(4 * n, 0), scene_i(4 * S, 0), log_n(owners, 0);
  std::vector<nep_mission_leg> log((size_t)owners * c.log_cap);
  for (int i = 0; i < n; i++) { for (int k = 0; k < 2; k++) { goal[3 * i + k] = uni(-8, 8); p[3 * i + k] = uni(-8, 8); } goal[3 * i + 2] = p[3 * i + 2] = 1.0; counts[4 * i] = 1; }
  for (double& v : script) v = uni(-8, 8);
  double t = 0.0;
  std::vector<double> pos((size_t)n * (T + 1) * 3), s_end((size_t)n * 12, 0.0);
  for (int r = 0; r < calls; r++) {
    for (int i = 0; i < n; i++) {
      double tgt[3] = {goal[3 * i], goal[3 * i + 1], goal[3 * i + 2]};
      if (rnd() < 0.3) for (int k = 0; k < 2; k++) tgt[k] = p[3 * i + k] + uni(-2, 2);
      for (int q = 0; q <= T; q++) for (int k = 0; k < 3; k++) pos[((size_t)i * (T + 1) + q) * 3 + k] = p[3 * i + k] + (tgt[k] - p[3 * i + k]) * q / T;
      for (int k = 0; k < 3; k++) { p[3 * i + k] = tgt[k]; s_end[(size_t)i * 12 + k] = tgt[k]; }
    }
    for (int s = 0; s < S; s++) {
      const int lo = s * N, o = mode == NEP_MISSION_PER_AGENT ? lo : s;
      nep_mission_scene sc{};
      sc.n_agents = N; sc.scene = s; sc.round_ticks = T; sc.n_poly = 0; sc.t_now = t; sc.dc = 0.1;
      sc.pos = pos.data() + (size_t)lo * (T + 1) * 3; sc.s_end = s_end.data() + (size_t)lo * 12; sc.pb = pb.data();
      sc.goal = goal.data() + 3 * lo; sc.done = done.data() + lo; sc.flags = flags.data() + lo; sc.t_issue = t_issue.data() + lo; sc.length = length.data() + lo;
      sc.completed = completed.data() + lo; sc.counts = counts.data() + 4 * lo; sc.sums = sums.data() + 2 * lo; sc.scene_i = scene_i.data() + 4 * s;
      sc.t_run = t_run.data() + s; sc.log = log.data() + (size_t)o * c.log_cap; sc.log_n = log_n.data() + o;
      if (nep_mission_step_script(&c, &sc, G, G ? script.data() + (size_t)lo * G * 3 : nullptr) != 0) { std::printf("nep_mission_step_script failed\n"); return 1; }
    }
    for (int q = 0; q < T; q++) t += 0.1;
  }
  int wrapped = 0;
  for (int i = 0; i < n; i++) {
    if (counts[4 * i + 3] != 0 && G) { std::printf("a scripted slot took the no-goal path\n"); return 1; }
    wrapped += counts[4 * i] > G + 1;
  }
  if (G && !wrapped) { std::printf("the table never wrapped\n"); return 1; }
  return 0;
}

int rings() {
  for (int cap = 1; cap <= 7; cap++)
    for (int head = 0; head < cap; head++)
      for (int size = 0; size <= cap; size++)
        for (int T : {1, 5, 9}) {
          std::vector<double> ring((size_t)cap * 12);
          for (double& v : ring) v = uni(-6, 6);
          nep_fleet_effort e{};
          if (nep_effort_step(2.0, 3.0, 5.0, 0.05, T, ring.data(), head, size, cap, 0, 1e-6, &e) != 0) return 1;
          if (e.n_ticks != (T < size ? T : size)) { std::printf("counted ticks\n"); return 1; }
          if (nep_effort_step(2.0, 3.0, 5.0, 0.05, T, ring.data(), head, size, cap, 1, 1e-6, &e) != 0 || e.n_ticks != (T < size ? T : size)) return 1;
        }
  nep_fleet_effort e{};
  double one[12] = {0};
  if (nep_effort_step(2.0, 3.0, 5.0, 0.05, 1, one, 1, 1, 1, 0, 0.0, &e) != NEP_E_ARG) return 1;      // head == cap
  if (nep_effort_step(2.0, 3.0, 5.0, 0.05, 1, one, 0, 1, 1, 0, -1.0, &e) != NEP_E_ARG) return 1;
  return 0;
}
}  // namespace

int main() {
  for (int mode : {NEP_MISSION_PER_AGENT, NEP_MISSION_FLEET_RUNS, NEP_MISSION_FLEET_TOGETHER})
    for (int G : {0, 1, 2, 3}) {
      if (walk(mode, 2, 5, 5, G, 80)) return 1;
      if (walk(mode, 2, 70, 1, G, 200)) return 1;
    }
  if (rings()) return 1;
  std::printf("mission_script_check ok\n");
  return 0;
}
