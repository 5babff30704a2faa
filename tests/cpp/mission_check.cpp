// mission_check.cpp — stand-alone driver of the host form of the fleet's mission controller (neptune_amd/csrc/mission_host.cpp:
// nep_mission_step), for a sanitizer build (tests/test_fleet_mission_cpu.py compiles both with -fsanitize=address,undefined).
// Seeded walks in both modes — 3 scenes, N = 5 and 70, round_ticks 1 and 5, 0 and 5 keep-out polygons of 3 to 8 vertices — with
// every array sized exactly, so that a read or write past one is caught; the accounting invariants are checked on the way.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "neptune_fleet.h"

namespace nep { void set_last_error(const std::string&) {} }

namespace {
uint64_t g_s = 0x1234567ull;
double rnd() { g_s = g_s * 6364136223846793005ull + 1442695040888963407ull; return (double)(g_s >> 11) * (1.0 / 9007199254740992.0); }
double uni(double a, double b) { return a + (b - a) * rnd(); }

int walk(int mode, int S, int N, int T, int n_poly, int calls) {
  nep_mission_cfg c{};
  c.mode = mode; c.max_goals = 3; c.max_attempts = 128; c.log_cap = 2; c.seed = 42 + (uint64_t)N;
  c.lo[0] = c.lo[1] = -9.0; c.hi[0] = c.hi[1] = 9.0; c.goal_z = 1.0; c.arrive_radius = 0.5;
  c.min_interval = mode == NEP_MISSION_PER_AGENT ? 0.5 : 0.0; c.timeout = 2.0; c.rest_v = 0.1; c.rest_a = 0.1;
  c.min_dist_self = mode == NEP_MISSION_PER_AGENT ? 3.0 : 0.0; c.tether_max = 14.0; c.close_pos = 0.5; c.close_goal = 1.0;
  const int n = S * N, owners = mode == NEP_MISSION_PER_AGENT ? n : S;
  std::vector<double> pb(2 * N), goal(3 * n), t_issue(n, 0.0), length(n, 0.0), sums(2 * n, 0.0), t_run(S, 0.0), p(3 * n);
  std::vector<int32_t> done(n, 1), flags(n, 0), completed(n, 0), counts(4 * n, 0), scene_i(4 * S, 0), log_n(owners, 0);
  std::vector<nep_mission_leg> log((size_t)owners * c.log_cap);
  for (int a = 0; a < N; a++) { pb[2 * a] = 10.0 * std::cos(6.283185307179586 * a / N); pb[2 * a + 1] = 10.0 * std::sin(6.283185307179586 * a / N); }
  for (int i = 0; i < n; i++) { goal[3 * i] = uni(-8, 8); goal[3 * i + 1] = uni(-8, 8); goal[3 * i + 2] = 1.0; p[3 * i] = uni(-8, 8); p[3 * i + 1] = uni(-8, 8); p[3 * i + 2] = 1.0; counts[4 * i] = 1; }
  std::vector<std::vector<int32_t>> off(S); std::vector<std::vector<double>> xy(S);
  for (int s = 0; s < S; s++) {
    off[s].assign(1, 0);
    for (int j = 0; j < n_poly; j++) {
      const int nv = 3 + (j + s) % 6;
      const double cx = uni(-7, 7), cy = uni(-7, 7), r = uni(0.8, 2.0);
      for (int v = 0; v < nv; v++) { xy[s].push_back(cx + r * std::cos(6.283185307179586 * v / nv)); xy[s].push_back(cy + r * std::sin(6.283185307179586 * v / nv)); }
      off[s].push_back(off[s].back() + nv);
    }
  }
  double t = 0.0;
  std::vector<double> pos((size_t)n * (T + 1) * 3), s_end((size_t)n * 12);
  for (int r = 0; r < calls; r++) {
    for (int i = 0; i < n; i++) {
      const double u = rnd();
      double tgt[3] = {goal[3 * i], goal[3 * i + 1], goal[3 * i + 2]};
      if (u < 0.3) for (int k = 0; k < 2; k++) tgt[k] = p[3 * i + k] + (tgt[k] - p[3 * i + k]) * 0.5;
      else if (u > 0.8) for (int k = 0; k < 2; k++) tgt[k] = p[3 * i + k] + uni(-2, 2);
      for (int q = 0; q <= T; q++) for (int k = 0; k < 3; k++) pos[((size_t)i * (T + 1) + q) * 3 + k] = p[3 * i + k] + (tgt[k] - p[3 * i + k]) * q / T;
      for (int k = 0; k < 12; k++) s_end[(size_t)i * 12 + k] = 0.0;
      for (int k = 0; k < 3; k++) { p[3 * i + k] = tgt[k]; s_end[(size_t)i * 12 + k] = tgt[k]; }
      if (rnd() < 0.2) s_end[(size_t)i * 12 + 3] = 0.5;
      if (rnd() < 0.1) s_end[(size_t)i * 12 + 7] = 0.5;
    }
    for (int s = 0; s < S; s++) {
      const int lo = s * N, o = mode == NEP_MISSION_PER_AGENT ? lo : s;
      nep_mission_scene sc{};
      sc.n_agents = N; sc.scene = s; sc.round_ticks = T; sc.n_poly = n_poly; sc.t_now = t; sc.dc = 0.1;
      sc.pos = pos.data() + (size_t)lo * (T + 1) * 3; sc.s_end = s_end.data() + (size_t)lo * 12; sc.pb = pb.data();
      sc.poly_off = off[s].data(); sc.poly_xy = xy[s].data();
      sc.goal = goal.data() + 3 * lo; sc.done = done.data() + lo; sc.flags = flags.data() + lo; sc.t_issue = t_issue.data() + lo; sc.length = length.data() + lo;
      sc.completed = completed.data() + lo; sc.counts = counts.data() + 4 * lo; sc.sums = sums.data() + 2 * lo; sc.scene_i = scene_i.data() + 4 * s;
      sc.t_run = t_run.data() + s; sc.log = log.data() + (size_t)o * c.log_cap; sc.log_n = log_n.data() + o;
      if (nep_mission_step(&c, &sc) != 0) { std::printf("nep_mission_step failed\n"); return 1; }
    }
    for (int q = 0; q < T; q++) t += 0.1;
    for (int i = 0; i < n; i++) {
      const int ended = counts[4 * i + 1] + counts[4 * i + 2];
      const int open = mode == NEP_MISSION_PER_AGENT ? (ended < c.max_goals) : (scene_i[4 * (i / N) + 3] == 0);
      if (counts[4 * i] != ended + open || ended > c.max_goals) { std::printf("accounting broken at slot %d\n", i); return 1; }
    }
  }
  int ended = 0;
  for (int i = 0; i < n; i++) ended += counts[4 * i + 1] + counts[4 * i + 2];
  if (ended == 0) { std::printf("the walk ended no leg\n"); return 1; }
  return 0;
}
}  // namespace

int main() {
  for (int T : {1, 5})
    for (int n_poly : {0, 5}) {
      if (walk(NEP_MISSION_PER_AGENT, 3, 5, T, n_poly, 60)) return 1;
      if (walk(NEP_MISSION_PER_AGENT, 3, 70, T, n_poly, 30)) return 1;
      if (walk(NEP_MISSION_FLEET_RUNS, 3, 5, T, n_poly, 80)) return 1;
    }
  nep_mission_cfg bad{};
  if (nep_mission_step(&bad, nullptr) != NEP_E_ARG) return 1;
  std::printf("mission_check ok\n");
  return 0;
}
