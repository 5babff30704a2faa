// moveback_check.cpp — stand-alone driver of the host form of the fleet loops' move-back rule (neptune_amd/csrc/moveback_host.cpp:
// nep_moveback_step), for a sanitizer build (tests/test_fleet_moveback_cpu.py compiles both with -fsanitize=address,undefined).
// Seeded walks — n = 1, 5 and 70 slots, with and without t_issue, radii below and above 0 — with every array sized exactly, so that
// a read or write past one is caught; the rule's invariants are checked on the way.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "neptune_fleet.h"

namespace nep { void set_last_error(const std::string&) {} }

namespace {
uint64_t g_s = 0x7654321ull;
double rnd() { g_s = g_s * 6364136223846793005ull + 1442695040888963407ull; return (double)(g_s >> 11) * (1.0 / 9007199254740992.0); }
double uni(double a, double b) { return a + (b - a) * rnd(); }

int walk(int n, bool with_issue, double radius, double timeout, int rounds) {
  const nep_moveback_cfg c{radius, timeout};
  std::vector<double> state(12 * (size_t)n), pb(2 * (size_t)n), t_issue(n, 0.0);
  std::vector<int32_t> flags(n);
  std::vector<nep_fe_start> start(n), before(n);
  for (int a = 0; a < n; a++) { pb[2 * a] = uni(-9, 9); pb[2 * a + 1] = uni(-9, 9); flags[a] = (int32_t)(rnd() * 16.0); }
  for (size_t i = 0; i < state.size(); i++) state[i] = uni(-9, 9);
  const std::vector<int32_t> sticky(flags);
  double t = 0.0;
  int sets = 0, by_radius = 0, by_timer = 0;
  for (int r = 0; r < rounds; r++) {
    for (int a = 0; a < n; a++) {
      for (int k = 0; k < 3; k++) { start[a].pos[k] = uni(-9, 9); start[a].vel[k] = uni(-1, 1); start[a].accel[k] = uni(-1, 1); start[a].goal[k] = uni(-9, 9); }
      start[a].t_start = t + 0.06;
      if (with_issue && rnd() < 0.15) t_issue[a] = t;                                     // a goal issued by the last call
      for (int k = 0; k < 2; k++) state[12 * (size_t)a + k] += 0.9 * (pb[2 * a + k] - state[12 * (size_t)a + k]) * rnd();      // drifts home
    }
    before = start;
    const std::vector<int32_t> f0(flags);
    if (nep_moveback_step(&c, n, state.data(), pb.data(), with_issue ? t_issue.data() : nullptr, 0.0, t, flags.data(), start.data()) != 0) { std::printf("nep_moveback_step failed\n"); return 1; }
    for (int a = 0; a < n; a++) {
      const double ti = with_issue ? t_issue[a] : 0.0;
      const bool on = (flags[a] & NEP_FLEET_FLAG_WAY_BACK) != 0, was = (f0[a] & NEP_FLEET_FLAG_WAY_BACK) != 0 || ti == t;
      if ((flags[a] & 15) != sticky[a]) { std::printf("a sticky bit moved at slot %d\n", a); return 1; }
      if (on && !was) { std::printf("slot %d is on its way back without a new goal\n", a); return 1; }
      const double d = std::hypot(state[12 * (size_t)a] - pb[2 * a], state[12 * (size_t)a + 1] - pb[2 * a + 1]);
      if (on && (t - ti > timeout || d < radius - 1e-9)) { std::printf("slot %d should have been released\n", a); return 1; }
      nep_fe_start want = before[a];
      if (on) { want.goal[0] = pb[2 * a]; want.goal[1] = pb[2 * a + 1]; }
      if (std::memcmp(&want, &start[a], sizeof want) != 0) { std::printf("slot %d: the start record differs from the rule's\n", a); return 1; }
      sets += ti == t; by_timer += was && !on && t - ti > timeout; by_radius += was && !on && !(t - ti > timeout);
    }
    for (int q = 0; q < 5; q++) t += 0.01;
  }
  if (sets == 0 || (radius > 0.0 ? by_radius == 0 : by_timer == 0)) { std::printf("the walk missed a path: %d set, %d by radius, %d by timer\n", sets, by_radius, by_timer); return 1; }
  return 0;
}
}  // namespace

int main() {
  for (int n : {1, 5, 70})
    for (bool with_issue : {false, true}) {
      if (walk(n, with_issue, 3.0, 0.4, 400)) return 1;
      if (walk(n, with_issue, 0.0, 0.2, 400)) return 1;
      if (walk(n, with_issue, -1.0, 0.0, 400)) return 1;
    }
  const nep_moveback_cfg bad{1.0, -1.0};
  double z[12] = {0}; int32_t f = 0; nep_fe_start s{};
  if (nep_moveback_step(&bad, 1, z, z, nullptr, 0.0, 0.0, &f, &s) != NEP_E_ARG) return 1;
  if (nep_moveback_step(nullptr, 1, z, z, nullptr, 0.0, 0.0, &f, &s) != NEP_E_ARG) return 1;
  std::printf("moveback_check ok\n");
  return 0;
}
