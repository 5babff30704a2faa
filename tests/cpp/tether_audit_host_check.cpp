// tether_audit_host_check.cpp — the tether audit's host form (include/neptune_entangle.h) as a stand-alone program, built from
// entangle_host.cpp alone with -fsanitize=address,undefined (tests/test_tether_audit_cpu.py): random walks of one vehicle among four
// others and three static representatives through nep_ent_track_step_audit next to nep_ent_track_step, with a roomy state and with
// one of four entries (moves dropped at the capacity), then the edges: the initial values, null arguments, a malformed state.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "neptune_entangle.h"

namespace {

int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

struct Rng {      // (a fixed sequence: the program's result does not depend on the machine)
  uint64_t s;
  double uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
  double sym(double a) { return (2.0 * uni() - 1.0) * a; }
};

struct Host {      // an eu::ent_state in arrays of `cap` entries
  std::vector<int32_t> alphas, bend, active; std::vector<double> betas; nep_ent_state c;
  Host(int cap, int n_active) : alphas(2 * cap), bend(cap), active(n_active), betas(cap) {
    c = nep_ent_state{0, 0, cap, n_active, alphas.data(), betas.data(), bend.data(), active.data()};
  }
  bool same(const Host& o) const {
    return c.n_alpha == o.c.n_alpha && c.n_bend == o.c.n_bend && alphas == o.alphas && bend == o.bend && active == o.active &&
           std::memcmp(betas.data(), o.betas.data(), betas.size() * sizeof(double)) == 0;
  }
};

void walk(uint64_t seed, int cap, int moves, int* dropped) {
  const int N = 5, S = 3;
  Rng r{seed};
  std::vector<double> pb(2 * N), rep(4 * S), lng(2 * S), pos(2 * N), nxt(2 * N);
  for (double& v : pb) v = r.sym(4.0);
  for (double& v : rep) v = r.sym(4.0);
  for (double& v : lng) v = 0.1 + 0.9 * r.uni();
  for (double& v : pos) v = r.sym(4.0);
  const nep_ent_cfg cfg{N, 1, 1, 1, 1.0, 12.0, S, 0, pb.data(), rep.data(), lng.data()};
  // every other agent publishes its base and up to two static representatives; the lists change now and then (the nine-argument form)
  std::vector<int32_t> off(N + 1), off_prev(N + 1), present(N, 1);
  std::vector<double> xy(2 * 3 * N), xy_prev(2 * 3 * N);
  auto publish = [&]() {
    int k = 0;
    for (int j = 0; j < N; j++) {
      off[j] = k;
      xy[2 * k] = pb[2 * j]; xy[2 * k + 1] = pb[2 * j + 1]; k++;
      const int extra = (int)(r.uni() * 3.0);
      for (int e = 0; e < extra; e++) { const int s = (int)(r.uni() * S), col = (int)(r.uni() * 2.0); xy[2 * k] = rep[(s * 2 + col) * 2]; xy[2 * k + 1] = rep[(s * 2 + col) * 2 + 1]; k++; }
    }
    off[N] = k;
  };
  publish();
  off_prev = off; xy_prev = xy;
  Host a(cap, N + S), b(cap, N + S);
  nep_tether_audit rec;
  CHECK(nep_tether_audit_init(&rec, 1) == NEP_OK);
  int n_drop = 0, ticks = 0;
  double longest = -INFINITY, sum = 0.0;
  for (int q = 1; q <= moves; q++) {
    for (int i = 0; i < 2 * N; i++) nxt[i] = pos[i] + r.sym(2.0);
    const nep_ent_track_inputs in{pos.data(), nxt.data(), present.data(), off.data(), xy.data(), off_prev.data(), xy_prev.data()};
    const int fa = nep_ent_track_step_audit(&cfg, &in, &a.c, &pos[0], &nxt[0], 0.05 * q, &rec);
    const int fb = nep_ent_track_step(&cfg, &in, &b.c, &pos[0], &nxt[0]);
    CHECK(fa >= 0 && fa == fb && a.same(b));
    double len = -1.0;
    CHECK(nep_ent_tether_length(&cfg, &a.c, &nxt[0], &len) == NEP_OK && len >= 0.0);
    CHECK(rec.last_len == len);
    if (fa & NEP_ENT_TRACK_CAP) n_drop++;
    else CHECK(((fa & NEP_ENT_TRACK_TOO_LONG) != 0) == (len > cfg.cable_length));
    ticks++; sum = sum + len; if (len > longest) longest = len;
    CHECK(a.c.n_alpha <= cap && rec.max_alpha <= cap && rec.max_bend <= NEP_MAX_BEND - 1);
    pos = nxt;
    off_prev = off; xy_prev = xy;
    if (r.uni() < 0.25) publish();
  }
  CHECK(rec.n_ticks == ticks && rec.n_dropped == n_drop && rec.max_len == longest && rec.sum_len == sum);
  CHECK(rec.tick_max_len >= 1 && rec.tick_max_len <= ticks && rec.t_max_len == 0.05 * rec.tick_max_len);
  CHECK(rec.n_too_long + rec.n_dropped <= ticks && rec.max_wind >= 0 && rec.wind_partner >= 0 && rec.wind_partner <= N);
  *dropped += n_drop;
}

}  // namespace

int main() {
  int dropped_roomy = 0, dropped_small = 0;
  for (uint64_t seed = 1; seed <= 6; seed++) { walk(seed, 64, 200, &dropped_roomy); walk(seed, 4, 200, &dropped_small); }
  CHECK(dropped_small > 0);
  // the initial values
  nep_tether_audit two[2];
  std::memset(two, 0x5a, sizeof two);
  CHECK(nep_tether_audit_init(two, 2) == NEP_OK);
  nep_tether_audit zero;
  std::memset(&zero, 0, sizeof zero);
  zero.max_len = -INFINITY;
  CHECK(std::memcmp(&two[0], &zero, sizeof zero) == 0 && std::memcmp(&two[1], &zero, sizeof zero) == 0);
  CHECK(nep_tether_audit_init(nullptr, 1) == NEP_E_ARG && nep_tether_audit_init(two, -1) == NEP_E_ARG && nep_tether_audit_init(two, 0) == NEP_OK);
  // null arguments and a malformed state
  const double pb[4] = {0, 0, 1, 1}, p[2] = {3, 4};
  const nep_ent_cfg cfg{2, 1, 1, 1, 1.0, 10.0, 0, 0, pb, nullptr, nullptr};
  Host st(8, 2);
  const int32_t off[3] = {0, 0, 0}, present[2] = {1, 1};
  const double z[4] = {0, 0, 0, 0};
  const nep_ent_track_inputs in{z, z, present, off, nullptr, off, nullptr};
  double len = 0.0;
  CHECK(nep_ent_tether_length(&cfg, &st.c, p, &len) == NEP_OK && len == 5.0);
  CHECK(nep_ent_tether_length(nullptr, &st.c, p, &len) == NEP_E_ARG && nep_ent_tether_length(&cfg, nullptr, p, &len) == NEP_E_ARG);
  CHECK(nep_ent_tether_length(&cfg, &st.c, nullptr, &len) == NEP_E_ARG && nep_ent_tether_length(&cfg, &st.c, p, nullptr) == NEP_E_ARG);
  st.c.n_alpha = 1; st.c.n_bend = 1; st.alphas[0] = 7; st.alphas[1] = 0; st.bend[0] = 0;      // the bend names nobody (2 agents, no statics)
  CHECK(nep_ent_tether_length(&cfg, &st.c, p, &len) == NEP_E_ARG);
  st.bend[0] = 3;                                                                               // ... or no list entry
  CHECK(nep_ent_tether_length(&cfg, &st.c, p, &len) == NEP_E_ARG);
  st.c.n_alpha = 0; st.c.n_bend = 0;
  nep_tether_audit rec;
  nep_tether_audit_init(&rec, 1);
  CHECK(nep_ent_track_step_audit(&cfg, &in, &st.c, z, p, 1.5, nullptr) == NEP_E_ARG);
  CHECK(nep_ent_track_step_audit(nullptr, &in, &st.c, z, p, 1.5, &rec) == NEP_E_ARG && nep_ent_track_step_audit(&cfg, nullptr, &st.c, z, p, 1.5, &rec) == NEP_E_ARG);
  CHECK(nep_ent_track_step_audit(&cfg, &in, nullptr, z, p, 1.5, &rec) == NEP_E_ARG && nep_ent_track_step_audit(&cfg, &in, &st.c, nullptr, p, 1.5, &rec) == NEP_E_ARG);
  CHECK(rec.n_ticks == 0);
  CHECK(nep_ent_track_step_audit(&cfg, &in, &st.c, z, p, 1.5, &rec) == 0 && rec.n_ticks == 1 && rec.max_len == 5.0 && rec.t_max_len == 1.5 && rec.tick_max_len == 1);
  if (failures) { std::printf("tether_audit_host_check: %d failures\n", failures); return 1; }
  std::printf("tether_audit_host_check ok (%d moves dropped at the capacity of 4, %d at 64)\n", dropped_small, dropped_roomy);
  return 0;
}
