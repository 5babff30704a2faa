// lds_layout_check — the kernels' LDS layouts (neptune_amd/csrc/lds_layout.h) on the CPU: host code, its own main, nothing but the header.
// 1. Over a grid of shapes, for every layout: every array lies inside [0, bytes), its offset is a multiple of its element's size (16
//    where the kernel reads or writes 16 bytes at once), arrays are pairwise disjoint except the pairs the layout declares as aliases,
//    and the derived counts agree with the offsets.  The arrays' extents are restated here, from the kernels' use of them.
// 2. stdin: one shape per line, `kind a b c ...`; the answer line repeats it and adds `: bytes and derived counts`
//    (tests/test_lds_layout_cpu.py compares them with tests/golden/lds_bytes.json, recorded before the header existed).
// The last line is "lds_layout_check ok".
#include "../../neptune_amd/csrc/lds_layout.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace nep;

struct Arr { const char* name; long long off, bytes; int align; const char* host; };      // host: the array whose storage this one borrows (an alias), or null
static long long g_checked = 0;

static void fail(const std::string& what, const char* shape) { std::printf("FAIL %s [%s]\n", what.c_str(), shape); std::exit(1); }

// arrays with storage of their own: inside, aligned, pairwise disjoint; aliases: inside their host's storage (host_end: where that ends)
static void check(const std::vector<Arr>& v, long long total, const char* shape) {
  for (const Arr& a : v) {
    if (a.bytes == 0) continue;
    if (a.off < 0 || a.off + a.bytes > total) fail(std::string(a.name) + " outside the launch's bytes", shape);
    if (a.off % a.align) fail(std::string(a.name) + " misaligned", shape);
    g_checked++;
  }
  for (size_t i = 0; i < v.size(); i++)
    for (size_t j = i + 1; j < v.size(); j++) {
      const Arr &a = v[i], &b = v[j];
      if (a.host || b.host || !a.bytes || !b.bytes) continue;
      if (a.off < b.off + b.bytes && b.off < a.off + a.bytes) fail(std::string(a.name) + " overlaps " + b.name, shape);
    }
}
// an alias [off, off + bytes) lies in the storage [lo, hi) it is declared to borrow
static void inside(const char* name, long long off, long long bytes, long long lo, long long hi, const char* shape) {
  if (off < lo || off + bytes > hi) fail(std::string(name) + " leaves the storage it borrows", shape);
}

static void check_sep(int nh, int N, int S, int ent) {
  char sh[96]; std::snprintf(sh, sizeof sh, "sep %d %d %d %d", nh, N, S, ent);
  const SepLayout L = sep_layout(nh, N, S, ent != 0);
  const int total = nh + N + S + (ent ? N * NEP_MAX_BEND : 0);
  check({{"sA", L.sA, 16LL * L.pool_pairs, 16, nullptr}, {"sBx", L.sBx, 32, 8, nullptr}, {"sBy", L.sBy, 32, 8, nullptr},
         {"sAtt", L.sAtt, 2LL * (total + 8), 2, nullptr}, {"sAct", L.sAct, ent ? 2LL * N : 0, 2, nullptr}}, L.bytes, sh);
  if (L.pool_pairs * 16 != L.sBx - L.sA) fail("pool_pairs is not the pool's extent", sh);
  if (L.pool_pairs < 64 * 8) fail("the pool is below its floor", sh);
  const SepLayout K = sep_carve(L.pool_pairs, sep_total(nh, N, S, ent != 0));      // what the wave works out from the pool_pairs it is passed
  if (K.sA != L.sA || K.sBx != L.sBx || K.sBy != L.sBy || K.sAtt != L.sAtt || K.sAct != L.sAct) fail("the wave's carve differs from the launch's", sh);
  if (L.bytes % 16) fail("bytes not a multiple of 16", sh);
}
static void check_fe(int N, int S, int W, int ns, int D, int ent, int big, int wgs) {
  char sh[128]; std::snprintf(sh, sizeof sh, "frontend %d %d %d %d %d %d big=%d wgs=%d", N, S, W, ns, D, ent, big, wgs);
  const FeLayout L = fe_layout(N, S, W, ns, D, ent != 0, big != 0, wgs);
  const FeSizes z = L.z;
  const long long cap = z.cap, MB = z.mb, NS = N + S, MW = (N + 31) / 32, SW = (S + 31) / 32, V = kFeObsLds * NEP_HULL_MAX_V * 2;
  const int a2 = (cap & 1) ? 8 : 16;      // p_box and o_V are read / written as double2: 16-byte aligned when cap is even (an odd beam width with an odd lattice puts them at 8 mod 16, as before the header: the offsets are pinned)
  std::vector<Arr> v = {
      {"s_f", L.s_f, 8 * cap, 8, nullptr}, {"b_end", L.b_end, 8 * 2 * MB * 6, 8, nullptr}, {"b_g", L.b_g, 8 * 2 * MB, 8, nullptr}, {"b_dist", L.b_dist, 8 * MB, 8, nullptr},
      {"b_f", L.b_f, 8 * MB, 8, nullptr}, {"p_box", L.p_box, 8 * 4 * MB, a2, nullptr}, {"o_aabb", L.o_aabb, 8 * 4 * NS, 8, nullptr}, {"o_V", L.o_V, 8 * V, a2, nullptr},
      {"r_f", L.r_f, 8 * cap, 8, L.rf_alias ? "o_aabb" : nullptr}, {"s_lat", L.s_lat, 8 * 4 * NEP_FE_MAX_SAMPLES, 8, nullptr}, {"s_vox", L.s_vox, 8 * cap, 8, nullptr},
      {"v_key", L.v_key, 8LL * z.vis, 8, nullptr}, {"d_slot", L.d_slot, 4LL * z.dd, 4, nullptr}, {"o_nv", L.o_nv, 4 * NS, 4, nullptr}, {"o_id", L.o_id, 4 * NS, 4, nullptr},
      {"s_i", L.s_i, 4 * 32, 4, nullptr}, {"r_id", L.r_id, 2 * cap, 2, nullptr}, {"s_state", L.s_state, cap, 1, nullptr},
      {"p_parent", L.p_parent, (NEP_MAX_POL + 1) * MB, 1, nullptr}, {"p_comb", L.p_comb, (NEP_MAX_POL + 1) * MB, 1, nullptr}, {"b_valid", L.b_valid, MB, 1, nullptr}};
  if (ent) {
    v.push_back({"m_ent", L.m_ent, 4 * MB * MW, 4, nullptr}); v.push_back({"m_base", L.m_base, 4 * MB * MW, 4, nullptr}); v.push_back({"m_stat", L.m_stat, 4 * MB * SW, 4, nullptr});
    v.push_back({"f_bits", L.f_bits, N, 1, nullptr}); v.push_back({"x_U", L.x_U, 4 * 2 * MW, 4, nullptr});
    if (wgs == 1) v.push_back({"work", L.work, 256LL * (long long)sizeof(nep_fe_ent_state), 8, nullptr});
    else if (L.work != -1) fail("working records in LDS without NEP_FE_ENT_WGS == 1", sh);
    if (L.big_lds_off) v.push_back({"big lists", L.big_lds_off, 256LL * kEntBigLdsBytes, 4, nullptr});
  }
  check(v, L.bytes, sh);
  if (L.bytes % 16) fail("bytes not a multiple of 16", sh);
  // the declared aliases, each inside the storage it borrows
  if (L.rf_alias != (4 * NS + V >= cap)) fail("rf_alias", sh);
  if (L.rf_alias) inside("r_f", L.r_f, 8 * cap, L.o_aabb, L.o_V + 8 * V, sh);
  if (L.ent_lists != L.o_aabb || L.x_hdr != L.s_f || L.x_pool != L.s_vox || L.p_list != L.r_id || L.x_ids != L.o_id || L.x_rec != L.o_aabb) fail("an alias does not start where its host does", sh);
  inside("ent_lists", L.ent_lists, (long long)L.n_lists_a * kEntLdsBytes, L.o_aabb, L.s_lat, sh);      // o_aabb, o_V and, with storage of its own, r_f
  if ((long long)(L.n_lists_a + 1) * kEntLdsBytes <= L.s_lat - L.o_aabb) fail("n_lists_a leaves room for a list unused", sh);
  inside("lists in d_slot", L.d_slot, (long long)L.n_lists_b * kEntLdsBytes, L.d_slot, L.d_slot + 4LL * z.dd, sh);
  inside("lists in s_f", L.s_f, (long long)L.n_lists_c * kEntLdsBytes, L.s_f, L.s_f + 8 * cap, sh);
  inside("lists in s_vox", L.s_vox, (long long)L.n_lists_c * kEntLdsBytes, L.s_vox, L.s_vox + 8 * cap, sh);
  inside("x_hdr", L.x_hdr, 4LL * L.x_words, L.s_f, L.s_f + 8 * cap, sh);
  inside("x_pool", L.x_pool, 4LL * L.x_words, L.s_vox, L.s_vox + 8 * cap, sh);
  inside("x_rec", L.x_rec, L.x_rec_bytes, L.o_aabb, L.o_V + 8 * V, sh);
  inside("x_ids", L.x_ids, 2 * N < 4 * NS ? 2 * N : 4 * NS, L.o_id, L.o_id + 4 * NS, sh);      // (the staged agents: at most N ids of 16 bits)
  if (ent && L.ent_lists % 4) fail("crossing lists misaligned", sh);
  // the big-record lists: behind everything else, only when the launch stays within the CU's LDS
  const FeLayout L0 = fe_layout(N, S, W, ns, D, ent != 0, false, wgs);
  const bool fits = big && ent && L0.bytes + 256 * kEntBigLdsBytes <= 160 * 1024;
  if (fits ? (L.big_lds_off != L0.bytes || L.bytes != L.big_lds_off + 256 * kEntBigLdsBytes) : (L.big_lds_off != 0 || L.bytes != L0.bytes)) fail("the big-record lists' place", sh);
  if (L.bytes > 160 * 1024 && L.big_lds_off) fail("big-record lists in a launch beyond 160 KiB", sh);
}
static void check_ent_check(int N, int S) {
  char sh[64]; std::snprintf(sh, sizeof sh, "ent_check %d %d", N, S);
  const EntCheckLayout L = ent_check_layout(N, S);
  check({{"m_agent", L.m_agent, 4LL * 2 * ((N + 63) / 64), 4, nullptr}, {"m_static", L.m_static, 4LL * 2 * ((S + 63) / 64), 4, nullptr},
         {"work", L.work, (long long)sizeof(nep_fe_ent_state), 8, nullptr}}, L.bytes, sh);
}
static void check_resolve(int N) {
  char sh[64]; std::snprintf(sh, sizeof sh, "resolve %d", N);
  const ResolveLayout L = resolve_layout(N);
  check({{"sAcc", L.sAcc, 4LL * N, 4, nullptr}, {"sBad", L.sBad, 4LL * N, 4, nullptr}, {"sRow", L.sRow, 4LL * N * L.W, 4, nullptr}, {"sBits", L.sBits, 4LL * L.W, 4, nullptr}}, L.bytes, sh);
  if (L.W != (N + 31) / 32) fail("W", sh);
}
static void check_audit(int N, int S, int vs) {
  char sh[64]; std::snprintf(sh, sizeof sh, "audit %d %d %d", N, S, vs);
  const AuditLayout L = audit_layout(N, S, vs);
  check({{"pxy", L.pxy, 16LL * S * vs, 8, nullptr}, {"pinv", L.pinv, 8LL * S * vs, 8, nullptr}, {"ag", L.ag, 32LL * N, 8, nullptr}, {"pnv", L.pnv, 4LL * S, 4, nullptr},
         {"apres", L.apres, 4LL * N, 4, nullptr}}, L.bytes, sh);
}
static void check_mission(int N, int nv, int np) {
  char sh[64]; std::snprintf(sh, sizeof sh, "mission %d %d %d", N, nv, np);
  const MissionLayout L = mission_layout(N, nv, np);
  check({{"s_end", L.s_end, 24LL * N, 8, nullptr}, {"s_new", L.s_new, 24LL * N, 8, nullptr}, {"s_kxy", L.s_kxy, 16LL * nv, 8, nullptr}, {"s_got", L.s_got, 4LL * N, 4, nullptr},
         {"s_off", L.s_off, 4LL * (np + 1), 4, nullptr}}, L.bytes, sh);
  // a scene's own counts never carve beyond the launch, which is sized with the maxima
  if (nv <= NEP_MISSION_MAX_VERT && np <= NEP_MISSION_MAX_POLY && L.bytes > mission_layout(N, NEP_MISSION_MAX_VERT, NEP_MISSION_MAX_POLY).bytes) fail("a scene's carve exceeds the launch", sh);
}

static void grid() {
  const int Ns[] = {1, 2, 5, 7, 8, 9, 10, 31, 32, 33, 63, 64, 65, 89, 90, 124, 125, 127, 128, 129, 192, 193, 253, 254, 256, 257, 320, 321, 492, 493, 681, 682, 1000};
  const int Ss[] = {0, 1, 2, 3, 20, 32, 33, 63, 64, 65, 100, 129};
  for (int N : Ns)
    for (int S : Ss) {
      for (int ent = 0; ent < 2; ent++) {
        check_sep(N, N, S, ent); check_sep(2 * N, N, S, ent);
      }
      check_ent_check(N, S);
      for (int vs : {1, 3, 4, 16}) check_audit(N, S, vs);
    }
  for (int N : Ns) { check_resolve(N); for (int nv : {0, 1, 7, NEP_MISSION_MAX_VERT}) for (int np : {0, 1, NEP_MISSION_MAX_POLY}) check_mission(N, nv, np); }
  const int fN[] = {1, 4, 5, 6, 7, 8, 9, 12, 13, 31, 32, 33, 64, 65, 187, 188, 256, 400, 1500};
  const int fS[] = {0, 1, 2, 20, 32, 33, 64, 65, 100};
  for (int W : {1, 2, 8, 31, 32, 33, 48, 64})
    for (int ns : {1, 2, 3, 4, 5})
      for (int N : fN)
        for (int S : fS)
          for (int ent = 0; ent < 2; ent++)
            for (int big = 0; big <= ent; big++)
              for (int wgs : {1, 3}) { check_fe(N, S, W, ns, 8, ent, big, wgs); if (N == 8) check_fe(N, S, W, ns, 3, ent, big, wgs); }
}

int main() {
  static_assert(kEntLdsBytes % 4 == 0 && (kEntLdsBytes / 4) % 2 == 1 && kEntBigLdsBytes % 4 == 0 && (kEntBigLdsBytes / 4) % 2 == 1, "a list is an odd number of dwords");
  static_assert(kEntLdsBytes >= NEP_FE_ENT_CAP * 3 + NEP_MAX_BEND && kEntBigLdsBytes >= kEntBigLdsCap * 3 + kEntBigLdsBend, "a list holds ids, cases and bend indices");
  grid();
  char line[512];
  while (std::fgets(line, sizeof line, stdin)) {
    char kind[32]; int a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int n = std::sscanf(line, "%31s %d %d %d %d %d %d %d %d", kind, a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7) - 1;
    if (n < 0) continue;
    std::string echo = kind; for (int i = 0; i < n; i++) echo += " " + std::to_string(a[i]);
    if (!std::strcmp(kind, "sep") && n == 4) { check_sep(a[0], a[1], a[2], a[3]); const SepLayout L = sep_layout(a[0], a[1], a[2], a[3] != 0); std::printf("%s : %d %d\n", echo.c_str(), L.bytes, L.pool_pairs); }
    else if (!std::strcmp(kind, "frontend") && n == 7) {      // N S W ns num_pol ent ent_ns -> bytes, children cap, xpool words, the big-record launch's big_lds_off and bytes
      check_fe(a[0], a[1], a[2], a[3], a[4], a[5], 0, NEP_FE_ENT_WGS); check_fe(a[0], a[1], a[2], a[3], a[4], a[5], a[5], NEP_FE_ENT_WGS);
      const FeLayout L = fe_layout(a[0], a[1], a[2], a[3], a[4], a[5] != 0), B = fe_layout(a[0], a[1], a[2], a[3], a[4], a[5] != 0, true);
      std::printf("%s : %d %d %lld %d %d\n", echo.c_str(), L.bytes, L.z.cap, a[5] ? fe_xpool_words(L, a[6]) : 0LL, a[5] ? B.big_lds_off : 0, a[5] ? B.bytes : 0);
    } else if (!std::strcmp(kind, "ent_check") && n == 2) { check_ent_check(a[0], a[1]); std::printf("%s : %d\n", echo.c_str(), ent_check_layout(a[0], a[1]).bytes); }
    else if (!std::strcmp(kind, "resolve") && n == 1) { check_resolve(a[0]); std::printf("%s : %d\n", echo.c_str(), resolve_layout(a[0]).bytes); }
    else if (!std::strcmp(kind, "audit") && n == 3) { check_audit(a[0], a[1], a[2]); std::printf("%s : %lld\n", echo.c_str(), audit_layout(a[0], a[1], a[2]).bytes); }
    else if (!std::strcmp(kind, "mission") && n == 3) { check_mission(a[0], a[1], a[2]); std::printf("%s : %d\n", echo.c_str(), mission_layout(a[0], a[1], a[2]).bytes); }
    else { std::printf("FAIL unknown row: %s", line); return 1; }
  }
  std::printf("%lld arrays checked\nlds_layout_check ok\n", g_checked);
  return 0;
}
