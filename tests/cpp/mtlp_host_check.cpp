// mtlp_host_check.cpp — the host form of the MTLP comparator (neptune_amd/csrc/mtlp_host.cpp, include/neptune_mtlp.h) as a
// stand-alone executable for -fsanitize=address,undefined: the cases in which a capacity binds (the node pool, the budget of pops,
// the path), one robot alone and NEP_MTLP_MAX_ROBOTS robots (a full list of 63 cable lines), the malformed inputs, and the exact arithmetic at the edges of the stated domain (coordinates of magnitude 1e5 and
// 2^20 that differ by 2^-60 in effect, the smallest multiples of 2^-60), with every output buffer allocated at its exact size, so
// that a write past one is an error the sanitizer reports.  Built from mtlp_host.cpp alone:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -Iinclude tests/cpp/mtlp_host_check.cpp neptune_amd/csrc/mtlp_host.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "neptune_mtlp.h"

namespace nep {
static std::string g_err;
void set_last_error(const std::string& msg) { g_err = msg; }
}  // namespace nep

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #x, nep::g_err.c_str()); std::exit(1); } } while (0)

namespace {

nep_mtlp_cfg make_cfg(int n, int max_nodes, int max_pops, int path_cap, double radius) {
  nep_mtlp_cfg c;
  c.resolution = 0.25; c.x_min = 0; c.x_max = 4; c.y_min = 0; c.y_max = 4; c.z_min = 0; c.z_max = 1; c.radius = radius; c.bias = 1.1;
  c.n_robots = n; c.max_nodes = max_nodes; c.max_pops = max_pops; c.path_cap = path_cap;
  return c;
}

struct Out {
  std::vector<int32_t> graph, status; std::vector<nep_mtlp_result> res; std::vector<double> path;
  Out(int r, int n, int path_cap) : graph((size_t)r * n * n, -7), status(r, -7), res((size_t)r * n), path((size_t)r * n * path_cap * 3, -7.0) {}
};

int g_exact = 0;      // sign evaluations that went to the integer path
int verdict(int which, const std::vector<double>& rec) {
  std::vector<double> in(16, 0.0);
  for (size_t k = 0; k < rec.size(); k++) in[k] = rec[k];
  int32_t v = -1, e = -1;
  CHECK(nep_mtlp_predicates_host(which, 1, in.data(), &v, &e) == 0);
  g_exact += e;
  return v;
}

}  // namespace

int main() {
  // ---- capacities: two robots, one reaches, one cannot (its goal lies below its cell's centre) and fills a pool of 40 / spends 9 pops
  const double bases[6] = {0.5, 0.5, 0.0, 3.5, 0.5, 0.0};
  const double sg[12] = {1.0, 1.0, 0.5, 3.0, 3.0, 0.7, 3.0, 1.0, 0.5, 1.0, 3.0, 0.5};
  for (int variant = 0; variant < 3; variant++) {
    const nep_mtlp_cfg c = variant == 0 ? make_cfg(2, 40, 1000, 3, 0.25) : variant == 1 ? make_cfg(2, 512, 9, 32, 0.25) : make_cfg(2, 1, 5, 1, 0.0);
    nep_mtlp_t* h = nep_mtlp_create(&c);
    CHECK(h);
    CHECK(nep_mtlp_search_bytes(h) > 0);
    Out o(1, 2, c.path_cap);
    CHECK(nep_mtlp_solve_host(h, 1, bases, sg, o.graph.data(), o.status.data(), o.res.data(), o.path.data()) == 0);
    CHECK(o.status[0] == 1 && o.graph[0] == 1 && o.graph[3] == 1);
    for (int i = 0; i < 2; i++) {
      CHECK(o.res[i].nodes_used <= c.max_nodes && o.res[i].pops <= c.max_pops && o.res[i].n_path <= c.path_cap);
      for (int k = 3 * o.res[i].n_path; k < 3 * c.path_cap; k++) CHECK(o.path[(size_t)i * c.path_cap * 3 + k] == 0.0);
    }
    if (variant == 0) CHECK(o.res[1].status == -1 && o.res[1].nodes_used == 40);      // the pool filled, then the list emptied
    if (variant == 1) CHECK(o.res[1].status == 0 && o.res[1].pops == 9);
    if (variant == 2) CHECK(o.res[0].status == -1 && o.res[0].nodes_used == 1 && o.res[0].pops == 1);
    nep_mtlp_destroy(h);
  }
  {      // a path longer than path_cap
    const nep_mtlp_cfg c = make_cfg(2, 512, 300, 4, 0.25);
    nep_mtlp_t* h = nep_mtlp_create(&c);
    CHECK(h);
    Out o(1, 2, 4);
    CHECK(nep_mtlp_solve_host(h, 1, bases, sg, o.graph.data(), o.status.data(), o.res.data(), o.path.data()) == 0);
    CHECK(o.res[0].status == 1 && o.res[0].n_path == 4 && (o.res[0].flags & NEP_MTLP_FLAG_PATH));
    nep_mtlp_destroy(h);
  }
  {      // one robot: no cable line, an empty dense block; the goal lies below its cell's centre, so 2 pops spend the budget
    const nep_mtlp_cfg c = make_cfg(1, 64, 2, 8, 0.25);
    nep_mtlp_t* h = nep_mtlp_create(&c);
    CHECK(h);
    const double b1[3] = {0.5, 0.5, 0.0}, s1[6] = {1.0, 1.0, 0.5, 3.0, 3.0, 0.55};
    Out o(1, 1, 8);
    CHECK(nep_mtlp_solve_host(h, 1, b1, s1, o.graph.data(), o.status.data(), o.res.data(), o.path.data()) == 0);
    CHECK(o.status[0] == 1 && o.graph[0] == 1);
    CHECK(o.res[0].status == 0 && o.res[0].pops == 2 && o.res[0].nodes_used > 1 && o.res[0].nodes_used <= 64 && o.res[0].n_path == 0 && o.res[0].n_ball_only == 0);
    for (int k = 0; k < 8 * 3; k++) CHECK(o.path[k] == 0.0);
    nep_mtlp_destroy(h);
  }
  // ---- NEP_MTLP_MAX_ROBOTS robots on a 1/16 lattice, 2 pops each: 4 096 graph entries, and robot 0's list of cable lines is full —
  // every later robot gives it one, 63 in all.  With a radius of 8 every one of them lies wholly inside the ball of every
  // neighbour of robot 0's start: its n_ball_only counts 63 lines times 26 neighbours, and its list empties at the first pop
  for (int variant = 0; variant < 2; variant++) {
    const int n = NEP_MTLP_MAX_ROBOTS;
    CHECK(n == 64);
    const nep_mtlp_cfg c = make_cfg(n, 256, 2, 4, variant == 0 ? 0.25 : 8.0);
    nep_mtlp_t* h = nep_mtlp_create(&c);
    CHECK(h);
    CHECK(nep_mtlp_search_bytes(h) >= (int64_t)((n - 1) * 6 * sizeof(double)));
    std::vector<double> b((size_t)n * 3), s((size_t)n * 6);
    uint32_t lcg = 12345u;
    auto lat = [&lcg](int lo, int hi) { lcg = lcg * 1664525u + 1013904223u; return (double)(lo + (int)((lcg >> 8) % (uint32_t)(hi - lo + 1))) / 16.0; };
    for (int i = 0; i < n; i++) {
      b[3 * i] = lat(4, 60); b[3 * i + 1] = lat(4, 60); b[3 * i + 2] = 0.0;
      s[6 * i] = lat(4, 60); s[6 * i + 1] = lat(4, 60); s[6 * i + 2] = lat(1, 15);
      s[6 * i + 3] = lat(4, 60); s[6 * i + 4] = lat(4, 60); s[6 * i + 5] = 0.6875;
    }
    s[0] = 2.0; s[1] = 2.0; s[2] = 0.3125; s[5] = 0.9375;      // robot 0: cell (8, 8, 1), and no neighbour above the goal height
    Out o(1, n, c.path_cap);
    CHECK(nep_mtlp_solve_host(h, 1, b.data(), s.data(), o.graph.data(), o.status.data(), o.res.data(), o.path.data()) == 0);
    CHECK(o.status[0] == 1);
    for (int i = 0; i < n; i++) {
      CHECK(o.graph[(size_t)i * n + i] == 1);
      for (int j = 0; j < n; j++) CHECK(o.graph[(size_t)i * n + j] == 0 || o.graph[(size_t)i * n + j] == 1);
      const nep_mtlp_result& r = o.res[i];
      CHECK(r.status >= -1 && r.status <= 1 && r.pops >= 1 && r.pops <= 2 && r.nodes_used >= 1 && r.nodes_used <= 256 && r.n_path <= c.path_cap && !(r.flags & NEP_MTLP_FLAG_STATE));
      for (int k = 3 * r.n_path; k < 3 * c.path_cap; k++) CHECK(o.path[(size_t)i * c.path_cap * 3 + k] == 0.0);
    }
    if (variant == 1) CHECK(o.res[0].n_ball_only == 63 * 26 && o.res[0].status == -1 && o.res[0].pops == 1 && o.res[0].nodes_used == 1);
    nep_mtlp_destroy(h);
  }
  // ---- malformed: configurations create refuses, runs outside the domain
  {
    nep_mtlp_cfg c = make_cfg(2, 64, 10, 8, 0.25);
    c.max_pops = 0; CHECK(!nep_mtlp_create(&c)); c.max_pops = 10;
    c.n_robots = 0; CHECK(!nep_mtlp_create(&c)); c.n_robots = NEP_MTLP_MAX_ROBOTS + 1; CHECK(!nep_mtlp_create(&c)); c.n_robots = 2;
    c.resolution = 0.001; CHECK(!nep_mtlp_create(&c)); c.resolution = std::nan(""); CHECK(!nep_mtlp_create(&c)); c.resolution = 0.25;
    c.x_max = 2e5; CHECK(!nep_mtlp_create(&c)); c.x_max = 4;
    c.radius = std::ldexp(1.0, -70); CHECK(!nep_mtlp_create(&c)); c.radius = -0.25; CHECK(!nep_mtlp_create(&c)); c.radius = 0.25;
    c.z_max = 0.0; CHECK(!nep_mtlp_create(&c)); c.z_max = 1;
    c.resolution = 1.0; c.max_nodes = 1 << 24; CHECK(!nep_mtlp_create(&c));      // 2^24 cells of 1 m beyond the grid: past 2^20
    CHECK(!nep_mtlp_create(nullptr));
    c = make_cfg(2, 64, 10, 8, 0.25);
    nep_mtlp_t* h = nep_mtlp_create(&c);
    CHECK(h);
    std::vector<double> b(4 * 6), s(4 * 12);
    for (int r = 0; r < 4; r++) { for (int k = 0; k < 6; k++) b[6 * r + k] = bases[k]; for (int k = 0; k < 12; k++) s[12 * r + k] = sg[k]; }
    b[6 * 1 + 2] = std::nan(""); s[12 * 2 + 7] = 100000.5; s[12 * 3 + 0] = std::ldexp(1.0, -61);
    Out o(4, 2, 8);
    CHECK(nep_mtlp_solve_host(h, 4, b.data(), s.data(), o.graph.data(), o.status.data(), o.res.data(), o.path.data()) == 0);
    CHECK(o.status[0] == 1 && !(o.res[0].flags & NEP_MTLP_FLAG_STATE) && o.res[0].pops > 0);
    for (int r = 1; r < 4; r++) {
      CHECK(o.status[r] == NEP_E_STATE);
      for (int k = 0; k < 4; k++) CHECK(o.graph[4 * r + k] == 0);
      for (int i = 0; i < 2; i++) CHECK(o.res[2 * r + i].status == -1 && o.res[2 * r + i].flags == NEP_MTLP_FLAG_STATE && o.res[2 * r + i].pops == 0);
      for (int k = 0; k < 2 * 8 * 3; k++) CHECK(o.path[(size_t)r * 2 * 8 * 3 + k] == 0.0);
    }
    CHECK(nep_mtlp_solve_host(h, -1, b.data(), s.data(), o.graph.data(), o.status.data(), o.res.data(), o.path.data()) == NEP_E_ARG);
    CHECK(nep_mtlp_solve_host(h, 1, nullptr, s.data(), o.graph.data(), o.status.data(), o.res.data(), o.path.data()) == NEP_E_ARG);
    CHECK(nep_mtlp_solve_host(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    nep_mtlp_destroy(h);
    double cb[15];
    CHECK(nep_mtlp_circle_bases(5, cb) == 0 && cb[2] == 0.0 && std::fabs(cb[0] + 10.0) < 1e-2);
    CHECK(nep_mtlp_circle_bases(0, cb) == NEP_E_ARG);
  }
  // ---- the exact arithmetic at the edges of the domain
  {
    const double e = std::ldexp(1.0, -60), big = 100000.0, top = 1048576.0;
    // segment/segment: q exactly on u v, and one step of 2^-60 (near zero) or one ulp (at 1e5) to either side of it
    CHECK(verdict(1, {-1, 0, 0, 0, 0, 0, 0, -1, 0, 0, 1, 0}) == 1);
    CHECK(verdict(1, {-1, 0, 0, -e, 0, 0, 0, -1, 0, 0, 1, 0}) == 0);
    CHECK(verdict(1, {-1, 0, 0, e, 0, 0, 0, -1, 0, 0, 1, 0}) == 1);
    const double below = std::nextafter(big, 0.0);
    CHECK(verdict(1, {-big, -big, 0, big, big, 0, -big, big, 0, big, -big, 0}) == 1);      // the diagonals of the whole domain
    CHECK(verdict(1, {-big, -big, 0, 0, 0, 0, e, e, 0, big, big, 0}) == 0);      // collinear, 2^-60 apart
    CHECK(verdict(1, {-big, -big, 0, below, big, 0, big, below, 0, big, big, 0}) == 0);
    // segment/triangle with vertices at +-2^20 (cell centres may lie that far): through a vertex, an edge, and 2^-60 beside them
    CHECK(verdict(0, {top, top, -1, top, top, 1, top, top, 0, -top, top, 0, top, -top, 0}) == 1);
    CHECK(verdict(0, {0, 0, -top, 0, 0, top, top, top, 0, -top, top, 0, top, -top, 0}) == 1);      // through the edge's middle
    CHECK(verdict(0, {-e, -e, -top, -e, -e, top, top, top, 0, -top, top, 0, top, -top, 0}) == 0);
    CHECK(verdict(0, {e, e, -top, e, e, top, top, top, 0, -top, top, 0, top, -top, 0}) == 1);
    CHECK(verdict(0, {0, 0, e, 1, 1, e, top, top, 0, -top, top, 0, top, -top, 0}) == 0);      // parallel, 2^-60 above
    CHECK(verdict(0, {0, 0, 0, 1, 1, 0, top, top, 0, -top, top, 0, top, -top, 0}) == 1);      // coplanar
    CHECK(verdict(0, {5, 5, 0, 7, 7, 0, 1, 1, 0, 2, 2, 0, 3, 3, 0}) == 0 && verdict(0, {3, 3, 0, 7, 7, 0, 1, 1, 0, 2, 2, 0, 3, 3, 0}) == 1);      // a collinear triangle
    CHECK(verdict(0, {2, 2, 0, 2, 2, 0, 2, 2, 0, 2, 2, 0, 2, 2, 0}) == 1);      // five times one point
    // ball/segment: radius 1e5 (squared 1e10) about a corner of the domain, a tangent line, and its neighbours at 2^-60 / one ulp
    CHECK(verdict(2, {0, 0, 0, -1, 0.25, 0, 1, 0.25, 0, 0.0625}) == 1);
    CHECK(verdict(2, {0, 0, 0, -1, 0.25 + std::ldexp(1.0, -54), 0, 1, 0.25 + std::ldexp(1.0, -54), 0, 0.0625}) == 0);
    CHECK(verdict(2, {e, 0, 0, 0, 0, 0, 0, 1, 0, 0}) == 0 && verdict(2, {e, 0, 0, 0, 0, 0, e, 0, 0, 0}) == 1);      // radius 0
    CHECK(verdict(2, {-big, -big, -big, -big, 0, -big - 1, -big, 0, -big + 1, big * big}) == 1);
    CHECK(verdict(2, {-big, -big, -big, -big, std::nextafter(0.0 + 1.0, 2.0) - 1.0, -top, -big, std::nextafter(1.0, 2.0) - 1.0, top, big * big}) == 0);
    CHECK(verdict(2, {0, 0, 0, 0.125, 0, 0, 0, 0.125, 0, 0.0625}) == 3);      // wholly inside
    CHECK(verdict(2, {0, 0, 0, 0.25, 0, 0, 0, 0.125, 0, 0.0625}) == 1);      // an end on the sphere
  }
  std::printf("exact sign evaluations: %d\n", g_exact);
  CHECK(g_exact >= 10);
  std::printf("mtlp_host_check ok\n");
  return 0;
}
