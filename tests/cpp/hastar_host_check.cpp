// hastar_host_check.cpp — the host form of the homotopic grid A* (neptune_amd/csrc/hastar_host.cpp, include/neptune_hastar.h) as a
// stand-alone executable for -fsanitize=address,undefined: the cases in which a capacity binds (signature, contact list, path, the
// pool of shortened lists, the node pool, the budget of pops) and the malformed inputs, with every output buffer allocated at its
// exact size, so that a write past one is an error the sanitizer reports.  Built from hastar_host.cpp alone:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -Iinclude tests/cpp/hastar_host_check.cpp neptune_amd/csrc/hastar_host.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "neptune_hastar.h"

namespace nep {
static std::string g_err;
void set_last_error(const std::string& msg) { g_err = msg; }
}  // namespace nep

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #x, nep::g_err.c_str()); std::exit(1); } } while (0)

namespace {

struct State {
  std::vector<int32_t> n_hsig, n_cont; std::vector<int16_t> id; std::vector<int8_t> sign; std::vector<double> cont;
  nep_hastar_state view;
  State(int n, int hsig_cap, int cont_cap) : n_hsig(n, 0), n_cont(n, 0), id((size_t)n * hsig_cap, 0), sign((size_t)n * hsig_cap, 0), cont((size_t)n * cont_cap * 2, 0.0) {
    view.hsig_cap = hsig_cap; view.cont_cap = cont_cap; view.n_hsig = n_hsig.data(); view.hsig_id = id.data(); view.hsig_sign = sign.data();
    view.n_cont = n_cont.data(); view.cont = cont.data();
  }
};

nep_hastar_cfg make_cfg(double cable, int max_pops, int max_nodes, int hsig_cap, int cont_cap, int path_cap) {
  nep_hastar_cfg c;
  c.resolution = 0.5; c.x_min = 0; c.x_max = 8; c.y_min = 0; c.y_max = 8; c.z_min = 0; c.z_max = 1; c.cable_length = cable; c.bias = 1.1;
  c.max_pops = max_pops; c.max_nodes = max_nodes; c.hsig_cap = hsig_cap; c.cont_cap = cont_cap; c.path_cap = path_cap;
  return c;
}

// one square obstacle at (4, 4) with its inflation by 0.3, and reps whose rays stand across the row y = 2.25
void set_world(nep_hastar_t* h, int n_rep) {
  const int32_t off[2] = {0, 4};
  const double un[8] = {4.25, 4.25, 4.25, 3.75, 3.75, 3.75, 3.75, 4.25};
  const double in[8] = {3.45, 3.45, 4.55, 3.45, 4.55, 4.55, 3.45, 4.55};
  CHECK(nep_hastar_set_uninflated(h, -1, 1, off, un) == 0);
  CHECK(nep_hastar_set_inflated(h, -1, 1, off, in) == 0);
  std::vector<double> rep;
  for (int r = 0; r < n_rep; r++) { const double x = 2.0 + 4.0 * (r + 1) / (n_rep + 1); rep.insert(rep.end(), {x, -0.75, x, -0.25}); }
  CHECK(nep_hastar_set_reps(h, -1, n_rep, n_rep ? rep.data() : nullptr) == 0);
}

struct Run { std::vector<nep_hastar_result> res; std::vector<double> path; State out; };

Run run(const nep_hastar_cfg& c, int n_rep, const std::vector<double>& start, const std::vector<double>& goal, State& in, int expect_rc = 0) {
  const int n = (int)start.size() / 2;
  nep_hastar_t* h = nep_hastar_create(&c, 2);
  CHECK(h);
  set_world(h, n_rep);
  Run r{std::vector<nep_hastar_result>(n), std::vector<double>((size_t)n * c.path_cap * 2, -1.0), State(n, c.hsig_cap, c.cont_cap)};
  std::vector<int32_t> scene(n);
  for (int s = 0; s < n; s++) scene[s] = s % 2;
  CHECK(nep_hastar_search_host(h, n, scene.data(), start.data(), goal.data(), &in.view, r.res.data(), r.path.data(), &r.out.view) == expect_rc);
  CHECK(nep_hastar_search_bytes(h) > 0);
  nep_hastar_destroy(h);
  return r;
}

State base_state(int n, int hsig_cap, int cont_cap, const std::vector<double>& start) {
  State st(n, hsig_cap, cont_cap);
  for (int s = 0; s < n; s++) { st.n_cont[s] = 1; st.cont[(size_t)s * cont_cap * 2] = start[2 * s]; st.cont[(size_t)s * cont_cap * 2 + 1] = start[2 * s + 1]; }
  return st;
}

}  // namespace

int main() {
  const std::vector<double> start = {1.25, 2.25, 1.25, 2.25}, goal = {6.75, 2.25, 6.75, 2.25};
  {      // nothing binds: reached, 12 cells, three crossings
    const nep_hastar_cfg c = make_cfg(100, 100000, 0, 8, 48, 48);
    State in = base_state(2, 8, 48, start);
    Run r = run(c, 3, start, goal, in);
    for (int s = 0; s < 2; s++) { CHECK(r.res[s].status == 1 && r.res[s].flags == 0 && r.res[s].n_path == 12 && r.res[s].g_cells == 11.0 && r.out.n_hsig[s] == 3 && r.out.n_cont[s] == 12); }
    CHECK(std::fabs(r.res[0].length_m - 5.5) < 1e-12);
  }
  {      // signature cap: a list of one entry cannot take the second crossing
    const nep_hastar_cfg c = make_cfg(100, 100000, 0, 1, 48, 48);
    State in = base_state(2, 1, 48, start);
    Run r = run(c, 3, start, goal, in);
    CHECK(r.res[0].flags & NEP_HASTAR_FLAG_HSIG); CHECK(r.out.n_hsig[0] <= 1);
  }
  {      // contact-list cap: the list outgrows five points long before the goal
    const nep_hastar_cfg c = make_cfg(100, 100000, 0, 8, 5, 48);
    State in = base_state(2, 8, 5, start);
    Run r = run(c, 0, start, goal, in);
    CHECK((r.res[0].flags & NEP_HASTAR_FLAG_CONT) && r.res[0].status == -1 && r.out.n_cont[0] == 1);
  }
  {      // path cap: four rows, the rest never written
    const nep_hastar_cfg c = make_cfg(100, 100000, 0, 8, 48, 4);
    State in = base_state(2, 8, 48, start);
    Run r = run(c, 0, start, goal, in);
    CHECK((r.res[1].flags & NEP_HASTAR_FLAG_PATH) && r.res[1].status == 1 && r.res[1].n_path == 4 && r.path[8] == 1.25 && r.path[8 + 6] == 2.75);
  }
  {      // pool of shortened lists: 4 nodes give 32 points, the initial list takes 31, a shortened child needs two
    const nep_hastar_cfg c = make_cfg(3.0, 100000, 4, 8, 32, 48);
    State in(2, 8, 32);
    for (int s = 0; s < 2; s++) {
      in.n_cont[s] = 31;
      for (int k = 0; k < 31; k++) { in.cont[((size_t)s * 32 + k) * 2] = 1.25 + 0.1 * (30 - k); in.cont[((size_t)s * 32 + k) * 2 + 1] = 2.25 + (k % 2 ? 0.15 : 0.0); }
    }
    Run r = run(c, 0, start, goal, in);
    CHECK((r.res[0].flags & NEP_HASTAR_FLAG_POOL) && r.res[0].status == -1 && r.res[0].n_length_checks > 0 && r.out.n_cont[0] == 31);
  }
  {      // a short cable: every child runs updateContPts_orig, the far ones are pruned, the open list empties
    const nep_hastar_cfg c = make_cfg(2.0, 100000, 0, 8, 48, 48);
    State in = base_state(2, 8, 48, start);
    Run r = run(c, 3, start, goal, in);
    CHECK(r.res[0].status == -1 && r.res[0].n_cable_pruned > 0 && r.res[0].flags == 0);
  }
  {      // node pool and budget of pops
    State in = base_state(2, 8, 48, start);
    Run r = run(make_cfg(100, 100000, 12, 8, 48, 48), 3, start, goal, in);
    CHECK(r.res[0].nodes_used == 12 && r.res[0].status == -1);
    Run q = run(make_cfg(100, 5, 0, 8, 48, 48), 3, start, goal, in);
    CHECK(q.res[0].status == 0 && q.res[0].pops == 5);
    Run z = run(make_cfg(100, 0, 1, 8, 48, 48), 3, start, goal, in);
    CHECK(z.res[0].status == 0 && z.res[0].pops == 0 && z.res[0].nodes_used == 1);
  }
  {      // malformed slots, and in place: state_out names state_in's arrays
    const nep_hastar_cfg c = make_cfg(100, 100000, 0, 8, 48, 48);
    State in = base_state(2, 8, 48, start);
    in.n_cont[1] = 49;
    nep_hastar_t* h = nep_hastar_create(&c, 1);
    CHECK(h);
    set_world(h, 3);
    std::vector<nep_hastar_result> res(2); std::vector<double> path(2 * 48 * 2);
    const int32_t scene[2] = {0, 0};
    CHECK(nep_hastar_search_host(h, 2, scene, start.data(), goal.data(), &in.view, res.data(), path.data(), &in.view) == 0);
    CHECK(res[0].status == 1 && in.n_cont[0] == 12 && in.n_hsig[0] == 3 && res[1].flags == NEP_HASTAR_FLAG_STATE && in.n_cont[1] == 0);
    nep_hastar_state wrong = in.view; wrong.cont_cap = 47;
    CHECK(nep_hastar_search_host(h, 2, scene, start.data(), goal.data(), &wrong, res.data(), path.data(), &in.view) == NEP_E_ARG);
    CHECK(nep_hastar_search_host(h, 2, nullptr, start.data(), goal.data(), &in.view, res.data(), path.data(), &in.view) == NEP_E_ARG);
    nep_hastar_destroy(h);
    double out[8];
    const double sq[8] = {4.25, 4.25, 4.25, 3.75, 3.75, 3.75, 3.75, 4.25};
    CHECK(nep_hastar_inflate(4, sq, 0.15, out, 4) == 4 && out[0] == 3.45 && out[1] == 3.45);
    CHECK(nep_hastar_inflate(4, sq, 0.15, out, 3) == NEP_E_CAP);
    const double seg[4] = {0, 0, 5, 5};
    CHECK(nep_hastar_gjk(4, sq, 2, seg) == 1 && nep_hastar_gjk(4, sq, 1, seg) == 0);
  }
  std::printf("hastar_host_check ok\n");
  return 0;
}
