// mtlp_host.cpp — the handle and the host form of the MTLP comparator (include/neptune_mtlp.h).  No HIP call; built like
// hastar_host.cpp (-O2 -ffp-contract=off).  The rule set is mtlp_common.h's, run one item at a time; the device form
// (mtlp_kernels.hip) compiles the same functions and equals this byte for byte.  This file stands alone:
// tests/cpp/mtlp_host_check.cpp is built from it and nothing else (it supplies nep::set_last_error itself).
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "mtlp_common.h"

namespace nep { void set_last_error(const std::string& msg); }

using namespace nep_mtlp_impl;

namespace {
int fail(int rc, const char* msg) { nep::set_last_error(msg); return rc; }
}  // namespace

extern "C" {

nep_mtlp_t* nep_mtlp_create(const nep_mtlp_cfg* cfg) {
  if (!cfg) { nep::set_last_error("bad arguments"); return nullptr; }
  const nep_mtlp_cfg& c = *cfg;
  for (double v : {c.resolution, c.x_min, c.x_max, c.y_min, c.y_max, c.z_min, c.z_max, c.radius})
    if (!in_domain(v)) { nep::set_last_error("resolution, bounds and radius must be finite multiples of 2^-60 of magnitude <= NEP_MTLP_MAX_COORD"); return nullptr; }
  if (!(c.resolution >= 0.0078125) || !(c.radius >= 0.0) || !std::isfinite(c.bias) || !(c.bias > 0.0)) {
    nep::set_last_error("resolution >= 2^-7, radius >= 0, bias finite and positive"); return nullptr;
  }
  if (c.n_robots < 1 || c.n_robots > NEP_MTLP_MAX_ROBOTS || c.path_cap < 1 || c.path_cap > (1 << 24) || c.max_nodes < 0) {
    nep::set_last_error("n_robots in 1 .. NEP_MTLP_MAX_ROBOTS, path_cap >= 1, max_nodes >= 0"); return nullptr;
  }
  if (c.max_pops <= 0) { nep::set_last_error("max_pops must be positive: there is no unbounded search"); return nullptr; }
  Par p;
  p.res = c.resolution; p.inv_res = 1.0 / c.resolution; p.xl = c.x_min; p.yl = c.y_min; p.zl = c.z_min; p.r2 = c.radius * c.radius; p.bias = c.bias;
  // mtlp::mtlp (solveMultiLinearPath.hpp:28-36)
  const double gx = (c.x_max - c.x_min) * p.inv_res, gy = (c.y_max - c.y_min) * p.inv_res, gz = (c.z_max - c.z_min) * p.inv_res;
  if (!(gx >= 1.0) || !(gy >= 1.0) || !(gz >= 1.0) || !(gx < 32768.0) || !(gy < 32768.0) || !(gz < 32768.0)) {
    nep::set_last_error("the grid needs 1 to 32767 cells along every axis"); return nullptr;
  }
  p.glx = (int)gx; p.gly = (int)gy; p.glz = (int)gz;
  const long long glxyz = (long long)p.glx * p.gly * p.glz, nodes = c.max_nodes > 0 ? c.max_nodes : glxyz;
  if (nodes < 1 || nodes > (1LL << 24)) { nep::set_last_error("the node pool (max_nodes, or GLX * GLY * GLZ) must hold 1 to 2^24 nodes"); return nullptr; }
  p.n = c.n_robots; p.max_nodes = (int)nodes; p.max_pops = c.max_pops; p.path_cap = c.path_cap;
  p.hash_size = 16; while (p.hash_size < 2 * p.max_nodes) p.hash_size *= 2;
  // no bounds test: a search can walk one cell per node beyond the grid.  Every centre it can reach must stay within 2^20
  const double lo[3] = {c.x_min, c.y_min, c.z_min}, hi[3] = {c.x_max, c.y_max, c.z_max};
  const int gl[3] = {p.glx, p.gly, p.glz};
  for (int k = 0; k < 3; k++) {
    const double a = std::fabs(lo[k]) > std::fabs(hi[k]) ? std::fabs(lo[k]) : std::fabs(hi[k]);
    if (!(((double)gl[k] + (double)nodes + 2.0) * c.resolution + a <= 1048576.0)) {
      nep::set_last_error("max_nodes * resolution would carry a search beyond 2^20, where the exact predicates end: lower max_nodes"); return nullptr;
    }
  }
  nep_mtlp_t* h = new (std::nothrow) nep_mtlp();
  if (!h) { nep::set_last_error("out of memory"); return nullptr; }
  h->cfg = c; h->par = p;
  return h;
}

void nep_mtlp_destroy(nep_mtlp_t* h) {
  if (!h) return;
  if (h->dev && h->dev_free) h->dev_free(h->dev);
  delete h;
}

int64_t nep_mtlp_search_bytes(const nep_mtlp_t* h) { return h ? (int64_t)work_bytes(h->par) : (int64_t)NEP_E_ARG; }

int nep_mtlp_solve_host(nep_mtlp_t* h, int32_t n_runs, const double* bases, const double* start_goal, int32_t* graph, int32_t* run_status,
                        nep_mtlp_result* result, double* path) {
  if (!h || n_runs < 0) return fail(NEP_E_ARG, "bad arguments");
  if (n_runs == 0) return 0;
  if (!bases || !start_goal || !graph || !run_status || !result || !path) return fail(NEP_E_ARG, "null argument");
  const Par& p = h->par;
  const int n = p.n;
  h->host_work.resize(work_bytes(p) + 16);
  char* mem = h->host_work.data();
  mem += (16 - ((uintptr_t)mem & 15)) & 15;
  SerialEx ex;
  for (int r = 0; r < n_runs; r++) {
    const double* b = bases + (size_t)r * n * 3; const double* sg = start_goal + (size_t)r * n * 6;
    int32_t* g = graph + (size_t)r * n * n;
    const bool ok = run_in_domain(b, sg, n);
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) g[i * n + j] = ok ? graph_entry(b, sg, i, j) : 0;
    run_status[r] = ok ? 1 : NEP_E_STATE;
    for (int i = 0; i < n; i++) {
      const size_t s = (size_t)r * n + i;
      search(ex, p, b, sg, g, i, ok, mem, result + s, path + s * p.path_cap * 3);
      h->host_flags |= result[s].flags;
    }
  }
  return 0;
}

int nep_mtlp_circle_bases(int32_t n, double* out) {
  if (n < 1 || !out) return fail(NEP_E_ARG, "bad arguments");
  // mtlp_node.cpp:295-313: doubles narrowed to float by cosf / sinf, widened again by the product
  const double circle_init_dist_to_agent = 2.5, circle_init_radius = 10;
  const double one_slice = 3.1415927 * 2 / n;
  for (int i = 0; i < n; i++) {
    const double theta = one_slice * i;
    out[3 * i] = -circle_init_radius * cosf((float)theta) - circle_init_dist_to_agent * cosf((float)(1.571 - theta));
    out[3 * i + 1] = -circle_init_radius * sinf((float)theta) + circle_init_dist_to_agent * sinf((float)(1.571 - theta));
    out[3 * i + 2] = 0.0;
  }
  return 0;
}

int nep_mtlp_predicates_host(int32_t which, int32_t n, const double* in, int32_t* verdict, int32_t* exact) {
  if (which < 0 || which > 2 || n < 0 || (n > 0 && (!in || !verdict || !exact))) return fail(NEP_E_ARG, "bad arguments");
  for (int k = 0; k < n; k++) {
    const double* q = in + 16 * (size_t)k;
    int nex = 0;
    if (which == 0) verdict[k] = seg_tri(q, q + 3, q + 6, q + 9, q + 12, nex);
    else if (which == 1) verdict[k] = seg_seg2(q, q + 3, q + 6, q + 9, 0, 1, nex);
    else verdict[k] = ball_seg(q, q[9], q + 3, q + 6, nex);
    exact[k] = nex;
  }
  return 0;
}

}  // extern "C"
