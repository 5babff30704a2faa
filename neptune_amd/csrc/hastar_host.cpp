// hastar_host.cpp — the handle, the setters and the host form of the homotopic grid A* (include/neptune_hastar.h).  No HIP call;
// built like plan_host.cpp (-O2 -ffp-contract=off).  The search is hastar_common.h's, run one item at a time; the device form
// (hastar_kernels.hip) compiles the same function and equals this byte for byte.  This file stands alone: tests/cpp/hastar_host_check.cpp
// is built from it and nothing else (it supplies nep::set_last_error itself).
#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "hastar_common.h"

namespace nep { void set_last_error(const std::string& msg); }

using namespace nep_hastar_impl;

namespace {
int fail(int rc, const char* msg) { nep::set_last_error(msg); return rc; }
bool pos_finite(double v) { return std::isfinite(v) && v > 0.0; }

int set_polys(nep_hastar_t* h, int32_t scene, int32_t n_poly, const int32_t* off, const double* xy, bool inflated) {
  if (!h || scene < -1 || scene >= h->n_scenes || n_poly < 0 || (n_poly > 0 && (!off || !xy))) return fail(NEP_E_ARG, "bad arguments");
  if (n_poly > 0 && off[0] != 0) return fail(NEP_E_ARG, "polygon offsets must start at 0");
  for (int k = 0; k < n_poly; k++) if (off[k + 1] - off[k] < 1) return fail(NEP_E_ARG, "every polygon needs at least one vertex");
  if (n_poly > 0 && 8LL * n_poly > 0x7fffffffLL) return fail(NEP_E_CAP, "too many polygons");
  const int nv = n_poly > 0 ? off[n_poly] : 0;
  for (int i = 0; i < 2 * nv; i++) if (!std::isfinite(xy[i])) return fail(NEP_E_ARG, "a vertex is not finite");
  for (int s = scene < 0 ? 0 : scene; s < (scene < 0 ? h->n_scenes : scene + 1); s++) {
    SceneHost& S = h->scenes[s];
    std::vector<int32_t>& o = inflated ? S.infl_off : S.un_off;
    std::vector<double>& v = inflated ? S.infl_xy : S.un_xy;
    if (n_poly > 0) o.assign(off, off + n_poly + 1); else o.assign(1, 0);
    v.assign(xy, xy + 2 * (size_t)nv);
  }
  h->dirty = true;
  return 0;
}
}  // namespace

extern "C" {

nep_hastar_t* nep_hastar_create(const nep_hastar_cfg* cfg, int32_t n_scenes) {
  if (!cfg || n_scenes < 1) { nep::set_last_error("bad arguments"); return nullptr; }
  const nep_hastar_cfg& c = *cfg;
  if (!pos_finite(c.resolution) || !pos_finite(c.bias) || !pos_finite(c.cable_length) || !std::isfinite(c.x_min) || !std::isfinite(c.x_max) ||
      !std::isfinite(c.y_min) || !std::isfinite(c.y_max) || !std::isfinite(c.z_min) || !std::isfinite(c.z_max)) {
    nep::set_last_error("resolution, bias and cable_length must be finite and positive, the bounds finite"); return nullptr;
  }
  if (c.max_pops < 0 || c.max_nodes < 0 || c.hsig_cap < 1 || c.cont_cap < 2 || c.path_cap < 1 || c.hsig_cap > 32767 || c.cont_cap > (1 << 20) || c.path_cap > (1 << 24)) {
    nep::set_last_error("max_pops and max_nodes >= 0, hsig_cap and path_cap >= 1, cont_cap >= 2"); return nullptr;
  }
  Par p;
  p.res = c.resolution; p.inv_res = 1.0 / c.resolution; p.xl = c.x_min; p.yl = c.y_min; p.cable = c.cable_length; p.bias = c.bias;
  // AstarPathFinder::init (:32-40)
  const double gx = (c.x_max - c.x_min) * p.inv_res, gy = (c.y_max - c.y_min) * p.inv_res, gz = (c.z_max - c.z_min) * p.inv_res;
  if (!(gx >= 1.0) || !(gy >= 1.0) || !(gx < 32768.0) || !(gy < 32768.0) || !(gz < 32768.0)) { nep::set_last_error("the grid needs 1 to 32767 cells along x and y"); return nullptr; }
  p.glx = (int)gx; p.gly = (int)gy;
  const long long glz = gz >= 1.0 ? (long long)(int)gz : 0, glxyz = (long long)p.glx * p.gly * glz;
  const long long nodes = c.max_nodes > 0 ? c.max_nodes : glxyz;
  if (nodes < 1 || nodes > (1LL << 24)) { nep::set_last_error("the node pool (max_nodes, or GLX * GLY * GLZ) must hold 1 to 2^24 nodes"); return nullptr; }
  p.max_nodes = (int)nodes; p.max_pops = c.max_pops; p.hsig_cap = c.hsig_cap; p.cont_cap = c.cont_cap; p.path_cap = c.path_cap;
  p.hash_size = 16; while (p.hash_size < 2 * p.max_nodes) p.hash_size *= 2;
  const long long pool = (long long)NEP_HASTAR_POOL_PER_NODE * p.max_nodes;
  p.pool_cap = (int)(pool > c.cont_cap ? pool : c.cont_cap);      // the initial list always fits
  nep_hastar_t* h = new (std::nothrow) nep_hastar();
  if (!h) { nep::set_last_error("out of memory"); return nullptr; }
  h->cfg = c; h->par = p; h->n_scenes = n_scenes; h->scenes.resize(n_scenes);
  return h;
}

void nep_hastar_destroy(nep_hastar_t* h) {
  if (!h) return;
  if (h->dev && h->dev_free) h->dev_free(h->dev);
  delete h;
}

int nep_hastar_set_inflated(nep_hastar_t* h, int32_t scene, int32_t n_poly, const int32_t* off, const double* xy) { return set_polys(h, scene, n_poly, off, xy, true); }
int nep_hastar_set_uninflated(nep_hastar_t* h, int32_t scene, int32_t n_poly, const int32_t* off, const double* xy) { return set_polys(h, scene, n_poly, off, xy, false); }

int nep_hastar_set_reps(nep_hastar_t* h, int32_t scene, int32_t n_rep, const double* rep) {
  if (!h || scene < -1 || scene >= h->n_scenes || n_rep < 0 || (n_rep > 0 && !rep)) return fail(NEP_E_ARG, "bad arguments");
  if (n_rep > NEP_HASTAR_MAX_REP) return fail(NEP_E_CAP, "more than NEP_HASTAR_MAX_REP reps");
  for (int i = 0; i < 4 * n_rep; i++) if (!std::isfinite(rep[i])) return fail(NEP_E_ARG, "a rep is not finite");
  for (int s = scene < 0 ? 0 : scene; s < (scene < 0 ? h->n_scenes : scene + 1); s++) h->scenes[s].rep.assign(rep, rep + 4 * (size_t)n_rep);
  h->dirty = true;
  return 0;
}

int nep_hastar_inflate(int32_t n_vert, const double* xy, double drone_radius, double* xy_out, int32_t cap) {
  if (n_vert < 1 || !xy || !xy_out || cap < 1 || !(drone_radius >= 0.0) || !std::isfinite(drone_radius)) return fail(NEP_E_ARG, "bad arguments");
  const double sd = 2 * drone_radius;
  std::vector<std::pair<double, double>> pts;
  for (int j = 0; j < n_vert; j++) {
    const double x = xy[2 * j], y = xy[2 * j + 1];
    if (!std::isfinite(x) || !std::isfinite(y)) return fail(NEP_E_ARG, "a vertex is not finite");
    pts.push_back({x + sd, y + sd}); pts.push_back({x + sd, y - sd}); pts.push_back({x - sd, y + sd}); pts.push_back({x - sd, y - sd});
  }
  std::sort(pts.begin(), pts.end());
  pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
  const int n = (int)pts.size();
  std::vector<std::pair<double, double>> hull(2 * n);
  int k = 0;
  auto cross = [](const std::pair<double, double>& o, const std::pair<double, double>& a, const std::pair<double, double>& b) {
    return (a.first - o.first) * (b.second - o.second) - (a.second - o.second) * (b.first - o.first);
  };
  if (n < 3) { for (int i = 0; i < n; i++) hull[k++] = pts[i]; }
  else {
    for (int i = 0; i < n; i++) { while (k >= 2 && cross(hull[k - 2], hull[k - 1], pts[i]) <= 0) k--; hull[k++] = pts[i]; }
    for (int i = n - 2, t = k + 1; i >= 0; i--) { while (k >= t && cross(hull[k - 2], hull[k - 1], pts[i]) <= 0) k--; hull[k++] = pts[i]; }
    k--;
  }
  if (k > cap) return fail(NEP_E_CAP, "the inflated polygon does not fit xy_out");
  for (int i = 0; i < k; i++) { xy_out[2 * i] = hull[i].first; xy_out[2 * i + 1] = hull[i].second; }
  return k;
}

int nep_hastar_gjk(int32_t n1, const double* xy1, int32_t n2, const double* xy2) {
  if (n1 < 1 || n2 < 1 || !xy1 || !xy2) return fail(NEP_E_ARG, "bad arguments");
  return gjk_collision(xy1, n1, xy2, n2) ? 1 : 0;
}

int64_t nep_hastar_search_bytes(const nep_hastar_t* h) { return h ? (int64_t)work_bytes(h->par) : (int64_t)NEP_E_ARG; }

int nep_hastar_search_host(nep_hastar_t* h, int32_t n_search, const int32_t* scene, const double* start, const double* goal,
                           const nep_hastar_state* state_in, nep_hastar_result* result, double* path, const nep_hastar_state* state_out) {
  if (!h || n_search < 0) return fail(NEP_E_ARG, "bad arguments");
  if (n_search == 0) return 0;
  if (!scene || !start || !goal || !state_in || !result || !path || !state_out) return fail(NEP_E_ARG, "null argument");
  const Par& p = h->par;
  for (const nep_hastar_state* st : {state_in, state_out}) {
    if (st->hsig_cap != p.hsig_cap || st->cont_cap != p.cont_cap) return fail(NEP_E_ARG, "a state's caps are not the handle's");
    if (!st->n_hsig || !st->hsig_id || !st->hsig_sign || !st->n_cont || !st->cont) return fail(NEP_E_ARG, "a state array is null");
  }
  h->host_work.resize(work_bytes(p) + 16);
  char* mem = h->host_work.data();
  mem += (16 - ((uintptr_t)mem & 15)) & 15;
  SerialEx ex;
  for (int s = 0; s < n_search; s++) {
    const bool bad = scene[s] < 0 || scene[s] >= h->n_scenes;
    Scene sc = scene_view(h->scenes[bad ? 0 : scene[s]]);
    StateSlot in{state_in->n_hsig + s, state_in->hsig_id + (size_t)s * p.hsig_cap, state_in->hsig_sign + (size_t)s * p.hsig_cap, state_in->n_cont + s,
                 state_in->cont + (size_t)s * p.cont_cap * 2};
    StateSlot out{state_out->n_hsig + s, state_out->hsig_id + (size_t)s * p.hsig_cap, state_out->hsig_sign + (size_t)s * p.hsig_cap, state_out->n_cont + s,
                  state_out->cont + (size_t)s * p.cont_cap * 2};
    search(ex, p, sc, start + 2 * (size_t)s, goal + 2 * (size_t)s, in, mem, result + s, path + (size_t)s * p.path_cap * 2, out, bad);
    h->host_flags |= result[s].flags;
  }
  return 0;
}

}  // extern "C"
