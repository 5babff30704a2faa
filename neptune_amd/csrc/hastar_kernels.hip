// hastar_kernels.hip — the device form of the homotopic grid A* (include/neptune_hastar.h): one wave per search, as
// frontend_astar_kernel is.  The search itself is hastar_common.h's search<Ex>, the function the host form
// runs; here Ex spreads the dense parts over the wave's 64 lanes — the (neighbour x inflated polygon) occupancy tests, the crossing
// tests of a neighbour against every rep, the obstacle loop of each point updateContPts_orig samples — and gathers them with a
// ballot.  The serial parts are wave-uniform.  No LDS: a search's working set lives in its block of global memory
// (nep_hastar_search_bytes), whose hot lines stay in the CU's L1 and the L2.  Compiled with -ffp-contract=off: every output byte
// equals the host form's.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "hastar_common.h"

namespace nep { void set_last_error(const std::string& msg); }

using namespace nep_hastar_impl;

namespace {

struct SceneDesc { int n_infl, infl_off, infl_xy, n_un, un_off, un_xy, n_rep, rep; };      // counts, and where a scene's arrays start in the two blobs
struct StateDev { int32_t* n_hsig; int16_t* hsig_id; int8_t* hsig_sign; int32_t* n_cont; double* cont; };

struct WaveEx {
  static constexpr int W = 64;
  __device__ int lane() const { return (int)threadIdx.x; }
  __device__ uint64_t ballot(bool p) const { return __ballot(p); }
  __device__ void sync() const { __syncthreads(); }
};

__global__ __launch_bounds__(64) void hastar_kernel(Par p, int n_search, int n_scenes, const SceneDesc* descs, const int32_t* ints, const double* dbls,
                                                     const int32_t* d_scene, const double* d_start, const double* d_goal, StateDev in, nep_hastar_result* d_result,
                                                     double* d_path, StateDev out, char* ws, size_t ws_stride, int* d_flags) {
  const int s = (int)blockIdx.x;
  if (s >= n_search) return;
  const int scn = d_scene[s];
  const bool bad = scn < 0 || scn >= n_scenes;
  Scene sc;
  const SceneDesc D = descs[bad ? 0 : scn];
  sc.n_infl = D.n_infl; sc.infl_off = ints + D.infl_off; sc.infl_xy = dbls + D.infl_xy;
  sc.n_un = D.n_un; sc.un_off = ints + D.un_off; sc.un_xy = dbls + D.un_xy;
  sc.n_rep = D.n_rep; sc.rep = dbls + D.rep;
  StateSlot si{in.n_hsig + s, in.hsig_id + (size_t)s * p.hsig_cap, in.hsig_sign + (size_t)s * p.hsig_cap, in.n_cont + s, in.cont + (size_t)s * p.cont_cap * 2};
  StateSlot so{out.n_hsig + s, out.hsig_id + (size_t)s * p.hsig_cap, out.hsig_sign + (size_t)s * p.hsig_cap, out.n_cont + s, out.cont + (size_t)s * p.cont_cap * 2};
  WaveEx ex;
  search(ex, p, sc, d_start + 2 * (size_t)s, d_goal + 2 * (size_t)s, si, ws + (size_t)s * ws_stride, d_result + s, d_path + (size_t)s * p.path_cap * 2, so, bad);
  if (threadIdx.x == 0 && d_result[s].flags) atomicOr(d_flags, d_result[s].flags);
}

struct Dev {
  char* ws = nullptr; int ws_searches = 0; size_t ws_stride = 0;
  SceneDesc* descs = nullptr; int32_t* ints = nullptr; double* dbls = nullptr;
  int* flags = nullptr;
};
void dev_free(void* q) {
  Dev* d = (Dev*)q;
  (void)hipFree(d->ws); (void)hipFree(d->descs); (void)hipFree(d->ints); (void)hipFree(d->dbls); (void)hipFree(d->flags);
  delete d;
}
int fail(int rc, const std::string& msg) { nep::set_last_error(msg); return rc; }
#define HA_HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(NEP_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

int upload_scenes(nep_hastar_t* h, Dev* d) {
  std::vector<SceneDesc> descs(h->n_scenes);
  std::vector<int32_t> ints; std::vector<double> dbls;
  for (int s = 0; s < h->n_scenes; s++) {
    const SceneHost& S = h->scenes[s]; SceneDesc& D = descs[s];
    D.n_infl = (int)S.infl_off.size() - 1; D.infl_off = (int)ints.size(); ints.insert(ints.end(), S.infl_off.begin(), S.infl_off.end());
    D.infl_xy = (int)dbls.size(); dbls.insert(dbls.end(), S.infl_xy.begin(), S.infl_xy.end());
    D.n_un = (int)S.un_off.size() - 1; D.un_off = (int)ints.size(); ints.insert(ints.end(), S.un_off.begin(), S.un_off.end());
    D.un_xy = (int)dbls.size(); dbls.insert(dbls.end(), S.un_xy.begin(), S.un_xy.end());
    D.n_rep = (int)(S.rep.size() / 4); D.rep = (int)dbls.size(); dbls.insert(dbls.end(), S.rep.begin(), S.rep.end());
    if (dbls.size() > 0x3fffffffu || ints.size() > 0x3fffffffu) return fail(NEP_E_CAP, "the scenes' statics exceed 2^30 values");
  }
  dbls.push_back(0.0);      // (never empty)
  HA_HIPCHK(hipDeviceSynchronize());
  (void)hipFree(d->descs); (void)hipFree(d->ints); (void)hipFree(d->dbls); d->descs = nullptr; d->ints = nullptr; d->dbls = nullptr;
  HA_HIPCHK(hipMalloc((void**)&d->descs, descs.size() * sizeof(SceneDesc)));
  HA_HIPCHK(hipMalloc((void**)&d->ints, ints.size() * sizeof(int32_t)));
  HA_HIPCHK(hipMalloc((void**)&d->dbls, dbls.size() * sizeof(double)));
  HA_HIPCHK(hipMemcpy(d->descs, descs.data(), descs.size() * sizeof(SceneDesc), hipMemcpyHostToDevice));
  HA_HIPCHK(hipMemcpy(d->ints, ints.data(), ints.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  HA_HIPCHK(hipMemcpy(d->dbls, dbls.data(), dbls.size() * sizeof(double), hipMemcpyHostToDevice));
  h->dirty = false;
  return 0;
}

}  // namespace

extern "C" {

int nep_hastar_search(nep_hastar_t* h, int32_t n_search, const int32_t* d_scene, const double* d_start, const double* d_goal,
                      const nep_hastar_state* d_state_in, nep_hastar_result* d_result, double* d_path, const nep_hastar_state* d_state_out, void* stream) {
  if (!h || n_search < 0) return fail(NEP_E_ARG, "bad arguments");
  if (n_search == 0) return 0;
  if (!d_scene || !d_start || !d_goal || !d_state_in || !d_result || !d_path || !d_state_out) return fail(NEP_E_ARG, "null argument");
  const Par& p = h->par;
  for (const nep_hastar_state* st : {d_state_in, d_state_out}) {
    if (st->hsig_cap != p.hsig_cap || st->cont_cap != p.cont_cap) return fail(NEP_E_ARG, "a state's caps are not the handle's");
    if (!st->n_hsig || !st->hsig_id || !st->hsig_sign || !st->n_cont || !st->cont) return fail(NEP_E_ARG, "a state array is null");
  }
  Dev* d = (Dev*)h->dev;
  if (!d) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) return fail(NEP_E_HIP, "no HIP device");
    d = new Dev();
    h->dev = d; h->dev_free = dev_free;
    HA_HIPCHK(hipMalloc((void**)&d->flags, sizeof(int)));
    HA_HIPCHK(hipMemset(d->flags, 0, sizeof(int)));
  }
  if (h->dirty) { const int rc = upload_scenes(h, d); if (rc < 0) return rc; }
  if (n_search > d->ws_searches) {
    HA_HIPCHK(hipDeviceSynchronize());
    (void)hipFree(d->ws); d->ws = nullptr; d->ws_searches = 0;
    d->ws_stride = work_bytes(p);
    HA_HIPCHK(hipMalloc((void**)&d->ws, d->ws_stride * (size_t)n_search));
    d->ws_searches = n_search;
  }
  StateDev in{d_state_in->n_hsig, d_state_in->hsig_id, d_state_in->hsig_sign, d_state_in->n_cont, d_state_in->cont};
  StateDev out{d_state_out->n_hsig, d_state_out->hsig_id, d_state_out->hsig_sign, d_state_out->n_cont, d_state_out->cont};
  hipLaunchKernelGGL(hastar_kernel, dim3((unsigned)n_search), dim3(64), 0, (hipStream_t)stream, p, (int)n_search, h->n_scenes, d->descs, d->ints, d->dbls,
                     d_scene, d_start, d_goal, in, d_result, d_path, out, d->ws, d->ws_stride, d->flags);
  HA_HIPCHK(hipGetLastError());
  return 0;
}

int nep_hastar_check(nep_hastar_t* h, void* stream) {
  if (!h) return fail(NEP_E_ARG, "bad arguments");
  int flags = h->host_flags;
  h->host_flags = 0;
  Dev* d = (Dev*)h->dev;
  if (d) {
    int dev_flags = 0;
    HA_HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    HA_HIPCHK(hipMemcpy(&dev_flags, d->flags, sizeof(int), hipMemcpyDeviceToHost));
    if (dev_flags) HA_HIPCHK(hipMemset(d->flags, 0, sizeof(int)));
    flags |= dev_flags;
  }
  if (flags) return fail(NEP_E_CAP, "a search hit a capacity: nep_hastar_result.flags says which (" + std::to_string(flags) + ")");
  return 0;
}

}  // extern "C"
