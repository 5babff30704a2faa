// mtlp_kernels.hip — the device form of the MTLP comparator (include/neptune_mtlp.h).  Two kernels per call: the order graph, one
// lane per ordered pair (i, j) of a run, and the searches, one wave per (run, robot), as hastar_kernel is.
// The rule set is mtlp_common.h's, the functions the host form runs; here Ex spreads an expansion's (neighbour x cable line) tests
// over the wave's 64 lanes and gathers them with a ballot.  The serial parts are wave-uniform.  No LDS: a search's working set
// lives in its block of global memory (nep_mtlp_search_bytes).  Compiled with -ffp-contract=off: every output byte equals the host
// form's.
#include <hip/hip_runtime.h>

#include <string>

#include "mtlp_common.h"

namespace nep { void set_last_error(const std::string& msg); }

using namespace nep_mtlp_impl;

namespace {

struct WaveEx {
  static constexpr int W = 64;
  __device__ int lane() const { return (int)threadIdx.x; }
  __device__ uint64_t ballot(bool p) const { return __ballot(p); }
  __device__ void sync() const { __syncthreads(); }
};

__global__ __launch_bounds__(256) void mtlp_graph_kernel(int n, long long n_entries, const double* d_bases, const double* d_sg, int32_t* d_graph, int32_t* d_run_status) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_entries) return;
  const int nn = n * n, r = (int)(e / nn), ij = (int)(e - (long long)r * nn), i = ij / n, j = ij - i * n;
  const double* b = d_bases + (size_t)r * n * 3; const double* sg = d_sg + (size_t)r * n * 6;
  const bool ok = run_in_domain(b, sg, n);
  d_graph[e] = ok ? graph_entry(b, sg, i, j) : 0;
  if (ij == 0) d_run_status[r] = ok ? 1 : NEP_E_STATE;
}

__global__ __launch_bounds__(64) void mtlp_search_kernel(Par p, int n_search, const double* d_bases, const double* d_sg, const int32_t* d_graph,
                                                          nep_mtlp_result* d_result, double* d_path, char* ws, size_t ws_stride, int* d_flags) {
  const int s = (int)blockIdx.x;
  if (s >= n_search) return;
  const int r = s / p.n, me = s - r * p.n;
  const double* b = d_bases + (size_t)r * p.n * 3; const double* sg = d_sg + (size_t)r * p.n * 6;
  const bool ok = run_in_domain(b, sg, p.n);
  WaveEx ex;
  search(ex, p, b, sg, d_graph + (size_t)r * p.n * p.n, me, ok, ws + (size_t)s * ws_stride, d_result + s, d_path + (size_t)s * p.path_cap * 3);
  const int f = d_result[s].flags & (NEP_MTLP_FLAG_PATH | NEP_MTLP_FLAG_STATE);
  if (threadIdx.x == 0 && f) atomicOr(d_flags, f);
}

__global__ __launch_bounds__(64) void mtlp_predicates_kernel(int which, int n, const double* in, int32_t* verdict, int32_t* exact) {
  const int k = (int)(blockIdx.x * 64 + threadIdx.x);
  if (k >= n) return;
  const double* q = in + 16 * (size_t)k;
  int nex = 0;
  if (which == 0) verdict[k] = seg_tri(q, q + 3, q + 6, q + 9, q + 12, nex);
  else if (which == 1) verdict[k] = seg_seg2(q, q + 3, q + 6, q + 9, 0, 1, nex);
  else verdict[k] = ball_seg(q, q[9], q + 3, q + 6, nex);
  exact[k] = nex;
}

struct Dev { char* ws = nullptr; long long ws_searches = 0; size_t ws_stride = 0; int* flags = nullptr; };
void dev_free(void* q) {
  Dev* d = (Dev*)q;
  (void)hipFree(d->ws); (void)hipFree(d->flags);
  delete d;
}
int fail(int rc, const std::string& msg) { nep::set_last_error(msg); return rc; }
#define MT_HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(NEP_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

}  // namespace

extern "C" {

int nep_mtlp_solve(nep_mtlp_t* h, int32_t n_runs, const double* d_bases, const double* d_start_goal, int32_t* d_graph, int32_t* d_run_status,
                   nep_mtlp_result* d_result, double* d_path, void* stream) {
  if (!h || n_runs < 0) return fail(NEP_E_ARG, "bad arguments");
  if (n_runs == 0) return 0;
  if (!d_bases || !d_start_goal || !d_graph || !d_run_status || !d_result || !d_path) return fail(NEP_E_ARG, "null argument");
  const Par& p = h->par;
  const long long n_search = (long long)n_runs * p.n, n_entries = n_search * p.n;
  if (n_search > 0x7fffffffLL || n_entries > (1LL << 38)) return fail(NEP_E_CAP, "too many runs for one launch");
  Dev* d = (Dev*)h->dev;
  if (!d) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) return fail(NEP_E_HIP, "no HIP device");
    d = new Dev();
    h->dev = d; h->dev_free = dev_free;
    MT_HIPCHK(hipMalloc((void**)&d->flags, sizeof(int)));
    MT_HIPCHK(hipMemset(d->flags, 0, sizeof(int)));
  }
  if (n_search > d->ws_searches) {
    MT_HIPCHK(hipDeviceSynchronize());
    (void)hipFree(d->ws); d->ws = nullptr; d->ws_searches = 0;
    d->ws_stride = work_bytes(p);
    MT_HIPCHK(hipMalloc((void**)&d->ws, d->ws_stride * (size_t)n_search));
    d->ws_searches = n_search;
  }
  hipLaunchKernelGGL(mtlp_graph_kernel, dim3((unsigned)((n_entries + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p.n, n_entries, d_bases, d_start_goal,
                     d_graph, d_run_status);
  MT_HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(mtlp_search_kernel, dim3((unsigned)n_search), dim3(64), 0, (hipStream_t)stream, p, (int)n_search, d_bases, d_start_goal,
                     (const int32_t*)d_graph, d_result, d_path, d->ws, d->ws_stride, d->flags);
  MT_HIPCHK(hipGetLastError());
  return 0;
}

int nep_mtlp_check(nep_mtlp_t* h, void* stream) {
  if (!h) return fail(NEP_E_ARG, "bad arguments");
  int flags = h->host_flags & (NEP_MTLP_FLAG_PATH | NEP_MTLP_FLAG_STATE);
  h->host_flags = 0;
  Dev* d = (Dev*)h->dev;
  if (d) {
    int dev_flags = 0;
    MT_HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    MT_HIPCHK(hipMemcpy(&dev_flags, d->flags, sizeof(int), hipMemcpyDeviceToHost));
    if (dev_flags) MT_HIPCHK(hipMemset(d->flags, 0, sizeof(int)));
    flags |= dev_flags;
  }
  if (flags) return fail(NEP_E_CAP, "a search hit a capacity or a run left the domain: nep_mtlp_result.flags says which (" + std::to_string(flags) + ")");
  return 0;
}

int nep_mtlp_predicates_device(int32_t which, int32_t n, const double* d_in, int32_t* d_verdict, int32_t* d_exact, void* stream) {
  if (which < 0 || which > 2 || n < 0 || (n > 0 && (!d_in || !d_verdict || !d_exact))) return fail(NEP_E_ARG, "bad arguments");
  if (n == 0) return 0;
  hipLaunchKernelGGL(mtlp_predicates_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (int)which, (int)n, d_in, d_verdict, d_exact);
  MT_HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
