// audit_kernels.hip — device form of the flight audit (nep_batch_audit, include/neptune_frontend.h): the clearances of what every
// agent of every scene flies, at the control ticks.  The arithmetic is audit_common.h's, which nep_audit_records (audit_host.cpp)
// shares; the device equals that host form bit for bit — built -ffp-contract=off like geom_kernels.hip.
#include <hip/hip_runtime.h>

#define NEP_AUDIT_FN __device__ inline
#include "nep_device.h"
#include "audit_common.h"

namespace nep {

using namespace nep_audit_impl;

static_assert(sizeof(AuditPart) == 56, "AuditPart is sized by hand in backend.hip's scratch");

namespace {

// One workgroup per (scene, run of ticks), one thread per agent.  The scene's polygons go into LDS once, with one reciprocal
// squared length per edge.  At every tick a thread evaluates its own record once and puts centre and box half-widths into LDS;
// after the barrier it walks all N entries and all polygon edges — every lane reads the same address, which LDS serves as a
// broadcast, and both loops are wave-uniform.  The running minima live in registers and go to the run's AuditPart.
__global__ __launch_bounds__(1024) void audit_chunk_kernel(AuditArgs aa) {
  extern __shared__ __attribute__((aligned(16))) unsigned char au_lds[];
  const int N = aa.N, S = aa.S, vs = aa.vstride;
  const int scene = blockIdx.x / aa.n_chunks, chunk = blockIdx.x - scene * aa.n_chunks;
  const int a = threadIdx.x;
  const AuditLayout L = audit_layout(N, S, vs);      // (lds_layout.h)
  double* pxy = lds_at<double>(au_lds, L.pxy);       // [S][vs][2] polygon vertices
  double* pinv = lds_at<double>(au_lds, L.pinv);     // [S][vs] 1 / |edge|^2
  double* ag = lds_at<double>(au_lds, L.ag);         // [N][4] x, y, hx, hy
  int* pnv = lds_at<int>(au_lds, L.pnv);             // [S] vertex counts (clamped to vs)
  int* apres = lds_at<int>(au_lds, L.apres);         // [N]
  const long sbase = (long)scene * aa.static_stride;
  for (int j = a; j < S; j += blockDim.x) { const int c = aa.static_nv[sbase + j]; pnv[j] = c < 0 ? 0 : (c > vs ? vs : c); }
  for (int e = a; e < S * vs; e += blockDim.x) {
    const int j = e / vs, v = e - j * vs;
    int c = aa.static_nv[sbase + j]; c = c < 0 ? 0 : (c > vs ? vs : c);
    const double* q = aa.static_xy + (sbase + j) * kHullV * 2;
    double x = 0.0, y = 0.0, inv = 0.0;
    if (v < c) { const int w = v + 1 == c ? 0 : v + 1; x = q[2 * v]; y = q[2 * v + 1]; inv = audit_edge_inv(x, y, q[2 * w], q[2 * w + 1]); }
    pxy[2 * e] = x; pxy[2 * e + 1] = y; pinv[e] = inv;
  }
  const nep_traj_rec* r = aa.recs + (long)scene * N + (a < N ? a : 0);
  const bool me = a < N && audit_present(r);
  if (a < N) {
    apres[a] = me;
    ag[4 * a + 2] = r->bbox[0] / 2 + aa.drone_radius; ag[4 * a + 3] = r->bbox[1] / 2 + aa.drone_radius;
  }
  const double t0 = aa.starts[(long)scene * N].t_start;
  const double inf = __builtin_huge_val();
  AuditPart P;
  P.c_d2 = inf; P.box = inf; P.stat = inf; P.c_k = P.b_k = P.s_k = 0; P.c_p = P.b_p = P.s_i = -1; P.n_pair = P.n_stat = 0;
  const int k_lo = chunk * aa.chunk_len, k_hi = min(k_lo + aa.chunk_len, aa.n_ticks);
  for (int k = k_lo; k < k_hi; k++) {
    const double t = t0 + (double)k * aa.tick;
    double px = 0.0, py = 0.0;
    __syncthreads();      // (the previous tick's readers are done; at the first tick: the staging above is visible)
    if (me) { const AuditState s = audit_eval(r, t); px = s.x; py = s.y; ag[4 * a] = px; ag[4 * a + 1] = py; }
    __syncthreads();
    if (!me) continue;    // (k is uniform: every thread meets both barriers of every tick)
    double tb = inf; int tbp = -1;
    for (int j = 0; j < N; j++) {
      if (!apres[j]) continue;
      const double dx = px - ag[4 * j], dy = py - ag[4 * j + 1];
      const double d2 = dx * dx + dy * dy;
      const double bc = audit_box_clear(dx, dy, ag[4 * j + 2], ag[4 * j + 3]);
      const bool other = j != a;
      if (other && d2 < P.c_d2) { P.c_d2 = d2; P.c_p = j + 1; P.c_k = k; }
      if (other && bc < tb) { tb = bc; tbp = j + 1; }
    }
    if (tb < P.box) { P.box = tb; P.b_p = tbp; P.b_k = k; }
    if (tb < 0.0) P.n_pair++;
    double ts = inf; int tsi = -1;
    for (int j = 0; j < S; j++) {
      const int c = pnv[j];
      if (c < 1) continue;
      const double* q = pxy + (size_t)j * vs * 2;
      const double* qi = pinv + (size_t)j * vs;
      double d2 = inf; bool inside = true;
      for (int v = 0; v < c; v++) { const int w = v + 1 == c ? 0 : v + 1; audit_edge(px, py, q[2 * v], q[2 * v + 1], q[2 * w], q[2 * w + 1], qi[v], d2, inside); }
      const double sd = audit_signed(d2, inside, c);
      if (sd < ts) { ts = sd; tsi = j; }
    }
    if (ts < P.stat) { P.stat = ts; P.s_i = tsi; P.s_k = k; }
    if (ts < 0.0) P.n_stat++;
  }
  if (me) aa.part[((long)scene * aa.n_chunks + chunk) * N + a] = P;
}

// One thread per (scene, agent): the runs' minima merged in tick order (strictly smaller wins, so the earlier tick keeps a tie),
// then path length and top speed, sums and maxima over the call's ticks in tick order.
__global__ void audit_merge_kernel(AuditArgs aa) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = aa.N;
  if (idx >= (long)aa.n_scenes * N) return;
  const int scene = (int)(idx / N), a = (int)(idx - (long)scene * N);
  const nep_traj_rec* r = aa.recs + idx;
  if (!audit_present(r)) return;
  const double t0 = aa.starts[(long)scene * N].t_start;
  nep_audit A = aa.out[idx];
  for (int c = 0; c < aa.n_chunks; c++) {
    const AuditPart P = aa.part[((long)scene * aa.n_chunks + c) * N + a];
    if (P.c_d2 < A.center_d2) { A.center_d2 = P.c_d2; A.center_partner = P.c_p; A.t_center = t0 + (double)P.c_k * aa.tick; }
    if (P.box < A.min_box_clear) { A.min_box_clear = P.box; A.box_partner = P.b_p; A.t_box = t0 + (double)P.b_k * aa.tick; }
    if (P.stat < A.min_static_dist) { A.min_static_dist = P.stat; A.static_index = P.s_i; A.t_static = t0 + (double)P.s_k * aa.tick; }
    A.n_pair_viol += P.n_pair; A.n_static_viol += P.n_stat;
  }
  A.min_center_dist = sqrt(A.center_d2);
  audit_path(r, t0, aa.tick, aa.n_ticks, &A);
  aa.out[idx] = A;
}

}  // namespace

void launch_audit(const AuditArgs& aa, hipStream_t st) {
  if (aa.n_scenes <= 0 || aa.N <= 0 || aa.n_ticks <= 0) return;
  const unsigned threads = (unsigned)((aa.N + 63) / 64 * 64);
  hipLaunchKernelGGL(audit_chunk_kernel, dim3((unsigned)(aa.n_scenes * aa.n_chunks)), dim3(threads), (size_t)audit_layout(aa.N, aa.S, aa.vstride).bytes, st, aa);
  const long total = (long)aa.n_scenes * aa.N;
  hipLaunchKernelGGL(audit_merge_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, st, aa);
}

}  // namespace nep
