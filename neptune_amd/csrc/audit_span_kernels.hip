// audit_span_kernels.hip — device form of the span audit (nep_batch_audit_span, include/neptune_frontend.h): the
// minima of the flight audit's three clearances over the whole window of a call, not only at its ticks.  The rule is
// audit_span_common.h's, which nep_span_audit_records (audit_span_host.cpp) shares; the device equals that host form byte for byte —
// built -ffp-contract=off like audit_kernels.hip.
#include <hip/hip_runtime.h>

#define NEP_AUDIT_FN __device__ inline
#define NEP_SPAN_MFN __device__ inline
#include "nep_device.h"
#include "audit_span_common.h"

namespace nep {

using namespace nep_span_impl;

namespace {

constexpr int kSpanWaves = 4;      // agents per workgroup, one wave each: they share the scene's staging

__device__ inline SpanAuditLayout span_layout(int N, int S, int vs) { return span_audit_layout(N, S, vs, kSpanLdsPieces, (int)sizeof(SpanPiece)); }

__device__ inline void span_shfl_min(SpanMin& m, int off) {
  const double v = __shfl_xor(m.v, off), t = __shfl_xor(m.t, off);
  const int who = __shfl_xor(m.who, off);
  span_take(m, v, t, who);
}

__device__ inline void span_wave_merge(SpanCall& c) {      // every lane of the wave gets the wave's minima
  for (int off = 32; off >= 1; off >>= 1) {
    span_shfl_min(c.center, off); span_shfl_min(c.box, off); span_shfl_min(c.stat, off);
    const double tb = __shfl_xor(c.tick_box, off), tsd = __shfl_xor(c.tick_stat, off);
    if (tb < c.tick_box) c.tick_box = tb;
    if (tsd < c.tick_stat) c.tick_stat = tsd;
  }
}

constexpr int kSpanBatches = 8;      // batches of 64 items a wave sorts into kept and skipped: 512 partners and polygons (beyond: nobody is skipped)

// One workgroup per (scene, kSpanWaves agents).  The workgroup stages the scene once: its polygons with one reciprocal squared
// length per edge (as audit_chunk_kernel does), and of every agent the first pieces of its record inside the window (kSpanLdsPieces;
// a record with more is read from global memory, which gives the same pieces) and a box round its positions over the window.  Then
// one wave audits one agent.  Its lanes take the partners and the polygons: first everybody at the call's ticks — the tick audit's
// work, and the minima it gives bound what the window can still hold — then the whole window of the items the boxes do not rule
// out (span_skip_pair, span_skip_poly), dealt out again over the lanes, one (agent, partner) or (agent, polygon) walk each: serial,
// divergent root finding.  The wave merges its lanes' findings in registers by the tie rule, which does not depend on who found
// what, and lane 0 folds the call into the agent's record.
__global__ __launch_bounds__(kSpanWaves * 64) void span_audit_kernel(SpanAuditArgs sa) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sp_lds[];
  const int N = sa.N, S = sa.S, vs = sa.vstride;
  const int groups = (N + kSpanWaves - 1) / kSpanWaves;
  const int scene = blockIdx.x / groups, grp = blockIdx.x - scene * groups;
  const int tid = threadIdx.x;
  const SpanAuditLayout L = span_layout(N, S, vs);      // (lds_layout.h)
  double* pxy = lds_at<double>(sp_lds, L.pxy);
  double* pinv = lds_at<double>(sp_lds, L.pinv);
  SpanPiece* pc = lds_rec<SpanPiece>(sp_lds, (int)L.pc);
  double* ts = lds_at<double>(sp_lds, L.ts);
  double* hxy = lds_at<double>(sp_lds, L.hxy);
  double* box = lds_at<double>(sp_lds, L.box);
  int* pnv = lds_at<int>(sp_lds, L.pnv);
  int* npc = lds_at<int>(sp_lds, L.npc);
  int* apres = lds_at<int>(sp_lds, L.apres);
  const long sbase = (long)scene * sa.static_stride;
  for (int j = tid; j < S; j += blockDim.x) { const int c = sa.static_nv[sbase + j]; pnv[j] = c < 0 ? 0 : (c > vs ? vs : c); }
  for (int e = tid; e < S * vs; e += blockDim.x) {
    const int j = e / vs, v = e - j * vs;
    int c = sa.static_nv[sbase + j]; c = c < 0 ? 0 : (c > vs ? vs : c);
    const double* q = sa.static_xy + (sbase + j) * kHullV * 2;
    double x = 0.0, y = 0.0, inv = 0.0;
    if (v < c) { const int w = v + 1 == c ? 0 : v + 1; x = q[2 * v]; y = q[2 * v + 1]; inv = audit_edge_inv(x, y, q[2 * w], q[2 * w + 1]); }
    pxy[2 * e] = x; pxy[2 * e + 1] = y; pinv[e] = inv;
  }
  const nep_traj_rec* recs = sa.recs + (long)scene * N;
  const SpanWin w = span_win(sa.starts[(long)scene * N].t_start, sa.tick, sa.n_ticks);
  for (int a = tid; a < N; a += blockDim.x) {
    const nep_traj_rec* r = recs + a;
    const bool pres = audit_present(r);
    apres[a] = pres;
    hxy[2 * a] = r->bbox[0] / 2 + sa.drone_radius; hxy[2 * a + 1] = r->bbox[1] / 2 + sa.drone_radius;
    npc[a] = pres ? span_stage(r, w.t0, w.t1, ts + a * kSpanLdsPieces, pc + a * kSpanLdsPieces, box + 4 * a) : 0;
  }
  __syncthreads();      // (the only barrier: a wave may leave behind it)
  const int a = grp * kSpanWaves + (tid >> 6), lane = tid & 63;
  if (a >= N || !apres[a]) return;
  SpanCall c;
  span_call_init(c);
  const SpanSrc A{recs + a, ts + a * kSpanLdsPieces, pc + a * kSpanLdsPieces, npc[a]};
  auto walk = [&](int item, bool ticks_only) {
    if (item < N) {
      const int j = item;
      SpanPairWalk W{recs + a, recs + j, A, SpanSrc{recs + j, ts + j * kSpanLdsPieces, pc + j * kSpanLdsPieces, npc[j]}, j + 1, hxy[2 * j], hxy[2 * j + 1], &c};
      if (ticks_only) span_ticks(w, W); else span_intervals(w, W);
    } else {
      const int j = item - N;
      SpanPolyWalk W{recs + a, A, pxy + (size_t)j * vs * 2, pinv + (size_t)j * vs, pnv[j], j, &c};
      if (ticks_only) span_ticks(w, W); else span_intervals(w, W);
    }
  };
  auto there = [&](int item) { return item < N ? (item != a && apres[item] != 0) : (item < N + S && pnv[item - N] >= 1); };
  for (int item = lane; item < N + S; item += 64) if (there(item)) walk(item, true);
  span_wave_merge(c);      // (every lane of the wave is here: a and apres[a] are the wave's)
  const SpanCall u = c;
  // who is kept, one bit per item; then kept item number lane, lane + 64, ... is this lane's
  unsigned long long keep[kSpanBatches];
  int total = 0;
  const int batches = (N + S + 63) / 64;
  for (int b = 0; b < kSpanBatches; b++) {
    keep[b] = 0;
    if (b >= batches) continue;
    const int item = b * 64 + lane;
    bool k = there(item);
    if (k && batches <= kSpanBatches) {
      k = item < N ? !span_skip_pair(box + 4 * a, box + 4 * item, hxy[2 * item], hxy[2 * item + 1], u.center.v, u.box.v)
                   : !span_skip_poly(box + 4 * a, pxy + (size_t)(item - N) * vs * 2, pnv[item - N], u.stat.v);
    }
    keep[b] = __ballot(k);
    total += __popcll(keep[b]);
  }
  if (batches <= kSpanBatches) {
    for (int n = lane; n < total; n += 64) {
      int left = n, b = 0;
      while (left >= __popcll(keep[b])) { left -= __popcll(keep[b]); b++; }
      unsigned long long m = keep[b];
      for (int i = 0; i < left; i++) m &= m - 1;
      walk(b * 64 + (__ffsll((long long)m) - 1), false);
    }
  } else {      // (more items than the bit sets hold: everybody's whole window)
    for (int item = lane; item < N + S; item += 64) if (there(item)) walk(item, false);
  }
  span_wave_merge(c);
  if (lane == 0) {
    nep_span_audit* out = sa.out + (long)scene * N + a;
    nep_span_audit R = *out;
    span_fold(c, w, &R);
    *out = R;
  }
}

}  // namespace

long long span_audit_lds_bytes(int N, int S, int vstride) { return span_audit_layout(N, S, vstride, kSpanLdsPieces, (int)sizeof(SpanPiece)).bytes; }

// more than 64 KB of dynamic LDS has to be asked for, per device: nep_batch_audit_span does on every call, which changes something
// only when the bytes have grown — at the first call, made outside any capture
hipError_t prepare_audit_span(long long lds_bytes) {
  static DynLdsAttr attr;
  return attr.ensure((const void*)span_audit_kernel, (size_t)lds_bytes);
}

void launch_audit_span(const SpanAuditArgs& sa, hipStream_t st) {
  if (sa.n_scenes <= 0 || sa.N <= 0 || sa.n_ticks <= 0) return;
  const int groups = (sa.N + kSpanWaves - 1) / kSpanWaves;
  hipLaunchKernelGGL(span_audit_kernel, dim3((unsigned)(sa.n_scenes * groups)), dim3(kSpanWaves * 64), (size_t)span_audit_lds_bytes(sa.N, sa.S, sa.vstride), st, sa);
}

}  // namespace nep
