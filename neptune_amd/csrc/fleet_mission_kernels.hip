// fleet_mission_kernels.hip — the mission controller of the device fleet loop (nep_batch_fleet_mission, include/neptune_fleet.h):
// successive goals, timeouts and leg records of every slot inside the captured round.  The arithmetic is mission_common.h's, which
// the host form (mission_host.cpp: nep_mission_step) shares; the device equals the host chain byte for byte — built
// -ffp-contract=off like fleet_kernels.hip.
//
// Layout: one wave (one 64-thread workgroup) per scene.  Lanes stride over the agents for the walk over the round's ticks and the
// triggers, and leave in LDS every agent's end position and what the call has to do for it.  The agents that need a goal are then
// taken in agent order (mode PER_AGENT: the set bits of a ballot per 64 agents; the run modes: everyone), and a draw is
// cooperative: lane l evaluates candidate k = 64 b + l against all five tests, the winner is the lowest set bit of the ballot, and
// batches b go on until one is found or max_attempts is reached — a serial rejection loop's result, whatever the scheduling.  The
// slot's owner lane (agent mod 64) writes the record, the totals and the goal with plain stores; the only atomic is the sticky
// global flag on the no-goal path.  Every branch around a barrier or a ballot depends on kernel arguments, on values all lanes
// load from the same address, or on a ballot's result.
// With a script (nep_batch_fleet_mission_script) the draw is replaced by a read of the slot's table: the length comes from device memory
// — one address, uniform — so a table replaced between replays of a captured round is the one that is read.
#include <hip/hip_runtime.h>

#define NEP_MISSION_FN __device__ inline
#include "nep_device.h"
#include "mission_common.h"

namespace nep {

using namespace nep_mission_impl;

static_assert(sizeof(nep_mission_cfg) == 136, "nep_mission_cfg is mirrored by hand in neptune_amd/abi.py");
static_assert(sizeof(nep_mission_leg) == 64, "nep_mission_leg is mirrored by hand in neptune_amd/abi.py");

namespace {

__device__ inline MissionSlot mission_slot(const FleetMissionArgs& ma, const FleetArgs& fa, long slot) {
  return MissionSlot{fa.goal + slot * 3, fa.done + slot, fa.sflags + slot, ma.t_issue + slot, ma.length + slot, ma.completed + slot, ma.counts + slot * 4, ma.sums + slot * 2};
}

// The draw of agent a by the whole wave: the accepted candidate of lowest k (-1: none of max_attempts), the same in every lane.
__device__ inline int mission_draw(const nep_mission_cfg& c, int lane, uint64_t h1, int a, int N, const double* end_pos, const double* pb, int n_poly,
                                   const int* poly_off, const double* poly_xy, const double* new_goal, const int* got, double& gx, double& gy) {
  for (int b = 0; b < c.max_attempts; b += 64) {
    double x, y;
    mission_candidate(c, h1, b + lane, x, y);
    const bool ok = mission_accept(c, x, y, a, N, end_pos, pb, n_poly, poly_off, poly_xy, new_goal, got);
    const unsigned long long m = __ballot(ok);
    if (m) {
      const int w = __ffsll((long long)m) - 1;
      gx = __shfl(x, w, 64); gy = __shfl(y, w, 64);
      return b + w;
    }
  }
  return -1;
}

// A scripted goal of `slot` (nep_batch_fleet_mission_script): row (issued - 1) mod n_goals of its table; every lane reads the same
// three doubles.  Returns k = 0: found.
__device__ inline int mission_scripted(const FleetMissionArgs& ma, long slot, int n_goals, double& gx, double& gy, double& gz) {
  const double* g = ma.script + (slot * n_goals + mission_script_row(ma.counts[slot * 4 + kIssued], n_goals)) * 3;
  gx = g[0]; gy = g[1]; gz = g[2];
  return 0;
}

__global__ __launch_bounds__(64) void fleet_mission_kernel(FleetMissionArgs ma, FleetArgs fa) {
  extern __shared__ __attribute__((aligned(16))) double ms_lds[];
  const int scene = blockIdx.x, lane = threadIdx.x;
  const int N = fa.N, T = fa.cfg.round_ticks, cap = fa.cap;
  const nep_mission_cfg& c = ma.cfg;
  int* scene_i = ma.scene_i + scene * 4;
  if (scene_i[kFinished]) return;                      // (one address for every lane: uniform)
  const int n_poly = ma.kn[scene];
  const int* g_off = ma.koff + (long)scene * (NEP_MISSION_MAX_POLY + 1);
  const int n_vert = n_poly > 0 ? g_off[n_poly] : 0;
  // the carve (lds_layout.h): end positions [N][3], goals drawn in this call [N][3] (before that: the leg lengths), keep-out vertices,
  // what to do per agent [N], polygon offsets
  const MissionLayout L = mission_layout(N, n_vert, n_poly);
  double* s_end = lds_at<double>(ms_lds, L.s_end);
  double* s_new = lds_at<double>(ms_lds, L.s_new);
  double* s_kxy = lds_at<double>(ms_lds, L.s_kxy);
  int* s_got = lds_at<int>(ms_lds, L.s_got);
  int* s_off = lds_at<int>(ms_lds, L.s_off);
  for (int i = lane; i < 2 * n_vert; i += 64) s_kxy[i] = ma.kxy[(long)scene * NEP_MISSION_MAX_VERT * 2 + i];
  for (int i = lane; i <= n_poly; i += 64) s_off[i] = g_off[i];
  const long base = (long)scene * N;
  const int origin = fa.origin[scene];                 // the scene's index in the flight it comes from: the generator's global slot and the log's `who`
  const long gbase = (long)origin * N;
  const double t_end = mission_t_end(fa.t_now[scene], fa.cfg.dc, T);
  const bool per_agent = c.mode == NEP_MISSION_PER_AGENT;
  const int n_script = ma.script ? ma.script_n[0] : 0;      // (one address for every lane: uniform; 0: the goals are drawn)
  // ---- the ticks and the triggers: lanes stride over the agents ----------------------------------------------------------------
  bool all_completed = true;
  for (int a0 = 0; a0 < N; a0 += 64) {
    const int a = a0 + lane;
    bool comp_ok = true;
    if (a < N) {
      const long slot = base + a;
      const int size = fa.size[slot], head = fa.head[slot];
      const double* st = fa.state + slot * 12;
      const double* ring = fa.ring + slot * cap * 12;
      const double* e = size < 1 ? st : ring + (long)((head + min(T - 1, size - 1)) % cap) * 12;      // p_T: the end state
      s_end[3 * a] = e[0]; s_end[3 * a + 1] = e[1]; s_end[3 * a + 2] = e[2];
      int todo = 0;
      double len = ma.length[slot];
      if (!(per_agent && mission_quota_used(c, ma.counts + slot * 4))) {
        const double goal[3] = {fa.goal[slot * 3], fa.goal[slot * 3 + 1], fa.goal[slot * 3 + 2]};
        int comp = ma.completed[slot];
        double prev[3] = {st[0], st[1], st[2]};
        for (int q = 1; q <= T; q++) {
          const double* g = size < 1 ? st : ring + (long)((head + min(q - 1, size - 1)) % cap) * 12;
          const double p[3] = {g[0], g[1], g[2]};
          mission_tick(c, prev, p, goal, len, comp);
          prev[0] = p[0]; prev[1] = p[1]; prev[2] = p[2];
        }
        ma.length[slot] = len; ma.completed[slot] = comp;
        comp_ok = comp != 0;
        if (per_agent) todo = mission_agent_trigger(c, e, goal, t_end - ma.t_issue[slot]);
      }
      s_got[a] = todo;
      s_new[3 * a] = len;
    }
    all_completed = all_completed && __ballot(!comp_ok) == 0ull;
  }
  __syncthreads();
  const double* pb = fa.pb;
  if (per_agent) {
    // ---- autoCMD: the agents whose leg ended, in agent order ------------------------------------------------------------------
    bool fin = true;
    for (int a0 = 0; a0 < N; a0 += 64) {
      const int mine = a0 + lane;
      unsigned long long m = __ballot(mine < N && s_got[mine] != 0);
      while (m) {
        const int a = a0 + __ffsll((long long)m) - 1; m &= m - 1ull;
        const long slot = base + a;
        const int outcome = s_got[a];
        const bool draws = mission_agent_draws(c, ma.counts + slot * 4);
        double gx = 0.0, gy = 0.0, gz = c.goal_z;
        int k = -1;
        if (draws && n_script > 0) k = mission_scripted(ma, slot, n_script, gx, gy, gz);
        else if (draws) k = mission_draw(c, lane, mission_h1(c.seed, (uint64_t)(gbase + a), (uint64_t)ma.counts[slot * 4 + kIssued]), a, N, s_end, pb, n_poly, s_off, s_kxy, s_new, s_got, gx, gy);
        __syncthreads();      // (every lane has read the slot's counts and the LDS lists before the owner changes them)
        if (lane == (a & 63)) {
          const bool none = mission_end_leg(c, mission_slot(ma, fa, slot), ma.log + slot * c.log_cap, ma.log_n + slot, (int)(gbase + a), outcome, t_end, draws, n_script > 0, k, gx, gy, gz);
          if (none) atomicOr(fa.gflags, NEP_FLAG_MISSION);
          s_got[a] = draws && k >= 0 ? kGotNew : kNoNew;
          if (draws && k >= 0) { s_new[3 * a] = gx; s_new[3 * a + 1] = gy; s_new[3 * a + 2] = gz; }
        }
        __syncthreads();
      }
      fin = fin && __ballot(mine < N && !mission_quota_used(c, ma.counts + (base + mine) * 4)) == 0ull;
    }
    if (fin && lane == 0) scene_i[kFinished] = 1;
    return;
  }
  // ---- benchmark_mtlp, auto_commands_together: the scene's run ------------------------------------------------------------------------------------------
  const double el = t_end - ma.t_run[scene];
  if (!mission_run_over(c, all_completed, el)) return;
  double sum = 0.0;
  if (lane == 0) for (int a = 0; a < N; a++) sum = sum + s_new[3 * a];      // (agent order: one lane)
  __syncthreads();
  const bool draws = mission_run_draws(c, scene_i);
  int attempts = 0;
  for (int a = 0; a < N; a++) {
    const long slot = base + a;
    double gx = 0.0, gy = 0.0, gz = c.goal_z;
    int k = -1;
    if (draws && n_script > 0) k = mission_scripted(ma, slot, n_script, gx, gy, gz);
    else if (draws) k = mission_draw(c, lane, mission_h1(c.seed, (uint64_t)(gbase + a), (uint64_t)ma.counts[slot * 4 + kIssued]), a, N, s_end, pb, n_poly, s_off, s_kxy, s_new, s_got, gx, gy);
    attempts += mission_attempts(c, draws, n_script > 0, k);
    __syncthreads();
    if (lane == (a & 63)) {
      const bool none = mission_end_run_slot(c, mission_slot(ma, fa, slot), el, t_end, draws, k, gx, gy, gz);
      if (none) atomicOr(fa.gflags, NEP_FLAG_MISSION);
      if (draws && k >= 0) { s_got[a] = kGotNew; s_new[3 * a] = gx; s_new[3 * a + 1] = gy; s_new[3 * a + 2] = gz; }
    }
    __syncthreads();
  }
  if (lane == 0) mission_end_run(c, scene_i, ma.t_run + scene, ma.log + (long)scene * c.log_cap, ma.log_n + scene, origin, all_completed, t_end, sum, N, attempts);
}

// the first leg of every slot: nep_batch_fleet_mission_init
__global__ void fleet_mission_seed_kernel(FleetMissionArgs ma, FleetArgs fa) {
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= (long)fa.n_scenes * fa.N) return;
  const long scene = slot / fa.N;
  ma.t_issue[slot] = fa.t_now[scene]; ma.length[slot] = 0.0; ma.completed[slot] = 0;
  ma.counts[slot * 4] = 1; ma.counts[slot * 4 + 1] = 0; ma.counts[slot * 4 + 2] = 0; ma.counts[slot * 4 + 3] = 0;
  ma.sums[slot * 2] = 0.0; ma.sums[slot * 2 + 1] = 0.0;
  if (slot % fa.N == 0) {
    ma.t_run[scene] = fa.t_now[scene];
    for (int i = 0; i < 4; i++) ma.scene_i[scene * 4 + i] = 0;
  }
}

}  // namespace

void launch_fleet_mission_seed(const FleetMissionArgs& ma, const FleetArgs& fa, hipStream_t st) {
  const long slots = (long)fa.n_scenes * fa.N;
  hipLaunchKernelGGL(fleet_mission_seed_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, ma, fa);
}
void launch_fleet_mission(const FleetMissionArgs& ma, const FleetArgs& fa, hipStream_t st) {
  hipLaunchKernelGGL(fleet_mission_kernel, dim3((unsigned)fa.n_scenes), dim3(64), ma.lds_bytes, st, ma, fa);
}

}  // namespace nep
