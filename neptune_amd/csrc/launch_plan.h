// launch_plan.h — the launch topology of one replan (Engine::run, backend.hip) and of one front-end call (frontend_call), decided once:
// the caller copies the facts out of its handle and its call (ReplanFacts, FrontendFacts), plan_replan / plan_frontend say what will be
// launched (ReplanPlan, FrontendPlan), the launch code follows the plan and the debug calls read it back (path_bits).  Every rule of the
// sequences is stated here and nowhere else.  Plain C++, no HIP: tests/cpp/launch_plan_check.cpp and fe_launch_plan_check.cpp run the rules
// without a GPU.  plan_replan allocates nothing and loops over nothing (the per-agent handle calls it on every optimize()).
#ifndef NEP_LAUNCH_PLAN_H_
#define NEP_LAUNCH_PLAN_H_

#include "../../include/neptune_backend.h"
#include "../../include/neptune_backend_debug.h"
#include "lds_layout.h"

namespace nep {

struct ReplanFacts {
  // the scene parameters
  int num_agents = 0, num_pol = 0, n_hull = 0, n_static = 0, ent_enabled = 0, hull_mode = 0, skip_own = 0, sep_rule = 0;
  double cull_radius = 0.0;
  // the handle's switches and state
  bool use_reg = false, lpt = true, have_history = false, presolve_kernel = true, presolve_fused = true, skip_lps = true, no_redo = false;
  bool statics_boxy = true, static_boxes_ok = false;
  int sep_pack = 0;                                  // 0 by launch size, -1 the unpacked kernel, 1..NEP_MAX_POL forced
  bool polish = true, polish_presolve = true, polish_buffers = false;      // (nep_*_set_polish; the pass's buffers exist)
  bool order_ok = false, order_key_ok = false, presolved_ok = false;       // d_order, d_order_key, d_presolved hold one entry per slot
  int scratch_chunks = 0;                            // > 0: the row scratch is the redo pass's pool of that many areas
  // the call
  int slots = 0, n_scenes = 0, n_rec = 0, phases = 3, hull_pb = 0;
  bool have_recs = false, lines_override = false, active = false;
};

enum Certificate { kCertNone = 0, kCertKernel = 1, kCertWave = 2 };      // the zero-iteration certificate: not ahead of the QP launch, qp_presolve_kernel, the separator's wave
enum QpKernel { kQpLds = 0, kQpReg = 1, kQpRegCull = 2, kQpRegCullPolish = 3 };      // qp_kernel, qp_reg_kernel<false>, <true, false>, <true, true>

struct ReplanPlan {
  bool geo = false, qp = false;                      // the halves of this call (phases & 1, phases & 2)
  bool hulls = false, grouped_hulls = false;         // the hull launch, and whether it is the eight-hulls-per-wave kernel
  bool fused_boxes = false, fused_order = false, box_kernel = false;
  bool skip = false;                                 // LPs whose box is far are skipped (and verified after the solve)
  bool separator = false; int sep_pack = 0;          // the separator launch; its segments per wave, 0: the unpacked kernel
  Certificate certificate = kCertNone;
  bool keyed = false;                                // the QP workgroups write their measured time into the ordering keys
  bool order_kernel = false, ordered_qp = false, polish_zero = false, active_list = false;
  QpKernel qp_kernel = kQpLds;
  bool redo_pass = false;                            // ... over the redo list, every row: qp_reg_kernel<false>
  bool polish_armed = false, polish_pass = false;    // the QP kernels list solves for the polish pass; the pass is launched
  bool grow_scratch = false;                         // the row scratch must first grow to one area per slot
  bool have_history = false;                         // what the call leaves behind for the next one
};

// --- the rules ---------------------------------------------------------------------------------------------------------------------

// "More than one wave of workgroups": below that a launch order changes nothing, every workgroup starts at once.
inline bool more_than_one_wave(long slots) { return slots > 1024; }

// Eight hulls per wave when there are enough trajectories to fill the chip with such waves (a wave of eight takes ~60 us,
// one hull per wave ~26 us: below ~2 000 trajectories the launch is one round of waves either way and the short waves
// finish first — 0.026 against 0.058 ms for one 64-agent scene; 0.077 both at 32 scenes; 0.271 against 0.183 ms at 128).
// nep_batch_set_hull_kernel forces one (tests, A/B).
inline bool eight_hulls_per_wave(int num_pol, int hull_mode, int n_scenes, int n_rec) {
  return num_pol <= 8 && (hull_mode ? hull_mode == 2 : (long)n_scenes * n_rec > 2048);
}

// LPs whose line is known to be far without solving them may be skipped when the presolve is on, the rule is the largest gap
// (box far => line far holds for that vertex only), the hull lists are the batch's (one per agent: the boxes are indexed
// by agent) and the interior point is the register kernel (the one that verifies them): see separator_body / qp_reg_kernel
inline bool can_skip_lps(const ReplanFacts& f) {
  return f.cull_radius > 0.0 && f.use_reg && f.sep_rule == 0 && f.skip_own == 1 && f.n_hull == f.num_agents && f.skip_lps && f.statics_boxy;
}
inline bool skip_mode(const ReplanFacts& f) { return can_skip_lps(f) && !f.no_redo; }      // ... and the replans that fail the verification go through the redo pass

// the polish pass finishes what the register kernel leaves.  Under the presolve only on request (nep_batch_set_polish(h, 2): on the
// near lines, and a certified point goes through the presolve's verification of the parked lines and the skipped LPs again —
// polish_slot): a pass over a handful of slots is 0.03-0.06 ms, 8 % of a presolved step
inline bool polish_armed(const ReplanFacts& f) {
  return f.polish && f.use_reg && (f.polish_presolve || !(f.cull_radius > 0.0)) && f.polish_buffers;
}

// segments per wave of the packed separator for this launch, 0 when the launch takes the unpacked kernel (skip: the plan's)
inline int segments_per_wave(const ReplanFacts& f, bool skip) {
  // (only with the spatial presolve: with every LP to solve a segment fills its wave by itself — 64 to 68 LPs — and the packed form is
  // slower, 0.53 against 0.41 ms per 4.2 M LPs: its step 1 is serial over the segments and its lanes hold different control points)
  const int total = f.n_hull + f.num_agents + f.n_static + (f.ent_enabled ? f.num_agents * NEP_MAX_BEND : 0);
  // the packed kernel's list entries are (segment << 13 | candidate) in 16 bits: candidates beyond 8 191 (about 800 agents with the
  // entangle rows, 4 000 without) take the unpacked kernel, whose entries hold 65 535 (size_scratch refuses more)
  if (!(((skip && f.cull_radius > 0.0 && f.sep_pack >= 0) || (f.cull_radius == 0.0 && f.sep_pack >= 1)) && f.sep_rule == 0 && total <= 8191)) return 0;
  int pack = 1; while (pack < NEP_MAX_POL && (long)f.slots * (NEP_MAX_POL / (pack * 2)) >= 4096) pack *= 2;      // (at least ~4 000 waves while the launch allows it)
  if (f.sep_pack >= 1 && f.sep_pack <= NEP_MAX_POL) pack = f.sep_pack;
  return pack;
}

inline ReplanPlan plan_replan(const ReplanFacts& f) {
  ReplanPlan p;
  const bool cull = f.cull_radius > 0.0;
  p.geo = (f.phases & 1) != 0; p.qp = (f.phases & 2) != 0;
  p.hulls = f.have_recs && p.geo;
  p.grouped_hulls = p.hulls && eight_hulls_per_wave(f.num_pol, f.hull_mode, f.n_scenes, f.n_rec);
  // the hull kernel makes the hulls' boxes itself (and zeroes the redo counters) when it is the eight-hulls-per-wave kernel over one hull list
  // per agent and the static polygons' boxes are in place (written at upload: push_static_boxes): one launch less per round
  p.fused_boxes = p.grouped_hulls && can_skip_lps(f) && !f.lines_override && f.static_boxes_ok && f.hull_pb <= 0
                  && f.n_rec == f.num_agents && f.n_hull == f.num_agents;
  // ... and, in one wave more, this round's launch order of the QP workgroups (order_kernel's counting sort: it only needs the previous
  // round's measured times), when the same call goes on to the QP half
  p.keyed = p.qp && f.lpt && f.order_key_ok;
  p.ordered_qp = p.keyed && f.have_history && more_than_one_wave(f.slots) && f.order_ok;
  p.fused_order = p.fused_boxes && p.ordered_qp;
  p.order_kernel = p.ordered_qp && !p.fused_order;      // (zeroes the polish pass's counters on its way; fused_order: the hull launch has done both)
  p.skip = can_skip_lps(f) && !f.lines_override;        // (lines from the host: no LP ran, none was skipped)
  // (a pooled handle asked for a replan without the redo pass — lines from the host, a rule or hull layout that cannot skip LPs: one area per slot after all)
  p.grow_scratch = f.scratch_chunks > 0 && !skip_mode(f);
  p.separator = p.geo && !f.lines_override;
  p.box_kernel = p.separator && p.skip && !p.fused_boxes;      // (zeroes the redo counters as well)
  p.sep_pack = segments_per_wave(f, p.skip);
  // the presolve's zero-iteration certificate ahead of the interior-point launch: the replans it finishes (nine in ten of the bench's
  // scenes) cost that launch an immediate return.  In the separator's own wave when that wave holds every segment of its slot (the
  // packed kernel at eight segments a wave: launches of some 4 096 slots and more) — everything the certificate reads is in that
  // wave's hands (qp_presolve.h) —, as a kernel of its own otherwise (qp_presolve_kernel.hip).  The fused form keeps to the cases it
  // is tested in: one call for both halves, no active set, and the launch order either made by the hull launch or not made at all
  // (a certified slot's key decays when it is certified: an order kernel between the separator and the QP launch would read the
  // decayed keys, where it reads the previous round's with the kernel of its own).  (The wave of an inactive slot returns at its
  // first line and would leave a stale mark.)
  const bool pre = p.qp && f.use_reg && f.presolve_kernel && cull && !f.lines_override && f.presolved_ok;
  const bool wave = pre && f.presolve_fused && f.phases == 3 && !f.active && p.skip && !p.order_kernel && p.sep_pack == NEP_MAX_POL;
  p.certificate = !pre ? kCertNone : wave ? kCertWave : kCertKernel;
  p.polish_armed = polish_armed(f);
  p.polish_zero = p.qp && !p.ordered_qp && p.polish_armed && !(f.use_reg && f.slots == 1);      // (a one-workgroup launch — the per-agent handle — sets the counters itself: qp_reg_kernel's last lines)
  p.active_list = p.qp && f.active;      // an active set: the QP launches run over the list of active slots (in the launch order made above), the inactive slots' outputs are written apart
  // the register kernel's instantiation: <CULL> with parked lines to verify (never with lines from the host), <.., POLISH> when it lists for the polish pass
  p.qp_kernel = !f.use_reg ? kQpLds : !(cull && !f.lines_override) ? kQpReg : p.polish_armed ? kQpRegCullPolish : kQpRegCull;
  // the presolve's redo pass: replans whose solution did not verify the skipped / parked lines (listed by the kernel above; the
  // list is empty nearly always) get every LP solved and every row through the interior point — qp_reg_kernel<false>, whatever the
  // certificate marked.  (no_redo: development aid — the flagged replans keep their presolved result for inspection)
  p.redo_pass = p.qp && p.skip && !f.no_redo;
  p.polish_pass = p.qp && p.polish_armed;      // (the slots the QP kernel listed: nearly always none — workgroups beyond the count return at once)
  p.have_history = p.qp ? p.keyed : f.have_history;
  return p;
}

// --- the front end (frontend_call, backend.hip -> launch_frontend, geom_kernels.hip) ------------------------------------------------
// The same for the six nep_batch_frontend* entry points: one call's facts, what it launches, in launch order.  fe_layout (lds_layout.h)
// is the only loop behind plan_frontend, as it was behind the launchers.

struct FrontendFacts {
  // the scene parameters
  int num_agents = 0, n_static = 0, num_pol = 0, hull_mode = 0;
  // the call: its searches and their kind, where its hulls come from (records: the call makes them; else gathered blocks), an active set
  // in force (nep_batch_set_active, which also sized the list's buffer)
  int slots = 0, n_scenes = 0;
  bool best_first = false, ent = false;
  int beam_width = 0, num_samples = 0;
  bool have_recs = false, active = false;
  // the handle's switches and state: nep_batch_set_launch_order (with the order's buffer in place), the keys' buffer holds one entry per
  // slot (Engine::fill's condition for ps.fe_order_key), a beam call has left its searches' times in the keys, the big-record
  // instantiation's betas have their global memory (the entangle-aware beam's scratch: sized at the call, or the call fails)
  bool lpt = true, order_key_ok = false, fe_history = false, big_beta = false;
  // process-wide A/B switches (nep_debug_set_global_option): keep the three-workgroup instantiation; 0 = no XCD placement
  bool fe_three = false; int fe_xcd = 1;
  // nep_batch_set_fe_astar_team: waves per search of the best-first search with the entangle check, 1 or 4 (read for that search alone)
  int team = 1;
};

enum FeOrder { kFeOrderNone = 0, kFeOrderXcd = 1, kFeOrderXcdKeyed = 2, kFeOrderKeyed = 3 };      // slot order; order_xcd_kernel without and with keys; order_kernel
// frontend_kernel<true, NEP_FE_ENT_WGS>, <false, 4>, <false, NEP_FE_WAVES>; frontend_astar_kernel<false>, <true> (kFeBestFirstEnt with
// FrontendPlan::team == 4: frontend_astar_team_kernel, the same search on four waves)
enum FeKernel { kFeBeamEnt = 0, kFeBeamFour = 1, kFeBeamThree = 2, kFeBestFirst = 3, kFeBestFirstEnt = 4 };
constexpr int kFeRedoCap = 256;      // searches one call can hand to the big-record instantiation (beyond it they stay flagged)

struct FrontendPlan {
  bool hulls = false, grouped_hulls = false;         // the hull launch, and whether it is the eight-hulls-per-wave kernel
  bool ent_sample = false;                           // ent_sample_kernel: the committed trajectories' samples and presence flags
  FeOrder order = kFeOrderNone;
  bool active_list = false;                          // active_list_kernel, and skipped_fe_kernel for the outputs of the inactive slots
  bool boxes = false, ent_pack = false;              // fe_box_kernel, ent_pack_kernel
  FeKernel kernel = kFeBeamFour; int lds_bytes = 0;  // the searches, one workgroup per slot, and their dynamic LDS
  int team = 1, team_lds_bytes = 0;                  // waves per search (the workgroup is 64 * team threads: kFeBestFirstEnt alone has a form with four); that form's LDS, 0 with team == 1
  bool big_redo = false; int big_grid = 0, big_lds_bytes = 0, big_lds_off = 0;      // frontend_kernel<true, 1, true> over the searches the launch above listed
  bool have_history = false;                         // what the call leaves behind for the next one
};

inline FrontendPlan plan_frontend(const FrontendFacts& f) {
  FrontendPlan p;
  const bool any = f.slots > 0, beam = !f.best_first;      // (no slot: the launchers launch nothing)
  p.hulls = f.have_recs;
  p.grouped_hulls = p.hulls && eight_hulls_per_wave(f.num_pol, f.hull_mode, f.n_scenes, f.num_agents);
  p.ent_sample = f.ent && f.have_recs;      // (gathered blocks carry the samples: nep_batch_hulls made them)
  // The launch order of the beam's workgroups (the best-first searches run in slot order).  A few whole scenes per XCD, the longest
  // expected searches first within each (order_xcd_kernel; it deals the slots out in eights: slots % 8 == 0), with the keys when the
  // previous beam call left them, the placement alone when not; launches it cannot take get the keyed order (order_kernel), which
  // needs the keys.  Neither below two waves of workgroups.
  const bool orderable = any && beam && f.lpt && more_than_one_wave(f.slots), keys = f.order_key_ok && f.fe_history;
  p.order = !orderable ? kFeOrderNone : (f.slots % 8 == 0 && f.fe_xcd) ? (keys ? kFeOrderXcdKeyed : kFeOrderXcd) : keys ? kFeOrderKeyed : kFeOrderNone;
  // an active set: the searches run over the list of active slots, in the launch order made above; the others get skipped_fe_kernel's outputs
  p.active_list = any && f.active;
  p.boxes = any && beam;      // (the beam's obstacle shortlist reads them; the best-first search tests every obstacle as the reference does)
  // one record per (scene, agent, interval) of what the entangle check reads.  A constant of the entangle-aware calls: every one of them
  // sizes the records' buffer before it launches (ent_packed, backend.hip)
  p.ent_pack = any && f.ent;
  p.lds_bytes = f.best_first ? (f.ent ? astar_ent_layout().bytes : 0) : fe_layout(f.num_agents, f.n_static, f.beam_width, f.num_samples, f.num_pol, f.ent).bytes;
  // a beam whose LDS leaves room for four workgroups on a CU (160 KB / 4) runs the instantiation bounded to 128 registers (11 spilled);
  // larger ones — more obstacles, a wider beam — the one bounded for three
  const bool four = p.lds_bytes <= 40 * 1024 && !f.fe_three;
  p.kernel = f.best_first ? (f.ent ? kFeBestFirstEnt : kFeBestFirst) : f.ent ? kFeBeamEnt : four ? kFeBeamFour : kFeBeamThree;
  // four waves per search: the handle's choice, for the best-first search with the check only (every other call keeps its form whatever the setting)
  p.team = p.kernel == kFeBestFirstEnt && f.team == kAsTeamWaves ? kAsTeamWaves : 1;
  p.team_lds_bytes = p.team == kAsTeamWaves ? astar_ent_team_layout().bytes : 0;
  // the searches in which a child outgrew the fixed record, again, with big records (nearly always none: the workgroups return at once).
  // A constant of the entangle-aware beam: its scratch (fe_ent_scratch) always holds the list, the pool and kFeRedoCap > 0.  Its lists
  // live in LDS when they have their betas' memory and the launch holds them (fe_layout's big)
  p.big_redo = any && beam && f.ent;
  if (p.big_redo) {
    const FeLayout lb = fe_layout(f.num_agents, f.n_static, f.beam_width, f.num_samples, f.num_pol, true, f.big_beta);
    p.big_grid = kFeRedoCap < f.slots ? kFeRedoCap : f.slots; p.big_lds_bytes = lb.bytes; p.big_lds_off = lb.big_lds_off;
  }
  p.have_history = beam ? true : f.fe_history;      // (a beam call's searches write the keys; a best-first call leaves the handle's state alone)
  return p;
}

// The record a call leaves of itself (the handle's last_plan): a QP half (phases == 2) keeps its geometry half's fields.
inline ReplanPlan record_of(ReplanPlan p, const ReplanPlan& before) {
  if (!p.geo) { p.box_kernel = before.box_kernel; p.grouped_hulls = before.grouped_hulls; p.fused_boxes = before.fused_boxes; p.fused_order = before.fused_order; }
  return p;
}

// NEP_PATH_* of a record
inline int path_bits(const ReplanPlan& p) {
  int b = 0;
  if (p.grouped_hulls) b |= NEP_PATH_HULLS_GROUPED;
  if (p.fused_boxes) b |= NEP_PATH_FUSED_BOXES;
  if (p.fused_order) b |= NEP_PATH_FUSED_ORDER;
  if (p.box_kernel) b |= NEP_PATH_BOX_KERNEL;
  if (p.certificate != kCertNone) b |= NEP_PATH_PRESOLVE_KERNEL;
  if (p.certificate == kCertWave) b |= NEP_PATH_FUSED_PRESOLVE;
  if (p.ordered_qp) b |= NEP_PATH_ORDERED_QP;
  if (p.redo_pass) b |= NEP_PATH_REDO_PASS;
  return b;
}

}  // namespace nep
#endif
