// fe_launch_plan_check.cpp — drives plan_frontend of neptune_amd/csrc/launch_plan.h (host code only, its own main;
// tests/test_fe_launch_plan_cpu.py).  stdin, one line per call: "new" starts a handle (no history of search times); "key=value ..." is one
// front-end call of it — the facts of nep::FrontendFacts by name, on top of the defaults below, and ent_samples (the samples per interval
// ent_sample_kernel's grid depends on).  fe_history is carried to the handle's next call as the plan says.  stdout, one line per call: the
// launches the plan implies, in order, as a kernel trace shows them — "name | grid | workgroup | static LDS", grids in work-items, joined
// by " ; " — then " # " and the plan's dynamic LDS bytes: lds, big_lds, big_off, and have_history.
// The grids are the launchers' (launch_hulls_ts, launch_ent_sample, launch_order_xcd, launch_qp_order, launch_active_list, launch_boxes,
// launch_frontend); the static LDS is what each kernel declares for itself, a property of the kernel, not of the plan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../neptune_amd/csrc/launch_plan.h"

using namespace nep;

static bool set_fact(FrontendFacts& f, int& ent_samples, const std::string& k, const char* v) {
  const int i = std::atoi(v); const bool b = i != 0;
#define F_INT(name) if (k == #name) { f.name = i; return true; }
#define F_BOOL(name) if (k == #name) { f.name = b; return true; }
  F_INT(num_agents) F_INT(n_static) F_INT(num_pol) F_INT(hull_mode) F_INT(slots) F_INT(n_scenes) F_BOOL(best_first) F_BOOL(ent)
  F_INT(beam_width) F_INT(num_samples) F_BOOL(have_recs) F_BOOL(active) F_BOOL(lpt) F_BOOL(order_key_ok) F_BOOL(fe_history) F_BOOL(big_beta)
  F_BOOL(fe_three) F_INT(fe_xcd)
#undef F_INT
#undef F_BOOL
  if (k == "ent_samples") { ent_samples = i; return true; }
  return false;
}

static std::string out;
static void launch(const char* name, long items, int wg, int static_lds) {
  char b[256];
  std::snprintf(b, sizeof b, "%s%s | %ldx1x1 | %dx1x1 | %d", out.empty() ? "" : " ; ", name, items, wg, static_lds);
  out += b;
}
static long blocks(long n, long per) { return (n + per - 1) / per; }

int main() {
  char line[4096];
  bool fe_history = false;
  while (std::fgets(line, sizeof line, stdin)) {
    if (std::strncmp(line, "new", 3) == 0) { fe_history = false; continue; }
    FrontendFacts f; int ent_samples = 3;
    f.fe_history = fe_history;
    bool any = false;
    for (char* tok = std::strtok(line, " \t\r\n"); tok; tok = std::strtok(nullptr, " \t\r\n")) {
      char* eq = std::strchr(tok, '=');
      if (!eq) { std::fprintf(stderr, "not key=value: %s\n", tok); return 2; }
      *eq = 0;
      if (!set_fact(f, ent_samples, tok, eq + 1)) { std::fprintf(stderr, "unknown fact: %s\n", tok); return 2; }
      any = true;
    }
    if (!any) continue;
    const FrontendPlan p = plan_frontend(f);
    fe_history = p.have_history;
    const long recs = (long)f.n_scenes * f.num_agents, slots = f.slots;
    out.clear();
    if (p.hulls && p.grouped_hulls) launch("nep::hull_group_kernel", recs * 64, 64, 10240);
    if (p.hulls && !p.grouped_hulls) launch("nep::hull_kernel", recs * f.num_pol * 64, 64, 3584);
    if (p.ent_sample) { const long b = blocks(recs * f.num_pol * (ent_samples + 1), 256); launch("nep::ent_sample_kernel", (b > 8192 ? 8192 : b) * 256, 256, 0); }
    if (p.order == kFeOrderXcd || p.order == kFeOrderXcdKeyed) launch("nep::order_xcd_kernel", 1024, 1024, 2048);
    if (p.order == kFeOrderKeyed) launch("nep::order_kernel", 1024, 1024, 4608);
    if (p.active_list) { launch("nep::active_list_kernel", 1024, 1024, 512); launch("nep::skipped_fe_kernel", blocks(slots, 64) * 64, 64, 0); }
    if (p.boxes) launch("nep::fe_box_kernel", blocks((long)f.n_scenes * (f.num_agents + f.n_static) * f.num_pol, 256) * 256, 256, 0);
    if (p.ent_pack) launch("nep::ent_pack_kernel", blocks(recs * f.num_pol, 256) * 256, 256, 0);
    if (slots > 0) switch (p.kernel) {
      case kFeBeamFour: launch("void nep::frontend_kernel<false, 4, false>", slots * 256, 256, 0); break;
      case kFeBeamThree: launch("void nep::frontend_kernel<false, 3, false>", slots * 256, 256, 0); break;
      case kFeBeamEnt: launch("void nep::frontend_kernel<true, 3, false>", slots * 256, 256, 0); break;
      case kFeBestFirst: launch("void nep::frontend_astar_kernel<false>", slots * 64, 64, 13312); break;
      case kFeBestFirstEnt: launch("void nep::frontend_astar_kernel<true>", slots * 64, 64, 0); break;
    }
    if (p.big_redo) launch("void nep::frontend_kernel<true, 1, true>", (long)p.big_grid * 256, 256, 0);
    std::printf("%s # %d %d %d %d\n", out.c_str(), p.lds_bytes, p.big_lds_bytes, p.big_lds_off, p.have_history ? 1 : 0);
    // what a plan must never say, whatever the facts
    const bool xcd = p.order == kFeOrderXcd || p.order == kFeOrderXcdKeyed, beam = p.kernel == kFeBeamFour || p.kernel == kFeBeamThree || p.kernel == kFeBeamEnt;
    if ((p.order != kFeOrderNone && (f.slots <= 1024 || !beam || !f.lpt)) || (xcd && f.slots % 8 != 0) || (p.order == kFeOrderKeyed && !f.fe_history)
        || ((p.order == kFeOrderXcdKeyed || p.order == kFeOrderKeyed) && !f.order_key_ok) || (p.boxes && !beam) || (p.big_redo && p.kernel != kFeBeamEnt)
        || (p.kernel == kFeBeamEnt && !p.big_redo && f.slots > 0) || (p.ent_pack != (f.ent && f.slots > 0)) || (p.ent_sample && !(f.have_recs && f.ent)) || (p.grouped_hulls && !p.hulls)
        || (p.kernel == kFeBeamFour && (p.lds_bytes > 40 * 1024 || f.fe_three)) || (p.big_redo && (p.big_grid < 1 || p.big_grid > kFeRedoCap || p.big_grid > f.slots))
        || (p.big_lds_off != 0 && (!f.big_beta || p.big_lds_bytes > kLdsPerCu)) || (beam && !p.have_history) || (!beam && p.have_history != f.fe_history)) {
      std::fprintf(stderr, "inconsistent plan\n"); return 3;
    }
  }
  std::printf("fe_launch_plan_check ok\n");
  return 0;
}
