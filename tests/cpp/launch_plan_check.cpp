// launch_plan_check.cpp — drives neptune_amd/csrc/launch_plan.h (host code only, its own main; tests/test_launch_plan_cpu.py).
// stdin, one line per call: "new" starts a handle (no history, no record of a last replan); "key=value ..." is one replan of it — the facts
// of nep::ReplanFacts by name, on top of the defaults below.  What a call leaves behind is carried to the handle's next call as the plan
// says: have_history, the record of the last replan, and a row-scratch pool that the call has grown.  stdout, one line per call:
//   bits launch_order_none polish_armed qp_kernel_name sep_pack certificate have_history
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../neptune_amd/csrc/launch_plan.h"

using namespace nep;

static bool set_fact(ReplanFacts& f, const std::string& k, const char* v) {
  const int i = std::atoi(v); const bool b = i != 0;
#define F_INT(name) if (k == #name) { f.name = i; return true; }
#define F_BOOL(name) if (k == #name) { f.name = b; return true; }
  F_INT(num_agents) F_INT(num_pol) F_INT(n_hull) F_INT(n_static) F_INT(ent_enabled) F_INT(hull_mode) F_INT(skip_own) F_INT(sep_rule)
  if (k == "cull_radius") { f.cull_radius = std::atof(v); return true; }
  F_BOOL(use_reg) F_BOOL(lpt) F_BOOL(have_history) F_BOOL(presolve_kernel) F_BOOL(presolve_fused) F_BOOL(skip_lps) F_BOOL(no_redo)
  F_BOOL(statics_boxy) F_BOOL(static_boxes_ok) F_INT(sep_pack) F_BOOL(polish) F_BOOL(polish_presolve) F_BOOL(polish_buffers)
  F_BOOL(order_ok) F_BOOL(order_key_ok) F_BOOL(presolved_ok) F_INT(scratch_chunks)
  F_INT(slots) F_INT(n_scenes) F_INT(n_rec) F_INT(phases) F_INT(hull_pb) F_BOOL(have_recs) F_BOOL(lines_override) F_BOOL(active)
#undef F_INT
#undef F_BOOL
  return false;
}

int main() {
  char line[4096];
  bool have_history = false, grown = false; ReplanPlan last;
  while (std::fgets(line, sizeof line, stdin)) {
    if (std::strncmp(line, "new", 3) == 0) { have_history = false; grown = false; last = ReplanPlan(); continue; }
    ReplanFacts f;
    f.have_history = have_history;
    bool any = false;
    for (char* tok = std::strtok(line, " \t\r\n"); tok; tok = std::strtok(nullptr, " \t\r\n")) {
      char* eq = std::strchr(tok, '=');
      if (!eq) { std::fprintf(stderr, "not key=value: %s\n", tok); return 2; }
      *eq = 0;
      if (!set_fact(f, tok, eq + 1)) { std::fprintf(stderr, "unknown fact: %s\n", tok); return 2; }
      any = true;
    }
    if (!any) continue;
    if (grown) f.scratch_chunks = 0;
    const ReplanPlan p = plan_replan(f);
    last = record_of(p, last);
    have_history = p.have_history; grown = grown || p.grow_scratch;
    std::printf("%d %d %d %s %d %d %d\n", path_bits(last), last.ordered_qp ? 0 : 1, last.polish_armed ? 1 : 0,
                f.use_reg ? "qp_reg_kernel" : "qp_kernel", p.sep_pack, (int)p.certificate, p.have_history ? 1 : 0);
    // what a plan must never say, whatever the facts
    if ((p.fused_order && !p.fused_boxes) || (p.fused_boxes && p.box_kernel) || (p.order_kernel && p.fused_order) || (p.polish_zero && p.ordered_qp)
        || (p.certificate == kCertWave && (p.sep_pack != NEP_MAX_POL || p.order_kernel || f.active)) || ((p.qp_kernel == kQpLds) != !f.use_reg)) {
      std::fprintf(stderr, "inconsistent plan\n"); return 3;
    }
  }
  std::printf("launch_plan_check ok\n");
  return 0;
}
