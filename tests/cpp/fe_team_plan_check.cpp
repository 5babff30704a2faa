// fe_team_plan_check.cpp — the launch plan of the best-first search on four waves per search (FrontendFacts::team, launch_plan.h) and the
// LDS layout of its kernel (astar_ent_team_layout, lds_layout.h): host code only, its own main; tests/test_fe_team_plan_cpu.py.
// stdin, one line per call: "key=value ..." — the facts of nep::FrontendFacts by name (fe_launch_plan_check.cpp's names).  stdout, per
// call: "T1 <fields>" — the plan with team = 1 —, "T4 <fields>" — with team = 4 —, each followed by " # " and the searches' launch as a
// kernel trace shows it (grid in work-items | workgroup).  The program itself checks, whatever the facts: the plan with team = 1 is the
// plan of facts that never heard of the field; team = 4 changes `team` and `team_lds_bytes` alone, and only for the best-first search
// with the check; a value other than 1 and 4 plans one wave.  Then the layout: sections inside the launch, aligned, disjoint, the
// one-wave carve at its own offsets, the byte count the plan launches with.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../neptune_amd/csrc/launch_plan.h"

using namespace nep;

static bool set_fact(FrontendFacts& f, const std::string& k, const char* v) {
  const int i = std::atoi(v); const bool b = i != 0;
#define F_INT(name) if (k == #name) { f.name = i; return true; }
#define F_BOOL(name) if (k == #name) { f.name = b; return true; }
  F_INT(num_agents) F_INT(n_static) F_INT(num_pol) F_INT(hull_mode) F_INT(slots) F_INT(n_scenes) F_BOOL(best_first) F_BOOL(ent)
  F_INT(beam_width) F_INT(num_samples) F_BOOL(have_recs) F_BOOL(active) F_BOOL(lpt) F_BOOL(order_key_ok) F_BOOL(fe_history) F_BOOL(big_beta)
  F_BOOL(fe_three) F_INT(fe_xcd)
#undef F_INT
#undef F_BOOL
  if (k == "ent_samples") return true;      // (not a fact of the plan)
  return false;
}

// every field of a plan but the two the team form may change
static std::string fields(const FrontendPlan& p) {
  char b[256];
  std::snprintf(b, sizeof b, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d", p.hulls, p.grouped_hulls, p.ent_sample, (int)p.order, p.active_list, p.boxes, p.ent_pack,
                (int)p.kernel, p.lds_bytes, p.big_redo, p.big_grid, p.big_lds_bytes, p.big_lds_off, p.have_history);
  return b;
}
static void print_plan(const char* tag, const FrontendPlan& p, long slots) {
  std::printf("%s %s team=%d team_lds=%d # %ldx1x1 | %dx1x1\n", tag, fields(p).c_str(), p.team, p.team_lds_bytes, slots * 64 * p.team, 64 * p.team);
}

struct Sec { const char* name; long off, bytes, align; };

static int check_layout() {
  const AstarEntLayout A = astar_ent_layout();
  const AstarEntTeamLayout T = astar_ent_team_layout();
  // the one-wave carve inside the team's, field for field
  if (T.one.work != A.work || T.one.ch != A.ch || T.one.hcost != A.hcost || T.one.lat != A.lat || T.one.heap != A.heap || T.one.ints != A.ints || T.one.path != A.path || T.one.bytes != A.bytes) {
    std::fprintf(stderr, "the one-wave carve moved\n"); return 4;
  }
  const std::vector<Sec> secs = {
      {"work", A.work, (long)(kAsNC + 1) * (long)sizeof(nep_fe_ent_state), 8}, {"ch", A.ch, (long)kAsNC * 17 * 8, 8}, {"hcost", A.hcost, (long)kAsNC * 8, 8},
      {"lat", A.lat, 4L * NEP_FE_MAX_SAMPLES * 8, 8}, {"heap", A.heap, (long)kAsHeapLds * 4, 4}, {"ints", A.ints, 10L * kAsNC * 4, 4}, {"path", A.path, (NEP_MAX_POL + 2) * 4L, 4},
      {"x_hdr", T.x_hdr, (long)kAsNC * kAsTeamSteps * 4, 4}, {"x_pool", T.x_pool, (long)kAsNC * kAsTeamSteps * kEntAddCap * 4, 4},
      {"x_stage", T.x_stage, (long)kAsTeamThreads * (kEntAddCap - 4) * 4, 4}, {"x_cn", T.x_cn, (long)kAsTeamThreads * 4, 4}, {"have", T.have, (long)kAsNC * 4, 4},
      {"ctl", T.ctl, (long)kAsTeamCtl * 4, 4}};
  for (size_t i = 0; i < secs.size(); i++) {
    const Sec& s = secs[i];
    if (s.off < 0 || s.off % s.align != 0 || s.off + s.bytes > T.bytes) { std::fprintf(stderr, "section %s: offset %ld, %ld bytes, launch %d\n", s.name, s.off, s.bytes, T.bytes); return 4; }
    for (size_t j = 0; j < i; j++)
      if (s.off < secs[j].off + secs[j].bytes && secs[j].off < s.off + s.bytes) { std::fprintf(stderr, "sections %s and %s overlap\n", secs[j].name, s.name); return 4; }
  }
  if (T.bytes % 16 != 0 || T.bytes > kLdsPerCu || T.x_hdr < A.bytes) { std::fprintf(stderr, "launch bytes %d\n", T.bytes); return 4; }
  // the header word: a list's offset in 16 bits, its length in 8; a work item's count and peak in 8 bits each; one round of items
  if ((long)kAsNC * kAsTeamSteps * kEntAddCap > 0xffff || kEntAddCap > 0xff || kAsNC * kAsTeamSteps > kAsTeamThreads || kAsTeamThreads != 64 * kAsTeamWaves) {
    std::fprintf(stderr, "header word or item count\n"); return 4;
  }
  std::printf("layout bytes=%d one=%d\n", T.bytes, A.bytes);
  return 0;
}

int main() {
  char line[4096];
  while (std::fgets(line, sizeof line, stdin)) {
    FrontendFacts f;
    bool any = false;
    for (char* tok = std::strtok(line, " \t\r\n"); tok; tok = std::strtok(nullptr, " \t\r\n")) {
      char* eq = std::strchr(tok, '=');
      if (!eq) { std::fprintf(stderr, "not key=value: %s\n", tok); return 2; }
      *eq = 0;
      if (!set_fact(f, tok, eq + 1)) { std::fprintf(stderr, "unknown fact: %s\n", tok); return 2; }
      any = true;
    }
    if (!any) continue;
    const FrontendPlan p0 = plan_frontend(f);      // facts that never heard of the field
    FrontendFacts f1 = f; f1.team = 1;
    FrontendFacts f4 = f; f4.team = 4;
    const FrontendPlan p1 = plan_frontend(f1), p4 = plan_frontend(f4);
    print_plan("T1", p1, f.slots);
    print_plan("T4", p4, f.slots);
    const bool team_call = p0.kernel == kFeBestFirstEnt;
    if (fields(p1) != fields(p0) || p1.team != 1 || p1.team_lds_bytes != 0 || p0.team != 1 || p0.team_lds_bytes != 0) { std::fprintf(stderr, "team = 1 is not the plan as it was\n"); return 3; }
    if (fields(p4) != fields(p0)) { std::fprintf(stderr, "team = 4 changed another field\n"); return 3; }
    if (p4.team != (team_call ? 4 : 1) || p4.team_lds_bytes != (team_call ? astar_ent_team_layout().bytes : 0)) { std::fprintf(stderr, "team = 4: waves or LDS\n"); return 3; }
    for (int other : {0, 2, 3, 5, 8, -4}) {
      FrontendFacts fo = f; fo.team = other;
      const FrontendPlan po = plan_frontend(fo);
      if (fields(po) != fields(p0) || po.team != 1 || po.team_lds_bytes != 0) { std::fprintf(stderr, "team = %d plans something\n", other); return 3; }
    }
  }
  if (int e = check_layout()) return e;
  std::printf("fe_team_plan_check ok\n");
  return 0;
}
