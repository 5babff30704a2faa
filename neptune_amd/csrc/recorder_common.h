// recorder_common.h — the layout of a fleet snapshot (include/neptune_fleet.h, section "recorder"), stated once: the host code
// (recorder_host.cpp: nep_fleet_snapshot_describe), the entry points (backend.hip) and the kernels (fleet_recorder_kernels.hip) all
// take the sections' sizes and offsets from here.  Plain C++, no HIP.
#ifndef NEP_RECORDER_COMMON_H_
#define NEP_RECORDER_COMMON_H_

#include <cstddef>
#include <cstdint>

#include "../../include/neptune_fleet.h"

namespace nep_recorder {

static_assert(sizeof(nep_fleet_snapshot_hdr) == NEP_SNAPSHOT_HDR_BYTES && NEP_SNAPSHOT_HDR_BYTES % 16 == 0, "the snapshot header is a fixed, 16-byte multiple");
static_assert(sizeof(nep_fleet_snapshot_stamp) == 16, "a ring stamp is one 16-byte store");
static_assert(NEP_SNAP_LOG_N + 1 == NEP_SNAPSHOT_N_SECTIONS, "one index per section");

inline int64_t pad16(int64_t b) { return (b + 15) / 16 * 16; }

// bytes of section `id` in one scene block: the scene's part of the handle's array, unpadded (0: the state has no such section)
inline int64_t section_bytes(const nep_fleet_snapshot_hdr& h, int id) {
  const int64_t N = h.N, cap = h.tether_cap;
  const bool ent = h.tether_form != 0, fixed = h.tether_form == 1, lists = h.tether_form == 2, mis = h.mission_mode != 0;
  const int64_t owners = h.mission_mode == NEP_MISSION_PER_AGENT ? N : 1;
  switch (id) {
    case NEP_SNAP_ORIGIN: case NEP_SNAP_ROUND: return 4;
    case NEP_SNAP_RING: return N * h.ring_cap * 12 * 8;
    case NEP_SNAP_HEAD: case NEP_SNAP_SIZE: case NEP_SNAP_K_END: case NEP_SNAP_FLOWN: case NEP_SNAP_DONE: case NEP_SNAP_OUTCOME: case NEP_SNAP_SFLAGS: return N * 4;
    case NEP_SNAP_STATE: return N * 12 * 8;
    case NEP_SNAP_GOAL: return N * 3 * 8;
    case NEP_SNAP_PWP: return N * (int64_t)sizeof(nep_pwp);
    case NEP_SNAP_PERIOD: case NEP_SNAP_PHASE: return h.timers ? N * 4 : 0;
    case NEP_SNAP_T_NOW: return 8;
    case NEP_SNAP_COUNTERS: return 4 * NEP_FLEET_N_COUNTERS;
    case NEP_SNAP_ENT: return fixed ? N * (int64_t)sizeof(nep_fe_ent_state) : 0;
    case NEP_SNAP_L_N_ALPHA: case NEP_SNAP_L_N_BEND: case NEP_SNAP_HELD: return lists ? N * 4 : 0;
    case NEP_SNAP_L_ID: return lists ? N * cap * 2 : 0;
    case NEP_SNAP_L_CS: return lists ? N * cap : 0;
    case NEP_SNAP_L_BETA: return lists ? N * cap * 8 : 0;
    case NEP_SNAP_L_BEND: return lists ? N * NEP_MAX_BEND * 2 : 0;
    case NEP_SNAP_PUB_N: case NEP_SNAP_PUB_PREV_N: case NEP_SNAP_ENT_FLAGS: case NEP_SNAP_ENT_EVER: case NEP_SNAP_ENT_WALKED: return ent ? N * 4 : 0;
    case NEP_SNAP_PUB_XY: case NEP_SNAP_PUB_PREV_XY: return ent ? N * NEP_MAX_BEND * 2 * 8 : 0;
    case NEP_SNAP_T_ISSUE: case NEP_SNAP_LENGTH: return mis ? N * 8 : 0;
    case NEP_SNAP_COMPLETED: return mis ? N * 4 : 0;
    case NEP_SNAP_COUNTS: case NEP_SNAP_SUMS: return mis ? N * 16 : 0;
    case NEP_SNAP_SCENE_I: return mis ? 16 : 0;
    case NEP_SNAP_T_RUN: return mis ? 8 : 0;
    case NEP_SNAP_LOG: return mis ? owners * h.log_cap * (int64_t)sizeof(nep_mission_leg) : 0;
    case NEP_SNAP_LOG_N: return mis ? owners * 4 : 0;
  }
  return 0;
}

// are the fields the sizes are made of in range (so that no product above overflows or goes negative)?
inline bool fields_ok(const nep_fleet_snapshot_hdr& h) {
  return h.n_scenes >= 1 && h.N >= 1 && h.N <= (1 << 20) && h.ring_cap >= 1 && h.ring_cap <= (1 << 20) && h.num_pol >= 1 && h.num_pol <= NEP_MAX_POL && h.max_states >= 1 &&
         h.tether_form >= 0 && h.tether_form <= 2 && (h.tether_form == 0 ? h.tether_cap == 0 : h.tether_form == 1 ? h.tether_cap == NEP_FE_ENT_CAP
                                                                                                  : h.tether_cap > NEP_FE_ENT_CAP && h.tether_cap <= NEP_ENT_LISTS_MAX_CAP) &&
         (h.mission_mode == 0 ? h.log_cap == 0 : (h.mission_mode >= NEP_MISSION_PER_AGENT && h.mission_mode <= NEP_MISSION_FLEET_TOGETHER) && h.log_cap >= 0 && h.log_cap <= (1 << 20)) &&
         (h.timers == 0 || h.timers == 1);
}

// the sections' offsets in a block and their unpadded sizes; returns the bytes of a block (a multiple of 16)
inline int64_t layout(const nep_fleet_snapshot_hdr& h, int64_t* offset, int64_t* bytes) {
  int64_t at = 0;
  for (int id = 0; id < NEP_SNAPSHOT_N_SECTIONS; id++) {
    const int64_t b = section_bytes(h, id);
    if (offset) offset[id] = at;
    if (bytes) bytes[id] = b;
    at += pad16(b);
  }
  return at;
}

// a ring of n_entries: header, stamp table [n_entries][n_scenes], blocks [n_entries][n_scenes]
inline int64_t ring_blocks_offset(const nep_fleet_snapshot_hdr& h, int64_t n_entries) { return NEP_SNAPSHOT_HDR_BYTES + n_entries * h.n_scenes * (int64_t)sizeof(nep_fleet_snapshot_stamp); }
inline int64_t ring_bytes(const nep_fleet_snapshot_hdr& h, int64_t n_entries) { return ring_blocks_offset(h, n_entries) + n_entries * h.n_scenes * h.scene_bytes; }

inline uint64_t fnv1a(uint64_t hash, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; i++) { hash ^= b[i]; hash *= 0x100000001b3ull; }
  return hash;
}
constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull;

// defined in recorder_host.cpp
uint64_t config_hash(const nep_fleet_cfg& cfg, double cable, const nep_mission_cfg& mis);
// 0, or NEP_E_ARG with the reason in *why: the header alone (magic, version, sizes, fields, scene_bytes against the layout)
int check_header(const nep_fleet_snapshot_hdr& h, const char** why);

}  // namespace nep_recorder
#endif  // NEP_RECORDER_COMMON_H_
