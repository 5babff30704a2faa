// recorder_check.cpp — drives the host side of the fleet recorder (neptune_amd/csrc/recorder_host.cpp: nep_fleet_snapshot_describe,
// the layout, the configuration hash) over good and broken headers.  Host code only, its own main: the CPU suite builds it with
// -fsanitize=address,undefined and runs it (tests/test_fleet_recorder_cpu.py).  Every blob is a heap buffer of exactly the bytes
// it claims, so a read past the header or past `bytes` is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "neptune_fleet.h"
#include "../../neptune_amd/csrc/recorder_common.h"

namespace nep { void set_last_error(const std::string&) {} }

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static nep_fleet_snapshot_hdr good(int n_scenes, int N, int ring_cap, int form, int cap, int mode, int log_cap, int timers) {
  nep_fleet_snapshot_hdr h{};
  h.magic = NEP_SNAPSHOT_MAGIC; h.version = NEP_SNAPSHOT_VERSION; h.hdr_bytes = NEP_SNAPSHOT_HDR_BYTES;
  h.n_scenes = n_scenes; h.N = N; h.num_pol = 8; h.ring_cap = ring_cap; h.max_states = 48;
  h.tether_form = form; h.tether_cap = cap; h.mission_mode = mode; h.log_cap = log_cap; h.timers = timers;
  h.scene_bytes = nep_recorder::layout(h, nullptr, nullptr);
  return h;
}

static int describe(const nep_fleet_snapshot_hdr& h, int64_t bytes, nep_fleet_snapshot_info* out) {
  std::vector<unsigned char> blob((size_t)(bytes > 0 ? bytes : 0));      // (the body's bytes are never read: zeros)
  if (blob.size() >= sizeof(h)) std::memcpy(blob.data(), &h, sizeof(h));
  else if (!blob.empty()) std::memcpy(blob.data(), &h, blob.size());
  return nep_fleet_snapshot_describe(blob.empty() ? (const void*)&h : blob.data(), bytes, out);
}

int main() {
  const nep_fleet_snapshot_hdr cases[] = {good(3, 6, 54, 0, 0, 0, 0, 0), good(2, 70, 54, 1, NEP_FE_ENT_CAP, NEP_MISSION_PER_AGENT, 2, 1),
                                          good(1, 7, 9, 2, 48, NEP_MISSION_FLEET_RUNS, 3, 0), good(128, 64, 54, 2, 4096, NEP_MISSION_PER_AGENT, 16, 1)};
  for (const nep_fleet_snapshot_hdr& h : cases) {
    const int64_t full = NEP_SNAPSHOT_HDR_BYTES + (int64_t)h.n_scenes * h.scene_bytes;
    nep_fleet_snapshot_info info;
    // truncated to the header and to less than the header; the full blob where it is small enough to allocate here
    EXPECT(describe(h, NEP_SNAPSHOT_HDR_BYTES, &info) == NEP_E_ARG);
    EXPECT(describe(h, NEP_SNAPSHOT_HDR_BYTES - 1, &info) == NEP_E_ARG);
    if (full < (1 << 26)) {
      EXPECT(describe(h, full - 1, &info) == NEP_E_ARG);      // truncated by one byte
      EXPECT(describe(h, full, &info) == 0);
      EXPECT(std::memcmp(&info.hdr, &h, sizeof(h)) == 0);
      int64_t at = 0;
      for (int i = 0; i < NEP_SNAPSHOT_N_SECTIONS; i++) {
        EXPECT(info.offset[i] == at && info.offset[i] % 16 == 0 && info.bytes[i] >= 0);
        at += (info.bytes[i] + 15) / 16 * 16;
      }
      EXPECT(at == h.scene_bytes && h.scene_bytes % 16 == 0);
      EXPECT(info.bytes[NEP_SNAP_RING] == (int64_t)h.N * h.ring_cap * 96 && info.bytes[NEP_SNAP_PWP] == (int64_t)h.N * (int64_t)sizeof(nep_pwp));
    }
    nep_fleet_snapshot_hdr b = h; b.magic ^= 1u;
    EXPECT(describe(b, full < (1 << 26) ? full : NEP_SNAPSHOT_HDR_BYTES, &info) == NEP_E_ARG);
    b = h; b.version = 2;
    EXPECT(describe(b, NEP_SNAPSHOT_HDR_BYTES, &info) == NEP_E_ARG);
    b = h; b.scene_bytes += 8;
    EXPECT(describe(b, NEP_SNAPSHOT_HDR_BYTES, &info) == NEP_E_ARG);
    b = h; b.scene_bytes -= 16;      // the last section would end past the block
    EXPECT(describe(b, NEP_SNAPSHOT_HDR_BYTES, &info) == NEP_E_ARG);
    b = h; b.N = -1;
    EXPECT(describe(b, NEP_SNAPSHOT_HDR_BYTES, &info) == NEP_E_ARG);
    b = h; b.scene_bytes = 0;
    EXPECT(describe(b, NEP_SNAPSHOT_HDR_BYTES, &info) == NEP_E_ARG);
  }
  EXPECT(nep_fleet_snapshot_describe(nullptr, 80, nullptr) == NEP_E_ARG);
  // the hash: FNV-1a's known answers, and every input counts
  EXPECT(nep_recorder::fnv1a(nep_recorder::kFnvBasis, "", 0) == 0xcbf29ce484222325ull);
  EXPECT(nep_recorder::fnv1a(nep_recorder::kFnvBasis, "a", 1) == 0xaf63dc4c8601ec8cull);
  EXPECT(nep_recorder::fnv1a(nep_recorder::kFnvBasis, "foobar", 6) == 0x85944171f73967e8ull);
  nep_fleet_cfg fc{}; fc.dc = 0.01; nep_mission_cfg mc{};
  const uint64_t h0 = nep_recorder::config_hash(fc, 0.0, mc);
  nep_fleet_cfg f2 = fc; f2.dc = 0.02; nep_mission_cfg m2 = mc; m2.seed = 1;
  EXPECT(h0 != nep_recorder::config_hash(f2, 0.0, mc) && h0 != nep_recorder::config_hash(fc, 1.0, mc) && h0 != nep_recorder::config_hash(fc, 0.0, m2));
  EXPECT(h0 == nep_recorder::config_hash(fc, 0.0, mc));
  if (fails) return 1;
  std::printf("recorder_check ok\n");
  return 0;
}
