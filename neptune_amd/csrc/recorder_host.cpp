// recorder_host.cpp — the host side of the fleet recorder that needs no device (include/neptune_fleet.h, section "recorder"): the
// header check, the layout of a scene block (recorder_common.h) behind nep_fleet_snapshot_describe, and the configuration hash.
// No HIP call; built like mission_host.cpp.
#include <cstring>
#include <string>

#include "recorder_common.h"

namespace nep { void set_last_error(const std::string& msg); }

namespace nep_recorder {

uint64_t config_hash(const nep_fleet_cfg& cfg, double cable, const nep_mission_cfg& mis) {
  uint64_t h = fnv1a(kFnvBasis, &cfg, sizeof(cfg));
  h = fnv1a(h, &cable, sizeof(cable));
  return fnv1a(h, &mis, sizeof(mis));
}

int check_header(const nep_fleet_snapshot_hdr& h, const char** why) {
  const char* w = nullptr;
  if (h.magic != NEP_SNAPSHOT_MAGIC) w = "not a fleet snapshot (magic)";
  else if (h.version != NEP_SNAPSHOT_VERSION) w = "a fleet snapshot of another version";
  else if (h.hdr_bytes != NEP_SNAPSHOT_HDR_BYTES) w = "a fleet snapshot with another header size";
  else if (!fields_ok(h)) w = "a fleet snapshot header with a field out of range";
  else if (h.scene_bytes <= 0 || h.scene_bytes % 16 != 0) w = "scene_bytes is not a positive multiple of 16";
  else if (layout(h, nullptr, nullptr) > h.scene_bytes) w = "a section of the scene block would end past scene_bytes";
  else if (layout(h, nullptr, nullptr) != h.scene_bytes) w = "scene_bytes is not what the header's fields give";
  if (why) *why = w;
  return w ? NEP_E_ARG : 0;
}

}  // namespace nep_recorder

extern "C" int nep_fleet_snapshot_describe(const void* host_blob, int64_t bytes, nep_fleet_snapshot_info* out) {
  if (!host_blob || !out) { nep::set_last_error("null argument"); return NEP_E_ARG; }
  if (bytes < (int64_t)NEP_SNAPSHOT_HDR_BYTES) { nep::set_last_error("fewer bytes than a snapshot header"); return NEP_E_ARG; }
  nep_fleet_snapshot_hdr h;
  std::memcpy(&h, host_blob, sizeof(h));
  const char* why = nullptr;
  if (nep_recorder::check_header(h, &why)) { nep::set_last_error(why); return NEP_E_ARG; }
  if ((bytes - NEP_SNAPSHOT_HDR_BYTES) / h.scene_bytes < h.n_scenes) { nep::set_last_error("fewer bytes than the header and its scene blocks"); return NEP_E_ARG; }
  std::memset(out, 0, sizeof(*out));
  out->hdr = h;
  nep_recorder::layout(h, out->offset, out->bytes);
  return 0;
}
