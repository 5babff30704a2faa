// fleet_recorder_kernels.hip — the fleet recorder's two copies (include/neptune_fleet.h, section "recorder"): the fleet state of every
// scene into a blob or a ring of blobs (fleet_snapshot_kernel: nep_batch_fleet_snapshot, nep_batch_fleet_snapshot_ring) and back
// (fleet_restore_kernel: nep_batch_fleet_restore).  The layout is recorder_common.h's; the host hands the kernels a table of
// sections — the handle's array, the scene's bytes of it, the offset in the block.
//
// Why a kernel and not a list of copies: inside a captured round every pointer of a copy node is fixed, and the ring's entry is
// round[scene] mod n_entries, which only the device knows.  A workgroup reads round[scene] from one address (a uniform load), so
// the block's base is the same in every lane.
//
// Layout of the work: a scene is shared by `parts` workgroups of 256 threads, the grid is capped (kRecorderMaxGrid) and strides
// over (scene, part).  Every section is copied at the widest access its size allows: a scene's part of an array starts at
// scene * bytes of an allocation, so 16-byte accesses need bytes % 16 == 0 — the rings, states, trajectories, published lists and
// the log at any N, the rest where N makes it so; otherwise 4 bytes (the per-slot int arrays at an N that is no multiple of 4),
// and single bytes only for a list-form sign array of an odd size.  The narrow paths write the section's zero padding.  Memory-bound
// and nothing else: no LDS, no atomics, no allocation; the ring's stamp and the header are ordinary vector stores.
#include <hip/hip_runtime.h>

#include "nep_device.h"

namespace nep {

namespace {

constexpr int kRecorderThreads = 256;
constexpr int kRecorderMaxGrid = 2048;
constexpr long kRecorderPartBytes = 64 * 1024;      // a workgroup's share of a scene block, about

// one section of one scene between the handle's array (`arr`, the scene's part) and the block (`blk`), by the threads
// first, first + step, ... of the scene's workgroups
template <bool kToBlob>
__device__ inline void recorder_copy(char* arr, char* blk, unsigned bytes, unsigned first, unsigned step) {
  if (bytes % 16 == 0) {
    uint4* a = (uint4*)arr; uint4* b = (uint4*)blk;
    for (unsigned i = first; i < bytes / 16; i += step) { if (kToBlob) b[i] = a[i]; else a[i] = b[i]; }
  } else if (bytes % 4 == 0) {
    unsigned* a = (unsigned*)arr; unsigned* b = (unsigned*)blk;
    const unsigned n = bytes / 4, n_pad = (bytes + 15) / 16 * 4;
    if (kToBlob) for (unsigned i = first; i < n_pad; i += step) b[i] = i < n ? a[i] : 0u;
    else for (unsigned i = first; i < n; i += step) a[i] = b[i];
  } else {
    const unsigned n_pad = (bytes + 15) / 16 * 16;
    if (kToBlob) for (unsigned i = first; i < n_pad; i += step) blk[i] = i < bytes ? arr[i] : (char)0;
    else for (unsigned i = first; i < bytes; i += step) arr[i] = blk[i];
  }
}

__global__ __launch_bounds__(kRecorderThreads) void fleet_snapshot_kernel(RecorderArgs ra) {
  const int n_scenes = ra.hdr.n_scenes, parts = ra.parts;
  const long scene_bytes = ra.hdr.scene_bytes;
  if (blockIdx.x == 0 && threadIdx.x == 0) *(nep_fleet_snapshot_hdr*)ra.blob = ra.hdr;
  for (int w = blockIdx.x; w < n_scenes * parts; w += gridDim.x) {
    const int scene = w / parts, part = w - scene * parts;
    char* blk;
    if (ra.n_entries > 0) {
      const int round = ra.round[scene];      // (one address for the workgroup: uniform)
      const int entry = (int)((unsigned)round % (unsigned)ra.n_entries);
      const long at = (long)entry * n_scenes + scene;
      char* stamps = ra.blob + NEP_SNAPSHOT_HDR_BYTES;
      if (part == 0 && threadIdx.x == 0) ((int4*)stamps)[at] = make_int4(1, round, ra.origin[scene], 0);
      blk = stamps + (long)ra.n_entries * n_scenes * 16 + at * scene_bytes;
    } else {
      blk = ra.blob + NEP_SNAPSHOT_HDR_BYTES + (long)scene * scene_bytes;
    }
    const unsigned first = (unsigned)part * kRecorderThreads + threadIdx.x, step = (unsigned)parts * kRecorderThreads;
    for (int i = 0; i < NEP_SNAPSHOT_N_SECTIONS; i++) {
      const RecorderSection& s = ra.sec[i];
      if (s.bytes) recorder_copy<true>(s.p + (long)scene * s.bytes, blk + s.off, s.bytes, first, step);
    }
  }
}

__global__ __launch_bounds__(kRecorderThreads) void fleet_restore_kernel(RecorderArgs ra) {
  const int parts = ra.parts, n = ra.src_scene < 0 ? ra.hdr.n_scenes : 1;
  const long scene_bytes = ra.hdr.scene_bytes;
  for (int w = blockIdx.x; w < n * parts; w += gridDim.x) {
    const int k = w / parts, part = w - k * parts;
    const int src = ra.src_scene < 0 ? k : ra.src_scene, dst = ra.src_scene < 0 ? k : ra.dst_scene;
    char* blk = ra.blob + NEP_SNAPSHOT_HDR_BYTES + (long)src * scene_bytes;
    const unsigned first = (unsigned)part * kRecorderThreads + threadIdx.x, step = (unsigned)parts * kRecorderThreads;
    for (int i = 0; i < NEP_SNAPSHOT_N_SECTIONS; i++) {
      const RecorderSection& s = ra.sec[i];
      if (s.bytes) recorder_copy<false>(s.p + (long)dst * s.bytes, blk + s.off, s.bytes, first, step);
    }
  }
}

int recorder_parts(long scene_bytes, int n_scenes) {
  long parts = (scene_bytes + kRecorderPartBytes - 1) / kRecorderPartBytes;
  const long most = kRecorderMaxGrid / (n_scenes < kRecorderMaxGrid ? n_scenes : kRecorderMaxGrid);
  if (parts > most) parts = most;
  return parts < 1 ? 1 : (int)parts;
}

}  // namespace

void launch_fleet_snapshot(const RecorderArgs& ra_in, hipStream_t st) {
  RecorderArgs ra = ra_in;
  ra.parts = recorder_parts(ra.hdr.scene_bytes, ra.hdr.n_scenes);
  const long work = (long)ra.hdr.n_scenes * ra.parts;
  hipLaunchKernelGGL(fleet_snapshot_kernel, dim3((unsigned)(work < kRecorderMaxGrid ? work : kRecorderMaxGrid)), dim3(kRecorderThreads), 0, st, ra);
}

void launch_fleet_restore(const RecorderArgs& ra_in, hipStream_t st) {
  RecorderArgs ra = ra_in;
  const int n = ra.src_scene < 0 ? ra.hdr.n_scenes : 1;
  ra.parts = recorder_parts(ra.hdr.scene_bytes, n);
  const long work = (long)n * ra.parts;
  hipLaunchKernelGGL(fleet_restore_kernel, dim3((unsigned)(work < kRecorderMaxGrid ? work : kRecorderMaxGrid)), dim3(kRecorderThreads), 0, st, ra);
}

}  // namespace nep
