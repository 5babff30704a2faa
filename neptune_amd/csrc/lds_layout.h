// lds_layout.h — the dynamic-LDS layout of every kernel that carves `extern __shared__` memory outside the QP kernels: one struct per
// kernel with the byte offset of every array, the launch's byte count and the counts derived from them, and one function that fills
// it.  The kernel takes its pointers from the struct (lds_at), the launcher its byte count and whatever it passes or sizes global
// memory with: an array added to a carve is added here, once, for both.  (The unpacked separator is passed its pool's size, pool_pairs,
// as before, and carves behind it with the function the launch's layout is made of, sep_carve.  The packed separator keeps its own
// carve: every form of it on this header measured 2 % slower at 256 agents with the entangle rows)  Plain C++, no HIP include, plain integers and flags in:
// tests/cpp/lds_layout_check.cpp runs every layout on the CPU (inside the launch, aligned, disjoint but for the declared aliases)
// and tests/golden/lds_bytes.json pins the byte counts to the formulas the launchers had before this header existed.
// Every dynamic carve starts 16-byte aligned (`extern __shared__ __attribute__((aligned(16)))`); the static LDS of these kernels
// is a multiple of 16 bytes, so an offset's alignment is the array's.  Offsets are ints: a shape the handles admit (65 535
// candidates per segment at most, size_scratch) stays far below 2^31; the audit, whose polygon count is not bounded that way, counts
// in 64 bits.  A shape whose bytes exceed the chip's 160 KB fails at launch, as before (HIPCHK(hipGetLastError())).
#ifndef NEP_LDS_LAYOUT_H_
#define NEP_LDS_LAYOUT_H_

#include "../../include/neptune_backend.h"
#include "../../include/neptune_frontend.h"
#include "../../include/neptune_fleet.h"

#if defined(__HIPCC__)
#define NEP_LDS_HD __host__ __device__ __forceinline__
#else
#define NEP_LDS_HD inline
#endif

namespace nep {

// The array of T at byte offset off of the carve.  An array's offset is a multiple of its element's size (the CPU check verifies
// it), and the address is formed the way `base + elements` forms it: the compiler sees the same indexing the hand-written carves gave
// it (with the offset added as bytes, the big-record front end took five registers more).  lds_rec: a record whose size is not its
// alignment (nep_fe_ent_state).
template <class T> NEP_LDS_HD T* lds_at(void* base, int off) { return (T*)base + off / (int)sizeof(T); }
template <class T> NEP_LDS_HD T* lds_at(void* base, long long off) { return (T*)base + off / (long long)sizeof(T); }
template <class T> NEP_LDS_HD T* lds_rec(void* base, int off) { return (T*)((char*)base + off); }
NEP_LDS_HD int lds_up(int v, int a) { return (v + a - 1) & ~(a - 1); }      // a: a power of two

// ---- constants the layouts are made of ----------------------------------------------------------------------------------------------
// Dynamic LDS a separator wave aims at: 10 KB, so that sixteen waves share a CU (see separator_body, geom_kernels.hip)
#ifndef NEP_SEP_LDS
#define NEP_SEP_LDS (10 * 1024)
#endif
constexpr int kSepLdsTarget = NEP_SEP_LDS;
constexpr int kFeObsLds = 24;   // shortlisted obstacles whose vertices are staged in LDS (the rest are read from global memory)
#ifndef NEP_FE_ENT_WGS
#define NEP_FE_ENT_WGS 3      // (round 4: 3 = 168 registers, 48 spilled, 52 KB of LDS at config 5) // workgroups per CU of the entangle instantiation: 2 = working records in global memory, registers bounded to 256 (19.9 ms per 2 048 config-5 searches); 1 = working records in LDS, 139 KB (27.4 ms: the list surgery is latency-bound, a second workgroup hides more than LDS saves)
#endif
constexpr int kEntAddCap = 32;      // new crossings one sampled step may add (EntAdd, ent_device.h)
constexpr int kEntLdsBytes = ((NEP_FE_ENT_CAP * 3 + NEP_MAX_BEND + 3) & ~3) | 4;      // a crossing list in LDS, per thread; an odd number of dwords, so that the threads' lists fall into different banks
constexpr int kEntBigLdsCap = 120, kEntBigLdsBend = 16;      // the big-record instantiation's lists (ent_lds_load_big, ent_device.h)
constexpr int kEntBigLdsBytes = ((kEntBigLdsCap * 3 + kEntBigLdsBend + 3) & ~3) | 4;      // per thread; an odd number of dwords
constexpr int kLdsPerCu = 160 * 1024;

// The front end's LDS arrays are sized for the configured beam width (not the maximum), so that narrower beams leave room for
// more workgroups per CU: cap = beam_width * num_samples^2 candidates per depth, hash tables a power of two above
// 1.25x (per-depth voxel table) / 2x (visited voxels, beam_width * num_pol keys) their load.
struct FeSizes { int cap, dd, vis, mb; };
NEP_LDS_HD FeSizes fe_sizes(int beam_width, int num_samples, int num_pol) {
  FeSizes z; z.cap = beam_width * num_samples * num_samples; if (z.cap < 64) z.cap = 64;
  z.dd = 64; while (z.dd * 4 < z.cap * 5) z.dd *= 2;
  z.vis = 64; while (z.vis < 2 * beam_width * num_pol) z.vis *= 2;
  z.mb = beam_width <= 32 ? 32 : NEP_FE_MAX_BEAM;      // stride of the per-rank arrays (the beam's width rounded up: a width-32 beam does not pay for 64 ranks of LDS)
  return z;
}

// ---- 1. separator_body (separator_kernel<RULE>, separator_redo_kernel<RULE>) ---------------------------------------------------------
// The pool of point sets takes what the fixed parts leave of kSepLdsTarget; with very long candidate lists (config 5 with the
// entangle rows) it keeps at least 64 x 8 pairs and the wave gets more LDS.
struct SepLayout {
  int sA;         // [pool_pairs] double2: the batch's point sets A, packed
  int sBx, sBy;   // [4] double each: the segment's control points
  int sAtt;       // [total + 8] unsigned short: the LPs the reference calls (total: every candidate of a segment)
  int sAct;       // [N] unsigned short: agents with an active entangle case (ent_enabled; behind sAtt's total + 8 entries)
  int pool_pairs, bytes;
};
NEP_LDS_HD int sep_total(int n_hull, int N, int S, bool ent_enabled) { return n_hull + N + S + (ent_enabled ? N * NEP_MAX_BEND : 0); }
// the offsets behind a pool of pool_pairs pairs: what the wave works out, from the pool_pairs the launch passes it (bytes: not set)
NEP_LDS_HD SepLayout sep_carve(int pool_pairs, int total) {
  SepLayout L;
  L.sA = 0; L.pool_pairs = pool_pairs;
  L.sBx = pool_pairs * 16; L.sBy = L.sBx + 4 * 8;
  L.sAtt = L.sBy + 4 * 8;
  L.sAct = L.sAtt + (total + 8) * 2;
  L.bytes = 0;
  return L;
}
// the launch: the pool's size, then the same carve
NEP_LDS_HD SepLayout sep_layout(int n_hull, int N, int S, bool ent_enabled) {
  const int total = sep_total(n_hull, N, S, ent_enabled);
  const int tail = 8 * 8 + lds_up((total + 8 + (ent_enabled ? N : 0)) * 2, 16);
  const int pool = (tail + 64 * 8 * 16 <= kSepLdsTarget ? kSepLdsTarget - tail : 64 * 8 * 16) & ~15;
  SepLayout L = sep_carve(pool / 16, total);
  L.bytes = pool + tail;
  return L;
}

// ---- 2. frontend_kernel<ENT, WGS, BIG> ------------------------------------------------------------------------------------------------
// big: the big-record instantiation with its per-thread lists in LDS (launch_frontend asks for them when it has their betas' global
// memory; they are granted when the launch stays within the CU's LDS).  ent_wgs: NEP_FE_ENT_WGS — 1 puts the working records in LDS.
struct FeLayout {
  FeSizes z;
  // arrays of their own, in carve order
  int s_f;                    // [cap] double: f of candidate id
  int b_end;                  // [2][mb][6] double
  int b_g;                    // [2][mb] double
  int b_dist, b_f;            // [mb] double each
  int p_box;                  // [mb][4] double: box of every parent's children
  int o_aabb;                 // [N+S][4] double: boxes of the shortlisted obstacles, dense
  int o_V;                    // [kFeObsLds][16][2] double: their vertices
  int s_lat;                  // [4][NEP_FE_MAX_SAMPLES] double: lattice tables
  int s_vox;                  // [cap] 64-bit
  int v_key;                  // [vis] 64-bit: visited voxels
  int d_slot;                 // [dd] int: voxel -> best candidate of the depth
  int o_nv, o_id;             // [N+S] int each, dense
  int s_i;                    // [32] int: counters
  int r_id;                   // [cap] unsigned short: ids of the voxel winners, dense
  int s_state;                // [cap] bytes
  int p_parent, p_comb;       // [NEP_MAX_POL + 1][mb] bytes each
  int b_valid;                // [mb] bytes
  // ... with the entangle check (ent) only
  int m_ent, m_base;          // [mb][MW] unsigned each
  int m_stat;                 // [mb][SW] unsigned
  int f_bits;                 // [N] bytes
  int x_U;                    // [2][MW] unsigned: cross_round's union mask and its prefix counts
  int work;                   // [256] nep_fe_ent_state: the threads' working records (ent_wgs == 1 only; -1: they are in global memory)
  int big_lds_off;            // [256][kEntBigLdsBytes]: the big-record instantiation's lists, behind everything else (big only; 0: none)
  // ALIASES: arrays that live in another's storage while its contents are dead
  bool rf_alias;              // r_f lives in o_aabb + o_V (they are big enough: 4 (N + S) + 768 >= cap), else it has storage of its own behind o_V
  int r_f;                    // [cap] double: f of the voxel winners, dense — written by the compaction, when the shortlist's boxes and vertices are dead
  int ent_lists;              // = o_aabb; [n_lists_a][kEntLdsBytes] over o_aabb, o_V and, when it has storage of its own, r_f: between a depth's GJK pass and its compaction
  int n_lists_a;              // crossing lists that storage holds
  int n_lists_b;              // ... d_slot's (the voxel table is dead, all -1, during the propagation)
  int n_lists_c;              // ... s_f's, and s_vox's as many again (big-record instantiation without lists of its own)
  int x_hdr, x_pool;          // = s_f, s_vox; [x_words] unsigned each: cross_round's headers and pool (fast instantiation)
  int x_words;
  int p_list;                 // = r_id; [cap] unsigned short: the survivors of a depth (the GJK work list has been consumed)
  int x_ids;                  // = o_id; the staged agents of cross_round (the shortlist's ids are dead by then)
  int x_rec, x_rec_bytes;     // = o_aabb; the staged packed records, over o_aabb and o_V
  int bytes;
};
NEP_LDS_HD FeLayout fe_layout(int N, int S, int beam_width, int num_samples, int num_pol, bool ent, bool big = false, int ent_wgs = NEP_FE_ENT_WGS) {
  FeLayout L;
  const FeSizes z = fe_sizes(beam_width, num_samples, num_pol);
  const int cap = z.cap, MB = z.mb, NS = N + S, V = kFeObsLds * NEP_HULL_MAX_V * 2, MW = (N + 31) >> 5, SW = (S + 31) >> 5;
  L.z = z;
  L.s_f = 0;
  L.b_end = L.s_f + cap * 8;
  L.b_g = L.b_end + 2 * MB * 6 * 8;
  L.b_dist = L.b_g + 2 * MB * 8;
  L.b_f = L.b_dist + MB * 8;
  L.p_box = L.b_f + MB * 8;
  L.o_aabb = L.p_box + MB * 4 * 8;
  L.o_V = L.o_aabb + 4 * NS * 8;
  L.rf_alias = 4 * NS + V >= cap;
  L.r_f = L.rf_alias ? L.o_aabb : L.o_V + V * 8;
  L.s_lat = L.o_V + V * 8 + (L.rf_alias ? 0 : cap * 8);
  L.s_vox = L.s_lat + 4 * NEP_FE_MAX_SAMPLES * 8;
  L.v_key = L.s_vox + cap * 8;
  L.d_slot = L.v_key + z.vis * 8;
  L.o_nv = L.d_slot + z.dd * 4;
  L.o_id = L.o_nv + NS * 4;
  L.s_i = L.o_id + NS * 4;
  L.r_id = L.s_i + 32 * 4;
  L.s_state = L.r_id + cap * 2;
  L.p_parent = L.s_state + cap;
  L.p_comb = L.p_parent + (NEP_MAX_POL + 1) * MB;
  L.b_valid = L.p_comb + (NEP_MAX_POL + 1) * MB;
  int end = L.b_valid + MB;
  L.m_ent = L.m_base = L.m_stat = L.f_bits = L.x_U = 0; L.work = -1;
  if (ent) {
    L.m_ent = lds_up(end, 4);      // (every array before r_id is a multiple of four bytes; r_id and s_state are 3 cap)
    L.m_base = L.m_ent + MB * MW * 4;
    L.m_stat = L.m_base + MB * MW * 4;
    L.f_bits = L.m_stat + MB * SW * 4;
    L.x_U = lds_up(L.f_bits + N, 4);
    end = L.x_U + 2 * MW * 4;
    if (ent_wgs == 1) { L.work = lds_up(L.f_bits + N + 3 + 8 * MW, 8); end = L.f_bits + lds_up(N, 4) + 8 * MW + 256 * (int)sizeof(nep_fe_ent_state) + 8; }
  }
  L.bytes = lds_up(end, 16);
  L.ent_lists = L.o_aabb; L.n_lists_a = (L.s_lat - L.o_aabb) / kEntLdsBytes;
  L.n_lists_b = z.dd * 4 / kEntLdsBytes; L.n_lists_c = cap * 8 / kEntLdsBytes;
  L.x_hdr = L.s_f; L.x_pool = L.s_vox; L.x_words = cap * 8 / 4;
  L.p_list = L.r_id; L.x_ids = L.o_id; L.x_rec = L.o_aabb; L.x_rec_bytes = (4 * NS + V) * 8;
  L.big_lds_off = 0;
  if (big && ent && L.bytes + 256 * kEntBigLdsBytes <= kLdsPerCu) { L.big_lds_off = L.bytes; L.bytes += 256 * kEntBigLdsBytes; }
  return L;
}
// words per slot of the global fallback of cross_round's LDS pool (FeEntArgs::xpool): survivors per round of the fast instantiation's
// propagation pass x sampled steps x kEntAddCap
NEP_LDS_HD long long fe_xpool_words(const FeLayout& L, int ent_ns) {
  const int n = L.n_lists_a + L.n_lists_b;
  return (long long)(n > 256 ? 256 : n) * (ent_ns > 0 ? ent_ns : 1) * kEntAddCap;
}

// ---- 3. ent_check_kernel ------------------------------------------------------------------------------------------------------------
struct EntCheckLayout {
  int m_agent, m_static;      // [2 ceil(N / 64)], [2 ceil(S / 64)] unsigned: who may add a crossing (+ 2 spare words: an even number, so that the record is 8-byte aligned)
  int work;                   // [1] nep_fe_ent_state: lane 0's working record
  int bytes;
};
NEP_LDS_HD EntCheckLayout ent_check_layout(int N, int S) {
  EntCheckLayout L;
  L.m_agent = 0; L.m_static = ((N + 63) >> 6) * 2 * 4;
  L.work = 2 * (((N + 63) >> 6) + ((S + 63) >> 6) + 1) * 4;
  L.bytes = L.work + (int)sizeof(nep_fe_ent_state);
  return L;
}

// ---- 4. safety_resolve_kernel -------------------------------------------------------------------------------------------------------
// quadratic in N: above the 64 KB default from N = 682 on (launch_safety raises the limit: up to N ~ 1 100)
struct ResolveLayout {
  int sAcc, sBad;             // [N] int each: accept flags, forced-bad flags
  int sRow;                   // [N][W] unsigned: symmetric conflict rows, W = ceil(N / 32)
  int sBits;                  // [W] unsigned: accepted ids so far, when they do not fit eight registers (N > 256)
  int W, bytes;
};
NEP_LDS_HD ResolveLayout resolve_layout(int N) {
  ResolveLayout L;
  L.W = (N + 31) >> 5;
  L.sAcc = 0; L.sBad = N * 4; L.sRow = 2 * N * 4; L.sBits = L.sRow + N * L.W * 4;
  L.bytes = L.sBits + L.W * 4;
  return L;
}

// ---- 5. audit_chunk_kernel ----------------------------------------------------------------------------------------------------------
struct AuditLayout {
  long long pxy;              // [S][vstride][2] double: polygon vertices
  long long pinv;             // [S][vstride] double: 1 / |edge|^2
  long long ag;               // [N][4] double: x, y, hx, hy
  long long pnv;              // [S] int: vertex counts
  long long apres;            // [N] int
  long long bytes;
};
NEP_LDS_HD AuditLayout audit_layout(int N, int S, int vstride) {
  AuditLayout L;
  const long long sv = (long long)S * vstride;
  L.pxy = 0; L.pinv = sv * 2 * 8; L.ag = L.pinv + sv * 8; L.pnv = L.ag + (long long)N * 4 * 8; L.apres = L.pnv + (long long)S * 4;
  L.bytes = L.apres + (long long)N * 4;
  return L;
}

// ---- 5b. span_audit_kernel (audit_span_kernels.hip) -----------------------------------------------------------------------------------
// (pieces: kSpanLdsPieces, piece_bytes: sizeof(SpanPiece), both audit_span_common.h's — this header knows neither)
struct SpanAuditLayout {
  long long pxy;              // [S][vstride][2] double: polygon vertices
  long long pinv;             // [S][vstride] double: 1 / |edge|^2
  long long pc;               // [N][pieces] SpanPiece: a record's pieces inside the window
  long long ts;               // [N][pieces] double: where each begins
  long long hxy;              // [N][2] double: inflated half-widths
  long long box;              // [N][4] double: a box round the record's positions over the window (the pruning bound)
  long long pnv;              // [S] int: vertex counts
  long long npc;              // [N] int: pieces staged (-1: more than `pieces`, read the record)
  long long apres;            // [N] int
  long long bytes;
};
NEP_LDS_HD SpanAuditLayout span_audit_layout(int N, int S, int vstride, int pieces, int piece_bytes) {
  SpanAuditLayout L;
  const long long sv = (long long)S * vstride, np = (long long)N * pieces;
  L.pxy = 0; L.pinv = sv * 2 * 8; L.pc = L.pinv + sv * 8; L.ts = L.pc + np * piece_bytes; L.hxy = L.ts + np * 8;
  L.box = L.hxy + (long long)N * 2 * 8;
  L.pnv = L.box + (long long)N * 4 * 8; L.npc = L.pnv + (long long)S * 4; L.apres = L.npc + (long long)N * 4;
  L.bytes = L.apres + (long long)N * 4;
  return L;
}

// ---- 6. fleet_mission_kernel --------------------------------------------------------------------------------------------------------
// (the kernel carves with its scene's vertex and polygon counts, the launch is sized with NEP_MISSION_MAX_VERT and NEP_MISSION_MAX_POLY)
struct MissionLayout {
  int s_end, s_new;           // [N][3] double each: end positions; goals drawn in this call (before that: the leg lengths)
  int s_kxy;                  // [n_vert][2] double: keep-out vertices
  int s_got;                  // [N] int: what to do per agent
  int s_off;                  // [n_poly + 1] int: polygon offsets
  int bytes;
};
NEP_LDS_HD MissionLayout mission_layout(int N, int n_vert, int n_poly) {
  MissionLayout L;
  L.s_end = 0; L.s_new = 3 * N * 8; L.s_kxy = L.s_new + 3 * N * 8; L.s_got = L.s_kxy + 2 * n_vert * 8; L.s_off = L.s_got + N * 4;
  L.bytes = L.s_off + (n_poly + 1) * 4;
  return L;
}

// ---- 7. frontend_astar_kernel<true> (fe_astar.h) --------------------------------------------------------------------------------------
// One wave per search, a fixed shape: 24.3 KB, six searches per CU by LDS (the kernel's registers admit no more than that either).
// The working records are what the carve is for: a child's list surgery is a chain of dependent reads and writes of its record, which
// in global memory are round trips (ent_check_kernel).  frontend_astar_kernel<false> has no records and keeps static arrays of the
// same two sizes.
constexpr int kAsNC = NEP_FE_MAX_SAMPLES * NEP_FE_MAX_SAMPLES;      // the children of an expansion, one lane each
constexpr int kAsHeapLds = 2048;                                    // heap entries kept in LDS (levels 0-10 of the heap: every sift starts or ends there)
struct AstarEntLayout {
  int work;                   // [kAsNC + 1] nep_fe_ent_state: every lane's child state; the last one is the expansion's parent, staged once
  int ch;                     // [kAsNC][17] double: a child of the expansion at hand (end state, cx, cy, g, h, cost)
  int hcost;                  // [kAsNC] double: per voxel group, the holder's cost
  int lat;                    // [4][NEP_FE_MAX_SAMPLES] double: lattice tables
  int heap;                   // [kAsHeapLds] int
  int ints;                   // [10][kAsNC] int: vx, vy, iz, f, pos, hst, hidx, new, grp, valid
  int path;                   // [NEP_MAX_POL + 2] int: the returned path's nodes by index; [NEP_MAX_POL + 1]: the rows to fill
  int bytes;
};
NEP_LDS_HD AstarEntLayout astar_ent_layout() {
  AstarEntLayout L;
  L.work = 0; L.ch = (kAsNC + 1) * (int)sizeof(nep_fe_ent_state); L.hcost = L.ch + kAsNC * 17 * 8; L.lat = L.hcost + kAsNC * 8;
  L.heap = L.lat + 4 * NEP_FE_MAX_SAMPLES * 8; L.ints = L.heap + kAsHeapLds * 4; L.path = L.ints + 10 * kAsNC * 4;
  L.bytes = lds_up(L.path + (NEP_MAX_POL + 2) * 4, 16);
  return L;
}

// ---- 8. frontend_astar_team_kernel (fe_astar.h) ---------------------------------------------------------------------------------------
// Four waves per search (nep_batch_set_fe_astar_team): the one-wave carve as it is, at the same offsets (`one`), and behind it what
// the dense crossing pass leaves for the surgery — a header word and kEntAddCap list words per (child, sampled step), the format of
// ent_cross_step / ent_propagate_pre — plus what the four waves hand each other.  A fixed shape, 79.2 KB: two workgroups per CU by LDS, as by registers (207).
constexpr int kAsTeamWaves = 4, kAsTeamThreads = 64 * kAsTeamWaves;
constexpr int kAsTeamSteps = 8;       // sampled steps of a child: nep_fe_cfg.ent_samples <= 8
constexpr int kAsTeamChunks = 8;      // contiguous chunks of the obstacle index range one (child, step) is split into, at most
constexpr int kAsTeamCtl = 16;        // control words (fe_astar.h: kTc*)
struct AstarEntTeamLayout {
  AstarEntLayout one;         // [0, one.bytes): astar_ent_layout(), offsets unchanged
  int x_hdr;                  // [kAsNC][kAsTeamSteps] unsigned: offset | n << 16 | overflow << 24 of a (child, step)'s list
  int x_pool;                 // [kAsNC * kAsTeamSteps][kEntAddCap] unsigned: the lists, one fixed block per (child with "have", step)
  int x_stage;                // [kAsTeamThreads][kEntAddCap - 4] unsigned: the tail of the list a work item is making (EntAdd::rest)
  int x_cn;                   // [kAsTeamThreads] unsigned: a work item's n | peak << 8 | overflow << 16
  int have;                   // [kAsNC] int: the children with "have", dense, in lattice order
  int ctl;                    // [kAsTeamCtl] int: loop control and verdicts
  int bytes;
};
NEP_LDS_HD AstarEntTeamLayout astar_ent_team_layout() {
  AstarEntTeamLayout L;
  L.one = astar_ent_layout();
  L.x_hdr = L.one.bytes;
  L.x_pool = L.x_hdr + kAsNC * kAsTeamSteps * 4;
  L.x_stage = L.x_pool + kAsNC * kAsTeamSteps * kEntAddCap * 4;
  L.x_cn = L.x_stage + kAsTeamThreads * (kEntAddCap - 4) * 4;
  L.have = L.x_cn + kAsTeamThreads * 4;
  L.ctl = L.have + kAsNC * 4;
  L.bytes = lds_up(L.ctl + kAsTeamCtl * 4, 16);
  return L;
}
static_assert(kAsNC * kAsTeamSteps <= kAsTeamThreads, "one work item per (child, step) at least: the dense pass is one round");
static_assert(kAsNC * kAsTeamSteps * kEntAddCap <= 0xffff, "a list's offset is 16 bits of its header word");
static_assert(kEntAddCap <= 0xff, "a work item's n and peak are 8 bits each");
static_assert(kAsNC <= 64, "the children are wave 0's lanes");

}  // namespace nep
#endif
