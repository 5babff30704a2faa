/* neptune_hastar.h — the reference's single-agent benchmark search (NeptuneRos::replanCB with enable_single_benchmark,
 * neptune_ros.cpp:491-613): AstarPathFinder (neptune/src/Astar_searcher.cpp), a grid A* whose nodes carry a homotopy signature
 * and a list of tether contact points ("Path Planning for a Tethered Mobile Robot", ICRA 2014), thousands of searches per
 * launch.  C99, self-contained: it includes no other header of this library.  A handle of its own; nothing here reads or
 * changes a nep_batch_t.
 *
 * The rules are the reference's, one for one (DESIGN.md section 39 lists them): the grid and its truncating index, occupancy as
 * gjk::collision of the inflated polygons with the +-0.05 box of a cell's centre, the successor order and the float diagonal
 * cost, updateHSig_orig with its last-entry-only cancellation, the cable test in mixed units (cells against metres) that runs
 * updateContPts_orig on the child's list only when the cell count exceeds the cable, getIz in 32-bit modular arithmetic, the
 * exact-match node table on (ix, iy, iz), libstdc++'s heap under CompareCost with in-place updates that do not re-order it,
 * and getPath.  The reference's 30 s wall-clock limit is a budget of pops, tested at the top of the loop.
 *
 * The device form (nep_hastar_search, one wave per search) and the host form (nep_hastar_search_host, no HIP call) are one
 * function compiled twice (neptune_amd/csrc/hastar_common.h) and agree on every output byte.                                  */
#ifndef NEPTUNE_HASTAR_H_
#define NEPTUNE_HASTAR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef NEP_E_ARG
#define NEP_E_ARG (-1)
#define NEP_E_STATE (-2)
#define NEP_E_HIP (-3)
#define NEP_E_CAP (-4)
#endif

/* nep_hastar_result.flags.  The reference's lists are std::vectors; the capacities are this build's, and a search says when
 * one of them bound:
 *   HSIG   a child whose signature would hold more than hsig_cap entries was dropped
 *   CONT   a child whose contact list would hold more than cont_cap points (before or after updateContPts_orig) was dropped
 *   PATH   the path has more than path_cap points; the first path_cap are returned, length_m is their length
 *   POOL   a child whose shortened contact list did not fit the search's pool (8 points per node of max_nodes) was dropped
 *   STATE  the slot's input was malformed (scene index out of range, n_hsig > hsig_cap, n_cont < 1 or > cont_cap, a start, goal
 *          or contact point that is not finite or beyond NEP_HASTAR_MAX_COORD in magnitude): status -1, nothing searched, the
 *          terminal state is the empty one                                                                                 */
#define NEP_HASTAR_FLAG_HSIG 1
#define NEP_HASTAR_FLAG_CONT 2
#define NEP_HASTAR_FLAG_PATH 4
#define NEP_HASTAR_FLAG_POOL 8
#define NEP_HASTAR_FLAG_STATE 16

#define NEP_HASTAR_MAX_COORD 100000.0 /* |x|, |y| of every point a search is given (updateContPts_orig samples every 0.2 m) */
#define NEP_HASTAR_MAX_REP 256     /* reps per scene (the crossing tests of a step are bit masks of this many bits) */
#define NEP_HASTAR_POOL_PER_NODE 8  /* points of the shortened-list pool per node of max_nodes */

/* nep_abi_sizeof(31): 96 bytes.  The reference's set-up (neptune_ros.cpp:347-351): resolution = a_star_fraction_voxel_size * 2,
 * the world's bounds, cable_length = tetherLength, bias = 1.1.  max_nodes = 0 takes the reference's pool, GLX * GLY * GLZ.   */
typedef struct nep_hastar_cfg {
  double resolution, x_min, x_max, y_min, y_max, z_min, z_max, cable_length, bias;
  int32_t max_pops, max_nodes;
  int32_t hsig_cap, cont_cap, path_cap;
} nep_hastar_cfg;

/* nep_abi_sizeof(32): 48 bytes.  nodes_used is node_used_num_, g_cells the terminal node's gScore (cells), length_m getPath's
 * length.  n_updates: open nodes overwritten in place; n_length_checks: children whose cell count exceeded the cable (each ran
 * updateContPts_orig); n_cable_pruned: those still longer than the cable afterwards.  Without success n_path, g_cells and
 * length_m are 0 and the terminal state is the initial one (the reference leaves terminal_ent_state_ alone).                */
typedef struct nep_hastar_result {
  int32_t status;                 /* 1 reached, 0 budget of pops spent, -1 open list empty */
  int32_t n_path, nodes_used, pops, n_updates, n_length_checks, n_cable_pruned;
  int32_t flags;
  double g_cells, length_m;
} nep_hastar_result;

/* nep_abi_sizeof(33): 48 bytes.  eu::ent_state_orig of `slots` searches as a struct of arrays (the style of nep_ent_lists).
 * The struct lives in host memory; its members point to host arrays (nep_hastar_search_host) or device arrays
 * (nep_hastar_search):
 *   n_hsig [slots], hsig_id [slots][hsig_cap] (1-based rep index), hsig_sign [slots][hsig_cap] (+1 / -1)
 *   n_cont [slots], cont [slots][cont_cap][2]       (contPts; the reference starts it as [base], so n_cont >= 1)
 * Entries beyond the counts are zero on the way in and on the way out.  hsig_cap and cont_cap are the handle's.              */
typedef struct nep_hastar_state {
  int32_t hsig_cap, cont_cap;
  int32_t* n_hsig;
  int16_t* hsig_id;
  int8_t* hsig_sign;
  int32_t* n_cont;
  double* cont;
} nep_hastar_state;

typedef struct nep_hastar nep_hastar_t;

/* No HIP call: a handle serves the host form on a machine without a GPU.  NULL (and nep_last_error) on a bad configuration:
 * a resolution, bias or cable that is not finite and positive, a grid without cells, caps < 1, max_pops < 0, n_scenes < 1.   */
nep_hastar_t* nep_hastar_create(const nep_hastar_cfg* cfg, int32_t n_scenes);
void nep_hastar_destroy(nep_hastar_t* h);

/* The statics of a scene, as the reference's three setters take them (setStaticObstVert's two lists, setStaticObstRep); the
 * counts are independent.  Polygons are CSR: off[n_poly + 1], xy[off[n_poly]][2]; every polygon has at least one vertex.
 * rep[n_rep][2][2]: rep[r][0] is staticObsRep[r].col(0), rep[r][1] is .col(1).  scene = -1 sets every scene.  Host arrays,
 * copied.  NEP_E_ARG on bad arguments, NEP_E_CAP beyond NEP_HASTAR_MAX_REP reps.  The next device search uploads them (that
 * call is eager: not inside a stream capture).                                                                              */
int nep_hastar_set_inflated(nep_hastar_t* h, int32_t scene, int32_t n_poly, const int32_t* off, const double* xy);
int nep_hastar_set_uninflated(nep_hastar_t* h, int32_t scene, int32_t n_poly, const int32_t* off, const double* xy);
int nep_hastar_set_reps(nep_hastar_t* h, int32_t scene, int32_t n_rep, const double* rep);

/* The inflation of neptune_ros.cpp:313-343: every vertex spread to its four corners at safe_dist = 2 * drone_radius, then the
 * convex hull, counter-clockwise from the lowest of the leftmost points.  Returns the number of vertices written to
 * xy_out[cap][2], NEP_E_CAP when they do not fit, NEP_E_ARG on bad arguments.  Host only.                                  */
int nep_hastar_inflate(int32_t n_vert, const double* xy, double drone_radius, double* xy_out, int32_t cap);

/* gjk::collision(vertices1, vertices2) as the search runs it, general in both vertex counts (occupancy has four points on the
 * second side, updateContPts_orig's line two): 1 collision, 0 none, NEP_E_ARG on a null pointer or a count < 1.  Host only.  */
int nep_hastar_gjk(int32_t n1, const double* xy1, int32_t n2, const double* xy2);

/* Bytes of working memory one search takes (nodes, signatures, heap, node table, contact-list pool): 212 + 3 hsig_cap
 * bytes per node of max_nodes at the most, plus 16 cont_cap.                                                                      */
int64_t nep_hastar_search_bytes(const nep_hastar_t* h);

/* n_search searches.  Search s runs in scene scene[s] from start[s] to goal[s] ([n_search][2]) with the initial tether state
 * state_in slot s, and writes result[s], path[s] ([n_search][path_cap][2], rows beyond n_path zero: the un-rounded start
 * first, the goal's cell centre last) and the terminal state into state_out slot s, in state_in's layout, so that searches
 * chain (neptune_ros.cpp:1667-1670) without a host round trip.  state_out may name state_in's arrays.
 *
 * nep_hastar_search: every pointer names device memory.  Asynchronous on `stream`.  The first call (and the first one after
 * a setter, or with more searches than any before) allocates and uploads and must be eager; later calls allocate nothing and
 * are capturable.  One wave per search.  NEP_E_HIP without a device.
 * nep_hastar_search_host: every pointer names host memory; no GPU, no HIP call.
 * NEP_E_ARG: a null pointer, n_search < 0, a state whose caps are not the handle's.                                          */
int nep_hastar_search(nep_hastar_t* h, int32_t n_search, const int32_t* d_scene, const double* d_start, const double* d_goal,
                      const nep_hastar_state* d_state_in, nep_hastar_result* d_result, double* d_path,
                      const nep_hastar_state* d_state_out, void* stream);
int nep_hastar_search_host(nep_hastar_t* h, int32_t n_search, const int32_t* scene, const double* start, const double* goal,
                           const nep_hastar_state* state_in, nep_hastar_result* result, double* path,
                           const nep_hastar_state* state_out);

/* Waits for `stream` and returns NEP_E_CAP when a search since the last check (device or host) set a flag, else 0; the
 * flags are then cleared.                                                                                                  */
int nep_hastar_check(nep_hastar_t* h, void* stream);

#ifndef NEPTUNE_BACKEND_H
int nep_abi_sizeof(int32_t which);
const char* nep_last_error(void);
#endif

#ifdef __cplusplus
}
#endif
#endif
