/* neptune_mtlp.h — the comparator of the reference's main benchmark (neptune_mtlp_benchmark): mtlp::solveMultiTetherLinearPath
 * (neptune/src/solveMultiLinearPath.cpp, mtlp_node.cpp), the sequential planner of Hert and Lumelsky for several tethered robots
 * in R3 ("Motion Planning in R3 for Multiple Tethered Robots", T-RA 1999), thousands of runs per launch.  C99, self-contained:
 * it includes no other header of this library.  A handle of its own; nothing here reads or changes a nep_batch_t.
 *
 * A run takes N bases and N start/goal pairs and gives the N x N order graph and, per robot, a 3-D grid A* path that avoids the
 * other robots' cable lines.  The rules are the reference's as written (DESIGN.md section 40 lists them):
 *   - the function returns before its motion profile, and the convex-hull branch cannot be selected: neither is built;
 *   - the order graph is the identity OR-ed with what both ordered visits of a pair set, the else-if chains as written;
 *   - THE ORDER OF THE ROBOTS IS ALWAYS 0 .. N-1: the reference's ordering loop starts with has_removal = false and never runs;
 *   - robot i's cable lines: for j < i none when graph(j, i) == 1, else base_j -> goal_j; for j > i base_j -> start_j;
 *   - a 26-connected search without a bounds test (a neighbour off the grid is an ordinary node; only a centre above the
 *     un-rounded goal height is skipped), the float 2-norm step cost, libstdc++'s heap under CompareCost with in-place updates
 *     that do not re-order it, a pool that ends an expansion when it is full, the goal test by index at the pop.
 *
 * The reference's geometric tests are CGAL do_intersect on an exact-predicates kernel: the verdict of the closed point sets.
 * Here every test is a double evaluation with a proven error bound (2^-49 times the sum of the absolute monomials: at most 8
 * roundings lie on any path from an input to the value) and, where that cannot decide a sign, fixed-width integer arithmetic
 * (192, 256 and 384 bits) on the inputs scaled by 2^60.  THE EXACT PATH'S DOMAIN: every coordinate of a base, start or goal is a
 * finite double of magnitude <= NEP_MTLP_MAX_COORD that is a multiple of 2^-60; a run with a value outside it is flagged STATE
 * and not searched.  The configuration's resolution (>= 2^-7), bounds and radius are held to the same domain by nep_mtlp_create,
 * which also refuses a pool that could carry a search to a cell centre beyond 2^20 in magnitude; with that every cell centre is
 * a multiple of 2^-60 too and every intermediate integer fits its width.
 *
 * Two readings CGAL would have decided and this library had to: a triangle whose three points are collinear (a CGAL
 * precondition that release builds do not check) is the closed hull of its points, counted in n_degenerate and flagged DEGEN;
 * the robot's sphere is the ball (distance <= radius), and n_ball_only counts the tests a surface reading would answer
 * differently (a cable line wholly inside the ball).
 *
 * The device form (nep_mtlp_solve: one lane per ordered pair for the graph, one wave per (run, robot) for the searches) and the
 * host form (nep_mtlp_solve_host, no HIP call) are one rule set compiled twice (neptune_amd/csrc/mtlp_common.h) and agree on
 * every output byte.                                                                                                        */
#ifndef NEPTUNE_MTLP_H_
#define NEPTUNE_MTLP_H_

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

/* nep_mtlp_result.flags:
 *   PATH   the path has more than path_cap points; the first path_cap are returned
 *   STATE  the run had an input outside the exact path's domain: status -1, nothing searched, the run's status is NEP_E_STATE
 *          and its graph is zero
 *   DEGEN  the search met a collinear triangle (n_degenerate > 0); nep_mtlp_check does not treat it as an error            */
#define NEP_MTLP_FLAG_PATH 1
#define NEP_MTLP_FLAG_STATE 2
#define NEP_MTLP_FLAG_DEGEN 4

#define NEP_MTLP_MAX_COORD 100000.0 /* |x| of every input coordinate */
#define NEP_MTLP_MAX_ROBOTS 64

/* nep_abi_sizeof(35): 88 bytes.  The reference's set-up (mtlp_node.cpp:280-323): resolution = a_star_fraction_voxel_size (not
 * doubled), the world's bounds, radius = drone_radius, bias = 1.1.  max_nodes = 0 takes the reference's pool, GLX * GLY * GLZ.
 * max_pops ends a search at the top of its loop with status 0; the reference has no such limit, the device needs one.      */
typedef struct nep_mtlp_cfg {
  double resolution, x_min, x_max, y_min, y_max, z_min, z_max, radius, bias;
  int32_t n_robots, max_nodes, max_pops, path_cap;
} nep_mtlp_cfg;

/* nep_abi_sizeof(36): 48 bytes.  nodes_used is node_used_num_, g_cells the terminal node's gScore.  n_updates: open nodes
 * overwritten in place.  n_degenerate: neighbours whose swept triangle (base, neighbour centre, current point) was collinear.
 * n_ball_only: (neighbour, cable line) tests in which the line lay wholly inside the open ball.  Without success n_path and
 * g_cells are 0.                                                                                                          */
typedef struct nep_mtlp_result {
  int32_t status;                 /* 1 reached, 0 budget of pops spent, -1 open list empty (or STATE) */
  int32_t n_path, nodes_used, pops, n_updates, flags;
  int64_t n_degenerate, n_ball_only;
  double g_cells;
} nep_mtlp_result;

typedef struct nep_mtlp nep_mtlp_t;

/* No HIP call: a handle serves the host form on a machine without a GPU.  NULL (and nep_last_error) on a bad configuration:
 * a value outside the domain above, a bias that is not finite and positive, a grid without cells, n_robots outside
 * 1 .. NEP_MTLP_MAX_ROBOTS, path_cap < 1, max_nodes < 0, max_pops <= 0 (there is no unbounded device search).              */
nep_mtlp_t* nep_mtlp_create(const nep_mtlp_cfg* cfg);
void nep_mtlp_destroy(nep_mtlp_t* h);

/* Bytes of working memory one search takes (nodes of 32 bytes, heap, node table, cable lines).                             */
int64_t nep_mtlp_search_bytes(const nep_mtlp_t* h);

/* n_runs runs of N = n_robots robots.  Run r reads bases[r] ([N][3]) and start_goal[r] ([N][2][3]: start, then goal) and writes
 * graph[r] ([N][N] int32, row-major: graph(i, j) is graph[r][i][j]), run_status[r] (1, or NEP_E_STATE), result[r][i],
 * and path[r][i] ([path_cap][3], rows beyond n_path zero: the un-rounded start first, the goal's cell centre last).
 *
 * nep_mtlp_solve: every pointer names device memory.  Asynchronous on `stream`.  The first call (and the first one with more
 * runs than any before) allocates and must be eager; later calls allocate nothing and are capturable.  NEP_E_HIP without a
 * device.  nep_mtlp_solve_host: every pointer names host memory; no GPU, no HIP call.  NEP_E_ARG: a null pointer, n_runs < 0. */
int nep_mtlp_solve(nep_mtlp_t* h, int32_t n_runs, const double* d_bases, const double* d_start_goal, int32_t* d_graph,
                   int32_t* d_run_status, nep_mtlp_result* d_result, double* d_path, void* stream);
int nep_mtlp_solve_host(nep_mtlp_t* h, int32_t n_runs, const double* bases, const double* start_goal, int32_t* graph,
                        int32_t* run_status, nep_mtlp_result* result, double* path);

/* Waits for `stream` and returns NEP_E_CAP when a search since the last check (device or host) set PATH or STATE, else 0; the
 * flags are then cleared.  DEGEN is not an error.                                                                          */
int nep_mtlp_check(nep_mtlp_t* h, void* stream);

/* The bases of the reference's circle_init_bases (mtlp_node.cpp:295-313) into out[n][3]: its float cosf / sinf and its
 * constants 3.1415927 and 1.571.  Host only.  NEP_E_ARG on n < 1 or a null pointer.                                       */
int nep_mtlp_circle_bases(int32_t n, double* out);

/* Debug: the three exact predicates on n records of 16 doubles each, verdict[n] (0 / 1) and exact[n] (how many sign
 * evaluations of the record fell through the filter to the integer path).
 *   which 0  segment/triangle in 3-D: p, q, a, b, c                       (15 doubles)
 *   which 1  segment/segment in 2-D: p, q, u, v as (x, y, ignored)        (12 doubles)
 *   which 2  ball/segment: centre, p, q, radius squared; verdict bit 0 is the ball's, bit 1 "wholly inside" (10 doubles)
 * Values must lie in the domain (magnitude <= 2^20, multiples of 2^-60; the radius squared a multiple of 2^-120).
 * _host: host memory, no HIP call.  _device: device memory, asynchronous on `stream`.                                      */
int nep_mtlp_predicates_host(int32_t which, int32_t n, const double* in, int32_t* verdict, int32_t* exact);
int nep_mtlp_predicates_device(int32_t which, int32_t n, const double* d_in, int32_t* d_verdict, int32_t* d_exact, void* stream);

#ifndef NEPTUNE_BACKEND_H
int nep_abi_sizeof(int32_t which);
const char* nep_last_error(void);
#endif

#ifdef __cplusplus
}
#endif
#endif
