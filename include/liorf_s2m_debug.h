/*
 * liorf_s2m_debug.h — diagnostic and benchmark entry points of libliorf_s2m.so.
 *
 * NOT part of the drop-in boundary (include/liorf_s2m.h is): nothing a mapOptimization node binds lives here.  These are
 * what the repository's own tools and tests use to look inside the registration path - per-launch timing of the
 * registration kernel, per-wave stage stamps, the device's sinf / cosf / atanf arithmetic, worklist statistics - and the
 * list of environment switches the library reads at s2m_create for A/B experiments.  They may change between rounds.
 * The observation hooks (s2m_debug_device_*, s2m_debug_lm_rows, s2m_debug_lm_close, s2m_debug_icp_*, s2m_debug_pg_*) run the product's own
 * kernels on given inputs and hand back what a stage wrote, so that tests can hold a stage against a reference of its own.
 *
 * Environment switches (all optional; defaults are what bench.py measures):
 *   S2M_NO_GRAPH=1         plain launches instead of the captured loop graph
 *   S2M_NO_FUSE=1          one k_finalize per iteration instead of closing iterations in the next launch's prologue
 *   S2M_FUSE_MAX=n         largest grid (workgroups x slots) whose iterations are closed in the prologue (512)
 *   S2M_SEGMENT=n          launches in the first range of an early-exit loop (8; 0 = the whole loop in one piece)
 *   S2M_DENSITY_RAW=n      box points above which a wave asks for a finer cut before launch 0 (320; 0 = off)
 *   S2M_BIG_BLOCKS=0       8-wave workgroups whatever the scan size
 *   S2M_SPLIT=0|1|2        fused kernel always / certify + search always / late split in lockstep batches (default)
 *   S2M_SPLIT_FROM=n, S2M_SEARCH_GRID=n, S2M_CLOSE_IN_SEARCH=1, S2M_LEAN=0, S2M_LOCKSTEP=0, S2M_BATCH_MINW=n, S2M_BATCH_ENTRIES=n
 *                          shape of the batch loop (liorf_amd/csrc/s2m_context.hpp, s2m_context::Tuning)
 *   S2M_ABLATE=bits        switch tiers / search paths off (tests): 1 no certificates, 2 no re-measuring, 16 ignore the prior in
 *                          the search, 32 ignore the plane cache, 64 no tiles (lanes served one by one), 128 tiles for any lane count
 *   S2M_TUNE=a,b,c,d       experiment thresholds (s2m_types.h, DevCtx::tune)
 */
#ifndef LIORF_S2M_DEBUG_H
#define LIORF_S2M_DEBUG_H

#include "liorf_s2m.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Observation hook: sinf / cosf (and atanf when `a` is not NULL) of n host floats as the device computes them -
 * sin/cos when it rebuilds the transform between LM iterations, atan in the ScanContext sector angle. They follow
 * the arithmetic of glibc's sinf / cosf / atanf, so that the device gives what the reference's host libm gives. */
int  s2m_debug_device_trig(s2m_handle h, const float* x, size_t n, float* s, float* c, float* a);
/* Diagnostics: workgroups the certify kernels of the last collected loop handed to the search kernel (slot < 0: the handle's own
 * loop; slot >= 0: that scan slot of the last batch). */
int  s2m_debug_deferred(s2m_handle h, int slot);
/* Benchmark helper: runs `reps` complete LM loops (max_iter iterations, early exit as
 * configured, each loop starting like a fresh scan) on the resident scan + map with plain
 * launches and a HIP-event pair on the handle's stream around every launch of the
 * per-iteration registration kernel (k_register: kNN + plane + Jacobian + block reduction);
 * returns the mean duration of those launches in ms. */
int  s2m_time_iteration_kernel(s2m_handle h, const float pose[6], int reps, float* ms_per_launch);
/* Same measurement, reported per LM iteration: ms_per_iter[it] = mean duration of launch `it` of the
 * loop over `reps` loops (cap >= max_iter entries). The first launches of a scan search without a prior
 * and cost more than the steady state. */
int  s2m_time_iterations(s2m_handle h, const float pose[6], int reps, float* ms_per_iter, int cap);

/* Benchmark helper: mean duration (microseconds) of a k_register launch over `reps` whole LM loops as the fused loop issues them,
 * measured with HIP events on the handle's stream around launch 0, launch 1, the run of back-to-back launches 2 .. max_iter-2 and
 * the last launch - four event pairs per loop instead of max_iter, so the event packets do not break up the back-to-back dispatch
 * (the gaps between consecutive launches are part of the figure). */
int  s2m_time_loop_launches(s2m_handle h, const float pose[6], int reps, float* us_per_launch);

/* Diagnostics: a full loop from `pose` (early_exit must be off), then `reps` back-to-back replays of its last registration
 * launch in the state the loop ended in; solve_prev != 0 closes the iteration before it in the launch's prologue each time
 * (the steady launch of the fused loop), 0 only rebuilds the transform.  Mean microseconds per replayed launch, gaps included. */
int  s2m_debug_time_steady(s2m_handle h, const float pose[6], int reps, int solve_prev, float* us_per_launch);

/* Diagnostics: `launches` > 0: that many k_register passes at `pose`, the last one recorded (1 = the pass
 * that inherits its prior from whatever ran before, 3 = steady state at this pose). `launches` < 0: a real LM
 * loop from `pose` exactly as s2m_optimize issues it, of which launch number N = -launches - 1 is recorded
 * (N = 0: the first launch of a scan, searching without a prior), including the fused close of the
 * iteration before it. Per wave (up to 64 locality-sorted scan points) S2M_PROF_WORDS words:
 * [0..3] wall clock (100 MHz) at start / after the search / after plane+Jacobian / at end; [4] search path
 * (1 LDS tile, 2 gather), [5] box rows, [6] points visited, [7] raw points; [8..12] ticks spent in
 * prior+box / row marking, points in the wave, staging, search; [13..15] path details; [16..22] wall clock
 * of the fused LM close: entry, partial sums reduced, normal equations, QR solved, update done, barrier
 * passed, transform built (0 when the launch closes nothing). Returns the number of waves written. */
#define S2M_PROF_WORDS 32
int  s2m_debug_wave_profile(s2m_handle h, const float pose[6], int launches, uint64_t* out, size_t cap_waves);

/* Observation hook: hypotf of n pairs of host floats as the device computes it in the Jacobi rotations of the
 * iteration-0 degeneracy analysis (cv::eigen): glibc's arithmetic, so that the device gives what the host's libm gives. */
int  s2m_debug_device_hypot(s2m_handle h, const float* x, const float* y, size_t n, float* r);

/* Observation hook: closes ONE LM iteration on given partial sums - everything of LMOptimization() behind the
 * per-point work (:1177-1292): second stage of the reduction, fp32 matAtA / matAtB, the QR solve, at iteration 0 the
 * degeneracy analysis, the projection, the pose update and the convergence test - and returns what the close wrote.
 *   rows     n_rows x 28 doubles in the layout of a workgroup's partial row: 21 upper-triangular JtJ sums (row-major),
 *            6 Jtr sums, the correspondence count. They go to the slot of parity iter & 1; the other active rows of
 *            that slot are zero; every row the close must not read (inactive rows, the whole other slot) is NaN.
 *            n_rows larger than the number of workgroups the resident scan's wave table needs: S2M_ERR_INVALID_ARG.
 *   pose0    the pose iteration `iter` ran with; degen_in / matP_in: isDegenerate and matP as left by iteration 0
 *   form 0   the stand-alone close k_finalize(iter) (iter == 0: with the degeneracy analysis)
 *   form 1   the prologue of the fused registration launch iter + 1 (iter >= 1), in the workgroup shape of the resident
 *            scan; the registration pass behind the prologue runs on the resident scan and map at the pose the close
 *            produced, its own results are ignored
 * Uses the handle's current parameters (min_corr, eig_thresh, conv_deg, conv_cm, early_exit, max_iter); iter in
 * 0 .. max_iter-1. Needs a resident scan and map (S2M_ERR_NO_SCAN). No kernel exists for the hook: it prepares the
 * state and launches what the loop launches. The state that persists from scan to scan (isDegenerate, matP) is not
 * touched: the next registration on the handle is the one a handle that never saw the hook computes. */
typedef struct s2m_debug_lm_close_out {
    float   AtA[36], AtB[6];   /* matAtA, matAtB as stored (fp32)                                  */
    int32_t n_sel_last;
    s2m_iter_trace trace;      /* the record of iteration `iter`                                   */
    float   pose[6];           /* transformTobeMapped after the close                              */
    float   pose_next[6];      /* the pose launch iter + 1 runs with (NaN: the close wrote none)   */
    int32_t iters_run, converged, done, stalled, is_degenerate;
    int32_t n_rows_active;     /* rows the close read: the workgroups the resident scan's wave table needs */
    float   matP[36];
} s2m_debug_lm_close_out;
int  s2m_debug_lm_close(s2m_handle h, int form, int iter, const double* rows, int n_rows, const float pose0[6],
                        int degen_in, const float matP_in[36], s2m_debug_lm_close_out* out);
/* The argument checks of s2m_debug_lm_close that need no handle and no GPU: S2M_OK or S2M_ERR_INVALID_ARG (a null pointer
 * - rows may be null when n_rows == 0 -, n_rows < 0, form outside {0, 1}, iter outside 0 .. max_iter-1, form 1 at iter 0). */
int  s2m_debug_lm_close_check_args(int form, int iter, int max_iter, const double* rows, int n_rows, const float pose0[6],
                                   const float matP_in[36], const s2m_debug_lm_close_out* out);

/* Observation hook: the partial rows ONE registration launch wrote - the stage between the plane fit and the close:
 * residual and weight, the Jacobian row (:1216-1234), the 28 products, the wave reduction, the workgroup's row.
 *   launch 0      what s2m_normal_eq queues in front of its k_finalize: the state upload at `pose`, then the first launch of
 *                 a scan (trig from the host's libm)
 *   launch N > 0  a real loop from `pose` exactly as s2m_optimize issues it (density re-split, R0 F0 R1 R2' ..., or certify +
 *                 search under S2M_SPLIT=1, one k_finalize per iteration under S2M_NO_FUSE=1) up to and including launch N,
 *                 nothing behind it. early_exit must be off and N < max_iter (S2M_ERR_INVALID_ARG otherwise)
 *   rows          takes n_rows_active x 28 doubles from slot launch & 1 of the partial rows (layout as s2m_debug_lm_close);
 *                 cap_rows smaller than n_rows_active: S2M_ERR_INVALID_ARG, with `out` filled in
 *   wave_table    optional: the {first point, count} entries launch N read, n_waves of them (room for the table's capacity,
 *                 see s2m_debug_scan_prep). Workgroup b's row sums the entries e with e % n_rows_active == b.
 * S2M_ERR_INVALID_ARG while an optimise is pending or on a scan slot of a batch; needs a resident scan and map
 * (S2M_ERR_NO_SCAN). No kernel exists for the hook: it queues what the product queues and copies back what the launch wrote.
 * Afterwards the handle is where s2m_set_scan left it - isDegenerate and matP that persist from scan to scan untouched, a
 * density re-split the hook's loop consumed pending again - so the next registration on the handle is the one a handle that
 * never saw the hook computes. */
typedef struct s2m_debug_lm_rows_out {
    int32_t n_rows_active;     /* workgroups the wave table needs: entries over waves per workgroup, rounded up, the grid at most */
    int32_t wpb, nblocks;      /* waves per workgroup and grid of the registration kernels              */
    int32_t n_waves;           /* wave-table entries launch N read                                      */
    float   pose_used[6];      /* the pose launch N ran with (N = 0: `pose`)                            */
    int32_t done;              /* the loop's done flag after the launches before N                      */
} s2m_debug_lm_rows_out;
int  s2m_debug_lm_rows(s2m_handle h, const float pose[6], int launch, double* rows, int cap_rows, s2m_debug_lm_rows_out* out,
                       int32_t* wave_table);
/* The argument checks of s2m_debug_lm_rows that need no handle and no GPU: S2M_OK or S2M_ERR_INVALID_ARG (a null pose or
 * out, rows null with cap_rows > 0, cap_rows < 0, launch outside 0 .. max_iter-1, launch > 0 with early_exit on). */
int  s2m_debug_lm_rows_check_args(const float pose[6], int launch, int max_iter, int early_exit, const double* rows, int cap_rows,
                                  const s2m_debug_lm_rows_out* out);

/* Observation hook: the preparation of the RESIDENT single scan, run again by either chain, and what it left.
 *   chain  S2M_DEBUG_PREP_NEW     what s2m_set_scan launches: k_polar_count, k_polar_prefix, the scatter with the cell scan in it,
 *                                 k_chunk_parts; with a pose the density wishes chunk by chunk with the state upload in the same
 *                                 launch (k_wave_density_state, as s2m_optimize_launch), then k_chunk_table_density
 *          S2M_DEBUG_PREP_LEGACY  the six kernels a scan slot of a batch runs (k_polar_scan and k_scatter_scan apart, k_chunk_table
 *                                 at once); with a pose the state upload, k_wave_density over that table, k_chunk_table_density
 *          S2M_DEBUG_PREP_READ    runs nothing: the buffers as they are
 *   pose   NULL: the ordering only - the handle is left as s2m_set_scan leaves it (density re-split pending; after the legacy
 *          chain with the extent-only table in place, after the new one with that table still to be built on demand -
 *          asking for wave_table or n_waves is such a demand).
 * Outputs, each optional: qperm n; qxyz 3 n (x, then y, then z, sorted order); chunk_parts and chunk_factor one per 64-point
 * chunk (chunk_factor as the density kernel left it, BEFORE k_chunk_table_density consumed it; without a pose as it is);
 * wave_table 2 per entry {first point, count}, room for the scan's table capacity (n/64 rounded up, times 12, plus 64 is
 * enough); *n_waves the entries in use (-1 with READ while no table has been built). The source of the scan must still be
 * readable (a host scan is: the library keeps its copy). The certificates of the scan are reset as by s2m_set_scan. */
#define S2M_DEBUG_PREP_READ   (-1)
#define S2M_DEBUG_PREP_NEW    0
#define S2M_DEBUG_PREP_LEGACY 1
int  s2m_debug_scan_prep(s2m_handle h, int32_t chain, const float pose[6], int32_t* qperm, float* qxyz, int32_t* chunk_parts,
                         int32_t* chunk_factor, int32_t* wave_table, int32_t* n_waves);

/* ---- the device loop of the ICP alignment (what s2m_loop_*_launch queues) -------------------------------------------
 * S2M_ICP_RANGE: iterations queued at a time; between two ranges the host looks at the state block once. */
#define S2M_ICP_RANGE 8
/* Observation hook: one nearest-neighbour search of every src point among the tgt points (host records, x y z at byte 0 / 4 / 8).
 * mode 0 = k_icp_nn, the tiled brute force of s2m_icp_align; mode 1 = the search of the device loop: the uniform grid over the
 * target with its brute-force fallback (after s2m_debug_icp_tuning(.., use_grid = 0): the brute force over every source). keys[i] = (fp32 d2 bits << 32) | target index with d2 = (dx*dx + dy*dy) + dz*dz, the
 * minimum over all finite targets (equal distances: the lower index); ~0 = no match (a non-finite source, no finite target).
 * *n_fallback: sources the grid handed to the brute force (0 in mode 0). The grid's cell edge is that of the default
 * icp_leaf (s2m_loop_default_params). S2M_ERR_BUSY while a launched closure is pending. */
int  s2m_debug_icp_nearest(s2m_handle h, const void* src, size_t n_src, const void* tgt, size_t n_tgt, size_t stride_bytes, int32_t mode,
                           uint64_t* keys, int32_t* n_fallback);
/* The same search `reps` times between HIP events on the loop stream: *us_search = microseconds per search, *us_build = the
 * grid's construction (box, counts, scan, scatter; 0 in mode 0). reps == 0 is s2m_debug_icp_nearest. keys may be NULL. */
int  s2m_debug_icp_time_nearest(s2m_handle h, const void* src, size_t n_src, const void* tgt, size_t n_tgt, size_t stride_bytes, int32_t mode,
                                int32_t reps, uint64_t* keys, int32_t* n_fallback, float* us_build, float* us_search);
/* s2m_icp_align's alignment by the device loop, synchronously on the loop stream and with no size gate: the grid search, every
 * iteration closed on the device by the host loop's own source, ranges of S2M_ICP_RANGE iterations, the fitness pass. The
 * result is bit for bit that of s2m_icp_align. */
int  s2m_debug_icp_align_device(s2m_handle h, const void* src, size_t n_src, const void* tgt, size_t n_tgt, size_t stride_bytes,
                                const s2m_icp_params* p /* NULL = defaults */, s2m_icp_result* out);
/* The same for one source against n_cand <= S2M_LOOP_MAX_CANDIDATES targets, aligned in lockstep by the slotted device loop
 * (what s2m_loop_verify_launch queues): tgts[i] holds n_tgts[i] records of the source's stride, out takes n_cand results.
 * out[i] is bit for bit s2m_icp_align(src, tgts[i]); the same target may be listed twice. */
int  s2m_debug_icp_align_many_device(s2m_handle h, const void* src, size_t n_src, const void* const* tgts, const size_t* n_tgts, int32_t n_cand,
                                     size_t stride_bytes, const s2m_icp_params* p /* NULL = defaults */, s2m_icp_result* out);
/* The same with a guess per target (guesses: n_cand row-major 4x4 back to back, or NULL for none): every slot of the device loop
 * owns its moving copy of the source, loaded through its own guess. out[i] is bit for bit s2m_icp_align_guess(src, tgts[i],
 * guesses + 16 * i), whatever the other slots hold. A guess s2m_icp_align_guess rejects is S2M_ERR_INVALID_ARG. */
int  s2m_debug_icp_align_guess_many_device(s2m_handle h, const void* src, size_t n_src, const void* const* tgts, const size_t* n_tgts,
                                           const float* guesses, int32_t n_cand, size_t stride_bytes,
                                           const s2m_icp_params* p /* NULL = defaults */, s2m_icp_result* out);
/* Experiment switch of the device loop's search for the launches and debug calls that follow: the cell edge in units of
 * icp_leaf (0 = built in), the largest shell radius searched before a point goes to the brute force (0 = built in), and
 * use_grid (0 = brute force only, 1 = grid, < 0 = built in). */
int  s2m_debug_icp_tuning(s2m_handle h, float cell_in_leaves, int32_t shell_cap, int32_t use_grid);
/* Observation hook: the uniform grids the device loop builds over n_cand = 1 .. S2M_LOOP_MAX_CANDIDATES host targets (non-empty,
 * records of one stride), laid out in slots as s2m_debug_icp_align_many_device lays them out and built by the loop's own
 * launches (block reset, box, shape, counts, scan, scatter) - no source, no search, and built whatever use_grid says. The cell
 * edge asked for is that of the other debug calls (the default icp_leaf times the edge of s2m_debug_icp_tuning).
 * out[i]: the grid of tgts[i] as the device holds it - origin, cell edge and its reciprocal, cells per axis (x fastest), finite
 * targets, and usable = 0 where no grid was built (an extent that overflows fp32; every source then goes to the brute force,
 * the targets are not counted and n_fin is 1 where one is finite).
 * cell_start, cell_end, order: each may be NULL, and so may each entry. cell_start[i] / cell_end[i] (room for
 * S2M_DEBUG_ICP_GRID_MAX_CELLS) take, per cell, the range of the cell's targets in the slot's sorted targets; order[i] (room for
 * n_tgts[i]) the index in tgts[i] of each of the n_fin sorted entries. Nothing is written to them for a target without a grid.
 * S2M_ERR_BUSY while a launched closure is pending. s2m_debug_icp_grid_check_args: the argument checks on their own (host
 * code, no handle, no GPU). */
#define S2M_DEBUG_ICP_GRID_MAX_CELLS 262144
typedef struct s2m_debug_icp_grid_out {
    float   lo[3];
    float   cell, inv;
    int32_t n[3];
    int32_t n_fin, usable;
} s2m_debug_icp_grid_out;
int  s2m_debug_icp_grid_check_args(const void* const* tgts, const size_t* n_tgts, int32_t n_cand, size_t stride_bytes, const s2m_debug_icp_grid_out* out);
int  s2m_debug_icp_grid(s2m_handle h, const void* const* tgts, const size_t* n_tgts, int32_t n_cand, size_t stride_bytes,
                        s2m_debug_icp_grid_out* out, int32_t* const* cell_start, int32_t* const* cell_end, int32_t* const* order);

/* ---- the tail rule of a launched pose-graph optimise (s2m_pg_optimize_launch) ------------------------------------------
 * Host code, no handle, no GPU, and the code the library runs when a launched optimise delivers its result: states are 12
 * doubles (R row-major, then t); with D = a_now a_launch^-1, X <- D X, i.e. D_R = A'_R A_R^T, D_t = A'_t - D_R A_t,
 * X_R <- D_R X_R, X_t <- D_R X_t + D_t, every three-term sum taken as ((a0 b0 + a1 b1) + a2 b2) with no fused products.
 * S2M_OK, or S2M_ERR_INVALID_ARG for a null pointer. */
int  s2m_debug_pg_rebase(const double a_launch[12], const double a_now[12], double X[12]);

/* ---- observation hooks of the pose graph's stages (liorf_amd/csrc/s2m_pose_graph.hip) ----------------
 * What s2m_pg_optimize and the marginals compute between their inputs and their results, one stage at a time. No kernel exists
 * for a hook: each prepares the device tables as an optimise does and queues the launches the product queues, on the work
 * arrays that every optimise and marginal rewrites before reading them, so that afterwards the graph is in the state a handle
 * that never saw the hook holds (s2m_debug_pg_set_estimate excepted: it is s2m_pg_set_initial in fp64). Every hook returns
 * S2M_ERR_BUSY while a launched optimise is pending. States are 12 doubles (R row-major, then t), tangent vectors 6 doubles
 * per key (rotation, translation). The chain is the first prior on key 0 and, per i, the first plain between i -> i+1, indexed
 * by key; the n_extra = n_factors - n_variables extra factors keep the order in which they were added.
 *
 * s2m_debug_pg_set_estimate: the estimate of `key` (0..N, N appends) from 12 doubles, past the float xyzrpy of
 * s2m_pg_set_initial. The values are taken as they are - not orthonormalised, not checked for finiteness. */
int  s2m_debug_pg_set_estimate(s2m_handle h, int32_t key, const double X[12]);
/* Linearises at the current estimates (pg_linearize) and reads back, each array optional (NULL skips it): rc n x 6, Binv and
 * Aof n x 36 (row-major 6x6; Aof[i] = whitened Jacobian of chain factor i with respect to key i-1, zero at i = 0), Ji, Jj
 * n_extra x 36, rx n_extra x 6, ferr and fw n + n_extra (chain first), the error sum and the minimum robust weight.
 * n_variables and n_extra must be the graph's (S2M_ERR_INVALID_ARG otherwise). */
int  s2m_debug_pg_linearize(s2m_handle h, int32_t n_variables, int32_t n_extra, double* rc, double* Binv, double* Aof, double* Ji, double* Jj,
                            double* rx, double* ferr, double* fw, double* err, double* wmin);
/* Linearises at the current estimates and applies one operator of that linearisation to host vectors. With J_c the chain's
 * whitened Jacobian, J_x the extra factors' and K = J_x J_c^-1:
 *   S2M_DEBUG_PG_FWD  out = J_c^-1 in   (6n -> 6n, the forward blocked scan)
 *   S2M_DEBUG_PG_BWD  out = J_c^-T in   (6n -> 6n, the backward blocked scan)
 *   S2M_DEBUG_PG_K    out = K in        (6n -> 6 n_extra, the forward scan, then k_pg_extra_u)
 *   S2M_DEBUG_PG_KT   out = K^T in      (6 n_extra -> 6n, k_pg_extra_gather, then the backward scan)
 * cols == 0: the single form, one vector. cols = 1 .. S2M_PG_BLOCK_COLUMNS: the block form, `cols` vectors one after the
 * other in `in` and in `out`. K and K^T need an extra factor. */
#define S2M_DEBUG_PG_FWD 0
#define S2M_DEBUG_PG_BWD 1
#define S2M_DEBUG_PG_K   2
#define S2M_DEBUG_PG_KT  3
int  s2m_debug_pg_apply(s2m_handle h, int32_t op, int32_t cols, const double* in, double* out);
/* The argument checks of s2m_debug_pg_apply that need no handle and no GPU: S2M_OK or S2M_ERR_INVALID_ARG (an empty graph,
 * op outside 0..3, K or K^T without an extra factor, cols outside 0 .. S2M_PG_BLOCK_COLUMNS, a null array). */
int  s2m_debug_pg_apply_check_args(int32_t n_variables, int32_t n_extra, int32_t op, int32_t cols, const double* in, const double* out);
/* Linearises at the current estimates and runs the CG on (I + K^T K) y = b for the given b, driven as the optimise drives it
 * (single form, cols == 0) or as the marginals' block solve does (cols >= 1, `cols` right-hand sides one after the other):
 * p->cg_rel_tol and p->cg_max_iterations as s2m_pg_optimize reads them (NULL: defaults; without an extra factor one
 * iteration). y: cols x 6n; out[c]: the recurrence's |r|^2, |b|^2, the iterations run and the stop flag of column c. */
typedef struct s2m_debug_pg_cg_out {
    double  rr, bb;
    int32_t iters, stop;
} s2m_debug_pg_cg_out;
int  s2m_debug_pg_cg(s2m_handle h, const s2m_pg_params* p, int32_t cols, const double* b, double* y, s2m_debug_pg_cg_out* out);
/* X[12 k ..] = estimate of key k (+) delta[6 k ..] through k_pg_retract; the estimates stay. n_variables must be the graph's. */
int  s2m_debug_pg_retract(s2m_handle h, int32_t n_variables, const double* delta, double* X);

/* ---- saving and loading a session: the staging chunk and the state a load rebuilds ----
 * s2m_debug_session_chunk: the bytes of one staging chunk of s2m_session_save / s2m_session_load (default 16 MiB; 0 restores
 *   it): a multiple of 32, at least 1024, so that a store of a few dozen small keys crosses many chunk edges. The blob does
 *   not depend on it.
 * s2m_debug_sc_keys: the fp32 ring keys (count x 20) and fp64 sector keys (count x 60) of descriptors first .. first+count-1
 *   as the store holds them.
 * s2m_debug_kf_frame: key `key`'s cached transform in the library's host mirror and in the device's frame table, its device
 *   position (x, y, z, 0) and the point count of the device's entry. */
int  s2m_debug_session_chunk(s2m_handle h, size_t chunk_bytes);
int  s2m_debug_sc_keys(s2m_handle h, int32_t first, int32_t count, float* ring, double* sector);
int  s2m_debug_kf_frame(s2m_handle h, int32_t key, float T_host[12], float T_device[12], float pos_device[4], int32_t* n_device);

/* ---- the key-frame selection stage by stage ----
 * s2m_debug_kf_select_last: what the most recent key-frame selection on the handle (s2m_extract_surrounding,
 *   s2m_extract_surrounding_at, s2m_global_map) left in device memory, copied out as it stands - no kernel runs. The caller
 *   sets the capacities and the four pointers; the hook fills the rest.
 *     path: S2M_DEBUG_KF_NARROW - a store of up to 4 096 keys, everything in one workgroup; S2M_DEBUG_KF_PRE - a larger store,
 *       the radius search over the whole grid and up to 4 096 candidates handed to that workgroup; S2M_DEBUG_KF_WIDE - more
 *       candidates, sorted and filtered by the device-wide radix passes. A note the host takes where it decides.
 *     n_cand, n_cent, n_frames, n_points: radius candidates (b), centroids of the key-pose filter (c), entries of the frame table
 *       after (f), records of the concatenated cloud.
 *     cent, nn: the first min(n_cent, cent_cap) centroids (x, y, z each) in ascending voxel index and the nearest key of each (d).
 *     keys, offsets: the first min(n_frames, frames_cap) keys of the frame table, and - when frames_cap >= n_frames - its
 *       n_frames + 1 offsets (offsets has room for frames_cap + 1 entries).
 *   S2M_ERR_INVALID_ARG for a null handle or out, or a null array with a capacity above 0; S2M_ERR_NO_SCAN before the first
 *   selection on the handle (one on an empty store does not count); S2M_ERR_CAPACITY, with the counts and what fits written,
 *   when n_cent > cent_cap or n_frames > frames_cap.
 * s2m_debug_kf_select_last_check_args: the argument checks on their own (host code, no handle, no GPU). */
#define S2M_DEBUG_KF_NARROW 0
#define S2M_DEBUG_KF_PRE    1
#define S2M_DEBUG_KF_WIDE   2
typedef struct s2m_debug_kf_select_out {
    int32_t  path;
    int32_t  n_cand, n_cent, n_frames;
    int64_t  n_points;
    size_t   cent_cap;      /* in: room in cent (x 3 floats) and nn */
    float*   cent;
    int32_t* nn;
    size_t   frames_cap;    /* in: room in keys; offsets holds frames_cap + 1 */
    int32_t* keys;
    int32_t* offsets;
} s2m_debug_kf_select_out;
int  s2m_debug_kf_select_last_check_args(const s2m_debug_kf_select_out* out);
int  s2m_debug_kf_select_last(s2m_handle h, s2m_debug_kf_select_out* out);

/* ---- the many-query form of the place query: its passes and the shape of its kernel ----
 * s2m_debug_sc_query_many_pass: at most this many queries per pass of s2m_sc_query_keys / _descriptors (0 restores the
 *   default, as many as the 64 MiB scratch bound allows). The rows do not depend on it.
 * s2m_debug_sc_query_many_shape: the stored descriptors a workgroup of k_sc_many_dist holds in LDS (tile_cands) and the
 *   queries it walks past them (block_queries), so that tests can place their sizes at the kernel's edges.
 * s2m_debug_sc_query_many_last: the passes of the handle's last many-query and the device bytes one of them used. */
int  s2m_debug_sc_query_many_pass(s2m_handle h, int32_t queries_per_pass);
int  s2m_debug_sc_query_many_shape(int32_t* tile_cands, int32_t* block_queries);
int  s2m_debug_sc_query_many_last(s2m_handle h, int32_t* passes, size_t* scratch_bytes);

/* ---- the ring-key prefilter of the place query: its passes and the shape of its selection kernel ----
 * s2m_debug_sc_ring_pass: at most this many queries per pass of the s2m_sc_ring_neighbours_* / s2m_sc_query_*_ring calls (0
 *   restores the default, as many as the 64 MiB scratch bound allows, at most 65535). The rows do not depend on it.
 * s2m_debug_sc_ring_shape: the stored ring keys a workgroup of k_sc_ring_select holds in LDS (tile_keys), the queries it walks
 *   past them (block_queries) and the 64-bit words of a query's candidate buffer (buffer_words), so that tests can place their
 *   sizes at the kernel's edges. A workgroup walks every tile of the range: there are no tile groups.
 * s2m_debug_sc_ring_last: the passes of the handle's last ring call and the device bytes one of them used. */
int  s2m_debug_sc_ring_pass(s2m_handle h, int32_t queries_per_pass);
int  s2m_debug_sc_ring_shape(int32_t* tile_keys, int32_t* block_queries, int32_t* buffer_words);
int  s2m_debug_sc_ring_last(s2m_handle h, int32_t* passes, size_t* scratch_bytes);

/* The table form of the device loop (icp_dev_begin / icp_dev_advance of a table set): n_pairs <= S2M_LOOP_MANY_MAX_PAIRS host pairs, each
 * with its own source and target (no size gate) and optionally a guess (guesses: NULL, or n_pairs pointers, each NULL or a
 * row-major 4x4), aligned in lockstep as s2m_debug_icp_align_many_device aligns the slots of one source. out[k] is bit for bit
 * s2m_icp_align(srcs[k], tgts[k]) / s2m_icp_align_guess with guesses[k]; a pair with an empty cloud gives that call's result
 * for it. n_pairs outside 1 .. S2M_LOOP_MANY_MAX_PAIRS is S2M_ERR_INVALID_ARG; S2M_ERR_BUSY while a closure is pending. */
int  s2m_debug_icp_align_pairs_device(s2m_handle h, const void* const* srcs, const size_t* n_srcs, const void* const* tgts,
                                      const size_t* n_tgts, int32_t n_pairs, size_t stride_bytes, const float* const* guesses,
                                      const s2m_icp_params* p, s2m_icp_result* out);
/* Observation hook: the close of one ICP iteration on the device (k_icp_close: Umeyama, the composition of T, PCL's convergence
 * state machine - liorf_amd/csrc/s2m_icp_close.hpp, the source the host loop runs too). No kernel exists for the hook: the
 * n <= S2M_LOOP_MANY_MAX_PAIRS state blocks of the table form take sums[17 k ..] (count, sum d2, sum src 3, sum tgt 3, sum tgt
 * src^T 9 row-major) and the state in[k], k_icp_close is launched once over all of them as an iteration launches it, out[k] is the
 * state it left. p: max_iterations, transformation_epsilon and euclidean_fitness_epsilon are read (NULL = defaults). A state that
 * comes in done comes back untouched. S2M_ERR_BUSY while a launched closure is pending; afterwards the handle is in the
 * state of one that never saw the hook (every alignment lays its blocks out anew). s2m_debug_icp_close_check_args: the
 * argument checks on their own (host code, no handle, no GPU). */
typedef struct s2m_debug_icp_state {
    float   T[16];          /* final_transformation_ so far, row-major */
    float   T_step[16];     /* transformation_ of the iteration closed last */
    double  prev_mse;       /* correspondences_prev_mse_ */
    int32_t it, conv, similar, done;
} s2m_debug_icp_state;
int  s2m_debug_icp_close_check_args(int32_t n, const double* sums, const s2m_debug_icp_state* in, const s2m_icp_params* p,
                                    const s2m_debug_icp_state* out);
int  s2m_debug_icp_close(s2m_handle h, int32_t n, const double* sums, const s2m_debug_icp_state* in, const s2m_icp_params* p /* NULL = defaults */,
                         s2m_debug_icp_state* out);
/* Observation hook: the 17 sums of iteration 0 of n_pairs alignments of host clouds, staged as s2m_debug_icp_align_pairs_device
 * stages them. form S2M_DEBUG_ICP_SUMS_SLOTS: one source (srcs[k] == srcs[0], n_srcs[k] == n_srcs[0]) against n_pairs <=
 * S2M_LOOP_MAX_CANDIDATES targets, laid out, loaded and prepared as the slotted device loop begins; S2M_DEBUG_ICP_SUMS_TABLE:
 * n_pairs <= S2M_LOOP_MANY_MAX_PAIRS pairs as the table form begins. Then one search, k_icp_sums_dev and k_icp_fold_dev exactly as
 * the first iteration queues them - no close, no transform, no guess. Every cloud is non-empty. sums: n_pairs x 17 folded sums
 * (layout as s2m_debug_icp_close takes them) of the correspondences with d2 <= max_correspondence_distance^2; n_rows[k]: the
 * partial rows of alignment k, min(ceil(n_src / 256), 256); parts, keys: NULL, or per alignment NULL or room for 256 x 17 partial
 * sums (n_rows[k] rows are written, in the order they are folded) and for the n_srcs[k] keys of the search (s2m_debug_icp_nearest).
 * S2M_ERR_BUSY while a launched closure is pending. s2m_debug_icp_sums_check_args: the argument checks on their own. */
#define S2M_DEBUG_ICP_SUMS_SLOTS 0
#define S2M_DEBUG_ICP_SUMS_TABLE 1
int  s2m_debug_icp_sums_check_args(const void* const* srcs, const size_t* n_srcs, const void* const* tgts, const size_t* n_tgts, int32_t n_pairs,
                                   size_t stride_bytes, int32_t form, const double* sums, const int32_t* n_rows);
int  s2m_debug_icp_sums(s2m_handle h, const void* const* srcs, const size_t* n_srcs, const void* const* tgts, const size_t* n_tgts, int32_t n_pairs,
                        size_t stride_bytes, int32_t form, double max_correspondence_distance, double* sums, int32_t* n_rows,
                        double* const* parts, uint64_t* const* keys);
/* s2m_loop_verify_many: the pairs of a pass for the calls that follow (0: the default, S2M_LOOP_MANY_MAX_PAIRS; other values are
 * clamped to [S2M_LOOP_MAX_CANDIDATES, S2M_LOOP_MANY_MAX_PAIRS]); what the last call did - its passes, the pairs it aligned, and
 * the bytes the handle holds for the submaps of a pass; and the plan on its own (host only, no handle): first_row_of_pass takes
 * *n_pass + 1 <= m + 1 entries, pass k being rows [first_row_of_pass[k], first_row_of_pass[k + 1]). */
int  s2m_debug_loop_verify_many_pass(s2m_handle h, int32_t pairs_per_pass);
int  s2m_debug_loop_verify_many_last(s2m_handle h, int32_t* passes, int32_t* pairs_aligned, size_t* bytes);
int  s2m_debug_loop_verify_many_plan(const int32_t* n_cand, int32_t m, int32_t pairs_per_pass, int32_t* first_row_of_pass, int32_t* n_pass);

/* ---- the loop detection by position for many keys: its passes and the shape of its kernel ----
 * s2m_debug_loop_detect_pass: at most this many queries per pass of s2m_loop_detect_keys (0 restores the default, as many as
 *   the 64 MiB scratch bound allows). The rows do not depend on it.
 * s2m_debug_loop_detect_shape: the stored keys a workgroup of k_loop_detect_many holds in LDS (tile_keys), the queries it walks
 *   past them (block_queries) and the most store splits of a grid (max_splits), so that tests can place their sizes at the
 *   kernel's edges.
 * s2m_debug_loop_detect_last: the passes of the handle's last s2m_loop_detect_keys and the device bytes one of them used.
 * s2m_debug_loop_detect_splits: at most this many store splits per grid (0 restores the plan's own, which takes more splits the
 *   fewer queries a pass holds). The rows do not depend on it; the benchmark uses it to show what the splits buy. */
int  s2m_debug_loop_detect_pass(s2m_handle h, int32_t queries_per_pass);
int  s2m_debug_loop_detect_splits(s2m_handle h, int32_t max_splits);
int  s2m_debug_loop_detect_shape(int32_t* tile_keys, int32_t* block_queries, int32_t* max_splits);
int  s2m_debug_loop_detect_last(s2m_handle h, int32_t* passes, size_t* scratch_bytes);

/* ---- what a batch issued (s2m_batch_set_scans, s2m_optimize_batch_launch / _collect, s2m_optimize_batch) ----
 * Host only, no kernel and no device memory: every number is noted where the library issues the launch or takes the decision,
 * none is worked out from n_scans afterwards. It proves which path a batch took; the results are held to their bits elsewhere.
 *   n_scans, n_live: the last batch launch's slots, and those of them that ran a loop (the others were skipped, :1297 / :1300).
 *   ctx_launches, init_launches: launches of k_set_ctxs (the slots whose DevCtx block had changed, 8 a launch) and of
 *     k_init_states (the live slots, 12 a launch) by that batch launch.
 *   prep_launches: scan-ordering tables (16 slots each) the s2m_batch_set_scans before that batch launch issued; a table of
 *     empty scans only is not issued. s2m_batch_set_scan / s2m_slot_set_scan do not count here.
 *   ranges_issued: graph launches of the batch, 0 (no live slot), 1, or 2 (early exit on and some slot not done after the
 *     first range; known once the batch is collected).
 *   graph_cached: 1 if every one of them was a graph captured by an earlier batch, 0 if one was captured now (or none issued).
 *   n_loops, loop[]: the lockstep loops of the graph, one per workgroup shape in use (the first two are reported): waves per
 *     workgroup, grid rows (slots), grid columns (workgroups), fused = 1 if the iterations close inside the registration kernel
 *     and 0 if k_finalize closes them, and first_split: the first launch, over the ranges issued, that ran the certify and
 *     the search kernel instead of the fused one (-1: none).
 * S2M_ERR_INVALID_ARG for a null argument. Before the first batch launch everything is 0 (first_split -1). */
typedef struct s2m_debug_batch_loop {
    int32_t wpb, nslots, nblocks, fused, first_split;
} s2m_debug_batch_loop;
typedef struct s2m_debug_batch_last_out {
    int32_t n_scans, n_live;
    int32_t ctx_launches, init_launches, prep_launches;
    int32_t ranges_issued, graph_cached;
    int32_t n_loops;
    s2m_debug_batch_loop loop[2];
} s2m_debug_batch_last_out;
int  s2m_debug_batch_last(s2m_handle h, s2m_debug_batch_last_out* out);

#ifdef __cplusplus
}
#endif
#endif /* LIORF_S2M_DEBUG_H */
