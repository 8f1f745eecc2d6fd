// s2m_pose_graph.hpp — the pose graph's device side (s2m_pose_graph.hip): factor linearisation, the block-bidiagonal chain
// solves as blocked scans, the extra factors' sparse products, the CG vector steps, retraction, error and pose read-out.
// DESIGN.md section 16 has the formulation: with J_c the (square, block lower bidiagonal) whitened Jacobian of the chain
// prior(0), between(0,1), between(1,2), ... and J_x the whitened rows of every other factor, the Gauss-Newton step is
//   delta = J_c^-1 y,   (I + K^T K) y = -(r_c + K^T r_x),   K = J_x J_c^-1,
// solved by CG in y.  J_c is never squared, so the nearly free translation of the whole map is not amplified.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace s2m {

constexpr int kPgGroup = 32;          // elements per group of the blocked scan
constexpr int kPgMaxLevels = 6;       // 32^6 keys
constexpr int kPgDotBlocks = 64;      // workgroups of a dot product's first stage (fixed, so sums are reproducible)
constexpr int kPgThreads = 256;
constexpr int kPgBlockCols = 24;      // right-hand sides one pass of the block solve advances in lockstep (a joint marginal: 12)

enum { kPgPrior = 0, kPgBetween = 1, kPgGps = 2 };

struct PgFactor {                     // measurement in fp64; sw = 1 / sqrt(variance) per residual row
    int32_t type, i, j, rows;
    double R[9], t[3], sw[6], k;      // k > 0: Cauchy scale
};

struct PgIncidence { int32_t factor, side; };      // an extra factor that touches a key (side 0: its i block, 1: its j block)

// x_e = M_e x_{e-1} + C0_e in_e over elements e = 0..n-1 (e = key, or n-1-key for the transposed solve)
struct PgScan {
    int32_t levels, rev;
    int32_t n[kPgMaxLevels];
    double* M[kPgMaxLevels];          // n x 36
    double* Pre[kPgMaxLevels];        // n x 36: M_e ... M_(first of e's group)
    double* loc[kPgMaxLevels];        // n x 6
    double* C0;                       // n x 36 (level 0 only)
};

struct PgScalars {
    double rr, bb, pq, alpha, beta, tol2, err, wmin;
    int32_t stop, iters, max_iters, pad;
};

struct PgDev {
    int32_t n, n_extra;
    double* X;                        // n x 12: R row-major, t
    double* Xtrial;
    const PgFactor* chain;            // n: [0] the prior on key 0, [i] between(i-1, i)
    const PgFactor* extra;            // n_extra
    const int32_t* inc_start;         // n + 1
    const PgIncidence* inc;
    double* Binv;                     // n x 36
    double* Aof;                      // n x 36: [i] = whitened Jacobian of chain[i] with respect to key i-1
    double* rc;                       // n x 6
    double* Ji; double* Jj; double* rx;   // extras: n_extra x 36, x 36, x 6
    double* ferr; double* fw;         // per factor (chain first, then extras): error term, robust weight
    PgScan fwd, bwd;
    double *b, *y, *r, *p, *q, *t1, *t2, *u, *g, *delta;   // 6n each (u: 6 n_extra)
    double* partial;                  // kPgDotBlocks
    PgScalars* sc;
};

hipError_t pg_linearize(hipStream_t s, const PgDev& d, const double* X);           // -> Binv, Aof, rc, Ji, Jj, rx, ferr, fw, both scans, sc->err / wmin
hipError_t pg_rhs(hipStream_t s, const PgDev& d);                                 // b = -(r_c + K^T r_x)
hipError_t pg_cg_begin(hipStream_t s, const PgDev& d, double tol, int max_iters); // y = 0, r = p = b
hipError_t pg_cg_iterations(hipStream_t s, const PgDev& d, int count);            // each a no-op once sc->stop is set
hipError_t pg_step(hipStream_t s, const PgDev& d);                                // delta = J_c^-1 y, Xtrial = X (+) delta
hipError_t pg_bwd_unit(hipStream_t s, const PgDev& d, int key, int axis);         // b = J_c^-T e_(6 key + axis)
hipError_t pg_fwd_y(hipStream_t s, const PgDev& d);                               // delta = J_c^-1 y
// One operator of the linearisation on the work vectors, by the launches pg_cg_iterations queues (the observation hooks of
// include/liorf_s2m_debug.h): 0: t1 = J_c^-1 p;  1: t2 = J_c^-T g;  2: u = K p (t1 = J_c^-1 p on the way);  3: t2 = K^T u (through g).
// 2 and 3 need an extra factor.
hipError_t pg_apply(hipStream_t s, const PgDev& d, int op);
hipError_t pg_retract(hipStream_t s, const PgDev& d);                             // Xtrial = X (+) delta

// ---- the block form of the linear solve: C <= kPgBlockCols right-hand sides advance in lockstep through shared launches,
// column c = grid row c (blockIdx.y).  `d` is a copy of the graph's PgDev whose vectors b .. delta, u, partial, sc and the
// scans' loc[] point at column 0 of block storage; column c lies `vec` (`u`, `loc_f`, `loc_b`) doubles further on, its
// kPgDotBlocks partials at partial + c kPgDotBlocks, its scalars at sc + c.  Every column runs the single form's per-column
// code with the single form's assignment of elements to lanes and workgroups, and stops by its own flag, so column c is
// bit for bit the single solve of the same right-hand side.
struct PgCols {
    int32_t cols, pad;
    size_t vec, u, loc_f, loc_b;
};
struct PgColAt { int32_t v[kPgBlockCols]; };
hipError_t pg_bwd_unit_cols(hipStream_t s, const PgDev& d, const PgCols& c, const PgColAt& at);   // b_c = J_c^-T e_(at[c])
hipError_t pg_cg_begin_cols(hipStream_t s, const PgDev& d, const PgCols& c, double tol, int max_iters);
hipError_t pg_cg_iterations_cols(hipStream_t s, const PgDev& d, const PgCols& c, int count);      // a stopped column is not touched
hipError_t pg_fwd_y_cols(hipStream_t s, const PgDev& d, const PgCols& c);                         // delta_c = J_c^-1 y_c
hipError_t pg_apply_cols(hipStream_t s, const PgDev& d, const PgCols& c, int op);                 // pg_apply on every column
// rows[12 c + 0..5] = delta_c of key ka[c], rows[12 c + 6..11] = delta_c of key kb[c] (zeros where kb[c] < 0)
hipError_t pg_rows_cols(hipStream_t s, const PgDev& d, const PgCols& c, const PgColAt& ka, const PgColAt& kb, double* rows);

// ---- the launched optimise: the Gauss-Newton loop of s2m_pg_optimize with its decisions taken on the device.  The record holds
// the result's fields, the running error, the gates of the kernels that return at their head (nonzero = skip) and A, the
// estimate of the last variable (12 doubles) after the last kept step.  pg_async_open linearises at d.X and opens the record;
// pg_async_segment queues, in this order: the head of a step (rhs, CG begin; runs if a step was opened), cg_chunk CG
// iterations (they stop by sc->stop), and the tail (step, linearisation at the trial point, close, trial -> d.X if the step
// is kept; runs if the CG has stopped).  Segments are queued back to back until `done` shows in the record; every kernel
// behind `done` returns at its head.  d.X holds the estimates throughout (no pointer swap).
struct PgRecord {
    int32_t iterations, inner_iterations, converged, done;
    int32_t skip_head, skip_tail, skip_keep, max_iterations;
    double  err, error_before, error_after, wmin, abs_tol, rel_tol;
    double  A[12];
};
hipError_t pg_async_open(hipStream_t s, const PgDev& d, PgRecord* rec, int max_iterations, double abs_tol, double rel_tol);
hipError_t pg_async_segment(hipStream_t s, const PgDev& d, PgRecord* rec, double tol, int max_cg, int cg_chunk);

hipError_t pg_poses(hipStream_t s, const double* X, int first, int count, float* xyzrpy, float4* pos);   // pos: may be null
// correctPoses() in two launches: 18 floats per key (pose vector, 3x4 transform) and a not-finite flag into `stage`, then - once
// the host has seen the flag - positions and cached transforms into the key-frame store
struct KfFrame;
hipError_t pg_store_stage(hipStream_t s, const double* X, int first, int count, float* stage, int32_t* bad);
hipError_t pg_store_write(hipStream_t s, const float* stage, int count, float4* pos, KfFrame* frames);

}  // namespace s2m
