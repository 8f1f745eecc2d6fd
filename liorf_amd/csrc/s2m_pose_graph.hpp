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

// ---- One family of kernels serves the optimise, the marginals and the launched optimise.
// Columns.  Every kernel of the linear solve (the chain scans, the extra factors' products, the CG steps, the unit vector)
// takes its column from its grid row (blockIdx.y): C <= kPgBlockCols right-hand sides advance in lockstep through shared
// launches.  `d` is then a copy of the graph's PgDev whose vectors b .. delta, u, partial, sc and the scans' loc[] point at
// column 0 of block storage; column c lies `vec` (`u`, `loc_f`, `loc_b`) doubles further on, its kPgDotBlocks partials at
// partial + c kPgDotBlocks, its scalars at sc + c, and it stops by its own flag.  The single solve is kPgOne on the graph's own
// PgDev.  Since one kernel serves both, with the same assignment of elements to lanes and workgroups whatever the number of
// columns, column c is by construction bit for bit the single solve of the same right-hand side.
struct PgCols {
    int32_t cols, pad;
    size_t vec, u, loc_f, loc_b;
};
constexpr PgCols kPgOne{ 1, 0, 0, 0, 0, 0 };        // one column: no stride is ever applied
struct PgColAt { int32_t v[kPgBlockCols]; };
// Gates.  Every kernel but the CG iteration's own (they stop by sc[c].stop) takes a PgGate and reads it first, before any
// other load: the int32 at base + c * stride bytes, nonzero = return at the head; a null base = run.  stride is
// sizeof(PgScalars) where column c stops by sc[c].stop (the scans and products inside a CG iteration) and 0 for a gate of
// the launched optimise's record.  No kernel waits for another.
struct PgGate {
    const int32_t* base;
    size_t stride;
};

hipError_t pg_linearize(hipStream_t s, const PgDev& d, const double* X, PgGate gate = {});   // -> Binv, Aof, rc, Ji, Jj, rx, ferr, fw, both scans, sc->err / wmin
hipError_t pg_rhs(hipStream_t s, const PgDev& d, PgGate gate = {});                          // b = -(r_c + K^T r_x)
hipError_t pg_step(hipStream_t s, const PgDev& d, PgGate gate = {});                         // delta = J_c^-1 y, Xtrial = X (+) delta
hipError_t pg_retract(hipStream_t s, const PgDev& d);                                        // Xtrial = X (+) delta
// y_c = 0, r_c = p_c = b_c; `close`, if given, is set to 1 behind it (the launched optimise shuts its head gate there)
hipError_t pg_cg_begin(hipStream_t s, const PgDev& d, const PgCols& c, double tol, int max_iters, PgGate gate = {}, int32_t* close = nullptr);
hipError_t pg_cg_iterations(hipStream_t s, const PgDev& d, const PgCols& c, int count);      // a stopped column is not touched
hipError_t pg_bwd_unit(hipStream_t s, const PgDev& d, const PgCols& c, const PgColAt& at);   // b_c = J_c^-T e_(at[c])
hipError_t pg_fwd_y(hipStream_t s, const PgDev& d, const PgCols& c);                         // delta_c = J_c^-1 y_c
// One operator of the linearisation on every column's work vectors, by the launches pg_cg_iterations queues (the observation
// hooks of include/liorf_s2m_debug.h): 0: t1 = J_c^-1 p;  1: t2 = J_c^-T g;  2: u = K p (t1 = J_c^-1 p on the way);
// 3: t2 = K^T u (through g).  2 and 3 need an extra factor.
hipError_t pg_apply(hipStream_t s, const PgDev& d, const PgCols& c, int op);
// rows[12 c + 0..5] = delta_c of key ka[c], rows[12 c + 6..11] = delta_c of key kb[c] (zeros where kb[c] < 0)
hipError_t pg_rows(hipStream_t s, const PgDev& d, const PgCols& c, const PgColAt& ka, const PgColAt& kb, double* rows);

// ---- the launched optimise: the Gauss-Newton loop of s2m_pg_optimize with its decisions taken on the device.  The record holds
// the result's fields, the running error, the gates (nonzero = skip) and A, the estimate of the last variable (12 doubles)
// after the last kept step.  pg_async_open linearises at d.X and opens the record (k_pg_open); pg_async_segment queues, in
// this order: the head of a step (pg_rhs, pg_cg_begin gated by skip_head; runs if a step was opened), cg_chunk CG iterations
// (they stop by sc->stop), k_pg_gate, and the tail (pg_step, pg_linearize at the trial point gated by skip_tail, k_pg_close,
// k_pg_keep: trial -> d.X if the step is kept; runs if the CG has stopped).  These are the functions s2m_pg_optimize calls,
// with a record gate where it passes none.  Segments are queued back to back until `done` shows in the record; every kernel
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
