// s2m_pg_consistency.hip — kernels of s2m_pg_consistent_loops (s2m_pg_consistency.hpp): which of many loop
// candidates agree with one another pair by pair, judged on the graph's current estimates before any of them becomes a factor.
//   k_pgc_steps_scan / k_pgc_scan_sums / k_pgc_scan_add   the chain length s[k] in whole micrometres, a blocked int64 prefix sum
//   k_pgc_pairs     a tile of 64 candidates in LDS, a row candidate per lane: one 64-bit word of the matrix per lane, one store
//   k_pgc_degree    a row's popcount;  k_pgc_rank  (degree descending, index ascending) with the degrees in LDS
//   k_pgc_permute   the matrix in rank order, a ballot per word
//   k_pgc_grow      one wave per start: lane w holds word w of the candidate set C, a step is one 512-byte row load and an AND
//   k_pgc_pick      the largest set (ties: the best-ranked start), grown once more to write selected[], degrees' sum, the record
// Compiled with -ffp-contract=off: no fused multiply-add, every three-term sum is ((a0 b0 + a1 b1) + a2 b2), so the NumPy model
// (tests/ref/pg_consistency_ref.py) restates the arithmetic bit for bit.  The chain length and everything behind the pair
// measure is integer or bit work.  No kernel uses atomics, none adds floating-point numbers across lanes, none waits for or
// reads the progress of another workgroup: every output word has one writer and is a fixed function of the inputs.
#include <math.h>

#include "s2m_pg_consistency.hpp"

namespace s2m {

namespace {

constexpr int T = kPgcTile;
constexpr int kScanThreads = 256, kScanPer = kPgcScanKeys / kScanThreads;   // keys per thread of a scan block
constexpr int kRankThreads = 256;
constexpr double kPgcStepCap = 2.5e11;               // micrometres: a longer (or not finite) step counts as this much, so 2^24 steps fit int64
static_assert(kScanPer * kScanThreads == kPgcScanKeys, "whole keys per thread");

typedef unsigned long long u64;

// ---- chain length ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long pgc_step(const double* __restrict__ X, int k)
{
    const double dx = X[12 * (size_t)k + 9] - X[12 * (size_t)(k - 1) + 9], dy = X[12 * (size_t)k + 10] - X[12 * (size_t)(k - 1) + 10],
                 dz = X[12 * (size_t)k + 11] - X[12 * (size_t)(k - 1) + 11];
    const double v = 1e6 * sqrt(((dx * dx + dy * dy) + dz * dz));
    return llrint(v < kPgcStepCap ? v : kPgcStepCap);
}

// inclusive scan of one value per thread over the workgroup (integers: any order gives the same sum)
__device__ __forceinline__ long long block_scan_incl(long long v, long long* buf /* [2][kScanThreads] */)
{
    const int t = threadIdx.x;
    int cur = 0;
    buf[t] = v;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const long long a = buf[cur * kScanThreads + t] + (t >= off ? buf[cur * kScanThreads + t - off] : 0);
        buf[(cur ^ 1) * kScanThreads + t] = a;
        cur ^= 1;
        __syncthreads();
    }
    return buf[cur * kScanThreads + t];
}

// block b: s[k] for its kPgcScanKeys keys, relative to the block's first key, and the block's total
__global__ __launch_bounds__(kScanThreads) void k_pgc_steps_scan(const double* __restrict__ X, int n, long long* __restrict__ s,
                                                                long long* __restrict__ blk)
{
    __shared__ long long buf[2 * kScanThreads];
    const int k0 = blockIdx.x * kPgcScanKeys + threadIdx.x * kScanPer;
    long long loc[kScanPer], run = 0;
#pragma unroll
    for (int j = 0; j < kScanPer; j++) {
        const int k = k0 + j;
        run += (k > 0 && k < n) ? pgc_step(X, k) : 0;
        loc[j] = run;
    }
    const long long before = block_scan_incl(run, buf) - run;
#pragma unroll
    for (int j = 0; j < kScanPer; j++)
        if (k0 + j < n) s[k0 + j] = before + loc[j];
    if (threadIdx.x == kScanThreads - 1) blk[blockIdx.x] = before + run;
}

// one workgroup: blk[b] becomes the sum of the blocks before b
__global__ __launch_bounds__(kScanThreads) void k_pgc_scan_sums(long long* __restrict__ blk, int nb)
{
    __shared__ long long buf[2 * kScanThreads];
    const int per = (nb + kScanThreads - 1) / kScanThreads;
    const int b0 = min(nb, (int)threadIdx.x * per), b1 = min(nb, b0 + per);
    long long run = 0;
    for (int b = b0; b < b1; b++) run += blk[b];
    long long before = block_scan_incl(run, buf) - run;
    for (int b = b0; b < b1; b++) { const long long v = blk[b]; blk[b] = before; before += v; }
}

__global__ __launch_bounds__(kScanThreads) void k_pgc_scan_add(long long* __restrict__ s, int n, const long long* __restrict__ blk)
{
    const int k = blockIdx.x * kScanThreads + threadIdx.x;
    if (k < n) s[k] += blk[k / kPgcScanKeys];
}

// ---- the pair measure --------------------------------------------------------------------------------------------------
// States are 12 doubles: R row-major, then t.
__device__ __forceinline__ void se3_inv(const double* A, double* O)              // (R^T, -(R^T t))
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) O[i * 3 + j] = A[j * 3 + i];
        O[9 + i] = -((A[i] * A[9] + A[3 + i] * A[10]) + A[6 + i] * A[11]);
    }
}

__device__ __forceinline__ void se3_mul(const double* A, const double* B, double* O)   // (A_R B_R, (A_R B_t) + A_t)
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) O[i * 3 + j] = (A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j]) + A[i * 3 + 2] * B[6 + j];
        O[9 + i] = ((A[i * 3] * B[9] + A[i * 3 + 1] * B[10]) + A[i * 3 + 2] * B[11]) + A[9 + i];
    }
}

struct PgcTol { double tol_m, tol_chord, rate_m, rate_chord; };

// a, b: X_from | X_to | Z of the candidate with the lower and the higher index; sa, sb: s[from], s[to] of each
__device__ __forceinline__ bool pgc_consistent(const double* a, const long long* sa, const double* b, const long long* sb, const PgcTol& tol)
{
    double inv[12], Ot[12], Of[12], M1[12], M2[12], D[12];
    se3_inv(a + 12, inv); se3_mul(inv, b + 12, Ot);          // O_t = X_to_a^-1 X_to_b
    se3_inv(a, inv);      se3_mul(inv, b, Of);               // O_f = X_from_a^-1 X_from_b
    se3_mul(a + 24, Ot, M1);                                 // M1 = Z_a O_t
    se3_mul(Of, b + 24, M2);                                 // M2 = O_f Z_b
    se3_inv(M1, inv);     se3_mul(inv, M2, D);               // D = M1^-1 M2 (only its diagonal and its t are used)
    const double rho2 = ((3.0 - D[0]) - D[4]) - D[8];
    const double d2 = (D[9] * D[9] + D[10] * D[10]) + D[11] * D[11];
    const long long df = sa[0] - sb[0], dt = sa[1] - sb[1];
    const double L = (double)((df < 0 ? -df : df) + (dt < 0 ? -dt : dt)) * 1e-6;
    const double tc = tol.tol_chord + tol.rate_chord * L, tm = tol.tol_m + tol.rate_m * L;
    return isfinite(rho2) && isfinite(d2) && rho2 <= tc * tc && d2 <= tm * tm;
}

// Workgroup (x, y), one wave: rows [x * T, x * T + T), one per lane, against the candidates of tile y; the lane builds word y of
// its row in a register and stores it.  Every lane reads the same item of the tile per step (an LDS broadcast).  A pair is always
// evaluated as (lower index, higher index), by the row lane of either side, so bits (p, q) and (q, p) come from the same
// arithmetic; only the tiles on the diagonal have lanes on both sides of that branch.  Lanes behind m walk along with the last
// row and store nothing; columns behind m leave their bits 0.
__global__ __launch_bounds__(T) void k_pgc_pairs(const double* __restrict__ X, const long long* __restrict__ s, const PgcCand* __restrict__ cand,
                                                 int m, int words, PgcTol tol, u64* __restrict__ mat)
{
    __shared__ double s_c[T][36];
    __shared__ long long s_s[T][2];
    const int lane = threadIdx.x;
    const int c0 = blockIdx.y * T, nc = min(T, m - c0);
    for (int e = lane; e < nc * 36; e += T) {
        const int k = e / 36, j = e % 36;
        const PgcCand& c = cand[c0 + k];
        s_c[k][j] = j < 12 ? X[12 * (size_t)c.from + j] : j < 24 ? X[12 * (size_t)c.to + (j - 12)] : c.Z[j - 24];
    }
    for (int e = lane; e < nc * 2; e += T) {
        const PgcCand& c = cand[c0 + e / 2];
        s_s[e / 2][e % 2] = s[(e % 2) ? c.to : c.from];
    }
    __syncthreads();
    const int p = blockIdx.x * T + lane;
    const bool live = p < m;
    const int pr = live ? p : m - 1;
    double row[36];
    long long rs[2];
    {
        const PgcCand& c = cand[pr];
#pragma unroll
        for (int j = 0; j < 12; j++) { row[j] = X[12 * (size_t)c.from + j]; row[12 + j] = X[12 * (size_t)c.to + j]; row[24 + j] = c.Z[j]; }
        rs[0] = s[c.from]; rs[1] = s[c.to];
    }
    u64 word = 0;
    for (int k = 0; k < nc; k++) {
        const int q = c0 + k;
        bool bit = false;
        if (pr < q) bit = pgc_consistent(row, rs, s_c[k], s_s[k], tol);
        else if (pr > q) bit = pgc_consistent(s_c[k], s_s[k], row, rs, tol);
        word |= (u64)(bit ? 1 : 0) << k;
    }
    if (live) mat[(size_t)p * words + blockIdx.y] = word;
}

// ---- degree, rank, the matrix in rank order ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pgc_degree(const u64* __restrict__ mat, int m, int words, int32_t* __restrict__ deg)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    int c = lane < words ? __popcll(mat[(size_t)p * words + lane]) : 0;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if (lane == 0) deg[p] = c;
}

// rank[p] = #{q : deg[q] > deg[p] or (deg[q] == deg[p] and q < p)}: a permutation, so order[] is written once everywhere
__global__ __launch_bounds__(kRankThreads) void k_pgc_rank(const int32_t* __restrict__ deg, int m, int32_t* __restrict__ rank, int32_t* __restrict__ order)
{
    __shared__ int32_t s_deg[S2M_PG_CONSISTENCY_MAX];
    for (int i = threadIdx.x; i < m; i += kRankThreads) s_deg[i] = deg[i];
    __syncthreads();
    const int p = blockIdx.x * kRankThreads + threadIdx.x;
    if (p >= m) return;
    const int d = s_deg[p];
    int r = 0;
    for (int q = 0; q < m; q++) {
        const int dq = s_deg[q];
        r += (dq > d || (dq == d && q < p)) ? 1 : 0;
    }
    rank[p] = r;
    order[r] = p;
}

// row r of the matrix in rank order: bit c is bit order[c] of row order[r]; a ballot makes word w, lane w keeps it
__global__ __launch_bounds__(64) void k_pgc_permute(const u64* __restrict__ mat, const int32_t* __restrict__ order, int m, int words,
                                                    u64* __restrict__ mat_rank)
{
    __shared__ u64 s_row[kPgcMaxWords];
    const int r = blockIdx.x, lane = threadIdx.x;
    const int p = order[r];
    s_row[lane] = lane < words ? mat[(size_t)p * words + lane] : 0;
    __syncthreads();
    u64 mine = 0;
    for (int w = 0; w < words; w++) {
        const int c = w * 64 + lane;
        bool bit = false;
        if (c < m) { const int q = order[c]; bit = (s_row[q >> 6] >> (q & 63)) & 1; }
        const u64 b = __ballot(bit);
        if (lane == w) mine = b;
    }
    if (lane < words) mat_rank[(size_t)r * words + lane] = mine;
}

// ---- the greedy growth -------------------------------------------------------------------------------------------------
// One wave grows the set of start v (a rank): lane w holds word w of C.  The best-ranked member of C is the lowest set bit of the
// lowest lane whose word is not 0.  The diagonal is 0, so a step clears at least bit u; the loop is bounded by m all the same.
// members: lane w's word of S, if wanted.  Returns |S|.
__device__ __forceinline__ int pgc_grow(const u64* __restrict__ mat_rank, int v, int m, int words, int lane, u64* members)
{
    u64 c = lane < words ? mat_rank[(size_t)v * words + lane] : 0;
    u64 mem = lane == (v >> 6) ? (u64)1 << (v & 63) : 0;
    int size = 1;
    for (int step = 0; step < m; step++) {
        const u64 nz = __ballot(c != 0);
        if (nz == 0) break;
        const int l = __ffsll((long long)nz) - 1;
        const u64 cw = __shfl(c, l);
        const int u = l * 64 + (__ffsll((long long)cw) - 1);
        if (u >= m) break;                                  // (no bit stands behind m; never a row outside the matrix)
        size++;
        if (lane == l) mem |= (u64)1 << (u & 63);
        c &= lane < words ? mat_rank[(size_t)u * words + lane] : 0;
    }
    if (members) *members = mem;
    return size;
}

__global__ __launch_bounds__(64) void k_pgc_grow(const u64* __restrict__ mat_rank, int m, int words, int32_t* __restrict__ size)
{
    const int n = pgc_grow(mat_rank, blockIdx.x, m, words, threadIdx.x, nullptr);
    if (threadIdx.x == 0) size[blockIdx.x] = n;
}

// One wave: the start with the largest set, equal sizes to the lowest rank; its set once more for the members; selected[] in the
// caller's order, every entry written once; the record.  out: selected | degree (written by k_pgc_degree) | PgcOut.
__global__ __launch_bounds__(64) void k_pgc_pick(const u64* __restrict__ mat_rank, const int32_t* __restrict__ order, const int32_t* __restrict__ size,
                                                 int m, int words, unsigned char* __restrict__ out, size_t deg_off, size_t rec_off)
{
    __shared__ u64 s_mem[kPgcMaxWords];
    const int lane = threadIdx.x;
    const int32_t* deg = reinterpret_cast<const int32_t*>(out + deg_off);
    int best = -1;                                          // (size << 13) | (8191 - rank): larger is better
    long long sum = 0;
    for (int r = lane; r < m; r += 64) {
        best = max(best, (size[r] << 13) | (8191 - r));
        sum += deg[r];
    }
    for (int off = 32; off > 0; off >>= 1) {
        best = max(best, __shfl_xor(best, off));
        sum += __shfl_xor(sum, off);
    }
    const int v = 8191 - (best & 8191);
    u64 mem;
    const int n_sel = pgc_grow(mat_rank, v, m, words, lane, &mem);
    s_mem[lane] = mem;
    __syncthreads();
    for (int c = lane; c < m; c += 64) out[order[c]] = (unsigned char)((s_mem[c >> 6] >> (c & 63)) & 1);
    if (lane == 0) {
        PgcOut* rec = reinterpret_cast<PgcOut*>(out + rec_off);
        rec->n_candidates = m; rec->n_selected = n_sel; rec->start = order[v]; rec->reserved = 0;
        rec->n_consistent_pairs = sum / 2;
    }
}

}  // namespace

hipError_t pgc_launch(hipStream_t stream, const PgcArgs& a)
{
    if (a.n <= 0 || a.m <= 0 || a.m > S2M_PG_CONSISTENCY_MAX) return hipErrorInvalidValue;
    const int words = (int)pgc_words(a.m), nb = (int)pgc_scan_blocks(a.n);
    int32_t* rank = a.rank;
    int32_t* order = rank + a.m;
    int32_t* size = order + a.m;
    int32_t* deg = reinterpret_cast<int32_t*>(a.out + pgc_deg_off(a.m));
    hipLaunchKernelGGL(k_pgc_steps_scan, dim3((unsigned)nb), dim3(kScanThreads), 0, stream, a.X, a.n, a.s, a.blk);
    hipLaunchKernelGGL(k_pgc_scan_sums, dim3(1), dim3(kScanThreads), 0, stream, a.blk, nb);
    hipLaunchKernelGGL(k_pgc_scan_add, dim3((unsigned)((a.n + kScanThreads - 1) / kScanThreads)), dim3(kScanThreads), 0, stream, a.s, a.n,
                       (const long long*)a.blk);
    hipLaunchKernelGGL(k_pgc_pairs, dim3((unsigned)words, (unsigned)words), dim3(T), 0, stream, a.X, (const long long*)a.s, a.cand, a.m, words,
                       PgcTol{ a.tol_m, a.tol_chord, a.rate_m, a.rate_chord }, a.mat);
    hipLaunchKernelGGL(k_pgc_degree, dim3((unsigned)a.m), dim3(64), 0, stream, (const u64*)a.mat, a.m, words, deg);
    hipLaunchKernelGGL(k_pgc_rank, dim3((unsigned)((a.m + kRankThreads - 1) / kRankThreads)), dim3(kRankThreads), 0, stream, (const int32_t*)deg,
                       a.m, rank, order);
    hipLaunchKernelGGL(k_pgc_permute, dim3((unsigned)a.m), dim3(64), 0, stream, (const u64*)a.mat, (const int32_t*)order, a.m, words, a.mat_rank);
    hipLaunchKernelGGL(k_pgc_grow, dim3((unsigned)a.m), dim3(64), 0, stream, (const u64*)a.mat_rank, a.m, words, size);
    hipLaunchKernelGGL(k_pgc_pick, dim3(1), dim3(64), 0, stream, (const u64*)a.mat_rank, (const int32_t*)order, (const int32_t*)size, a.m, words,
                       a.out, pgc_deg_off(a.m), pgc_rec_off(a.m));
    return hipGetLastError();
}

}  // namespace s2m
