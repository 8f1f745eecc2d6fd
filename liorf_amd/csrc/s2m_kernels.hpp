// s2m_kernels.hpp — hand-written HIP kernels (gfx950 / CDNA4, wave64) of the scan-to-map
// registration path: the LM loop.  The heads of a launch, the wave table (extent-only and
// re-split for the map's density), the closing step, k_register (s2m_register.hpp, included below), k_finalize and the
// uploads of the context and state blocks.  Included by s2m_abi.hip alone: the code of a loop
// kernel depends on which other loop kernels share its module, so they all stay in this one.
// The map index and the scan ordering are s2m_prep.hpp's, the helpers shared with them s2m_device.hpp's.
// Compiled with -ffp-contract=off: every fp32 expression that mirrors the
// reference is evaluated as written (one rounding per operation), and HIP's default
// correctly-rounded fp32 divide/sqrt keeps the per-correspondence arithmetic bit-identical
// to an x86-64 (no-FMA) build of the reference.
//
// Reference citations are file:line into jimmyshe/liorf (src/mapOptmization.cpp unless named).
#pragma once
#include "s2m_device.hpp"

namespace s2m {

// The head of a registration launch.  Line 0 of DevCtx and line 0 of DevState are read whole, field by field, as the first
// thing a kernel does - before the `done` branch, so that the two misses overlap and nothing is fetched where it is first
// used, one dependent round trip per field group (both blocks are always allocated: reading them in a launch that returns at
// once is harmless).  What they hold is exactly what the next requests need: the rows of partial sums the previous launch
// left, the wave's first table entry, then its points.  LmParams: the four parameters the close reads at the end of its
// serial part, from line 2 - asked for with the second group of requests.
struct CtxHead { int32_t nblocks, n_q; const int2* wave_table; double* partials; const float *qx, *qy, *qz; float4 *cert, *plane_cache; };
struct StateHead { int32_t done, n_waves, isDegenerate, T_valid; float pose[6]; };      // pose: pose2[slot]
struct LmParams { int32_t min_corr, early_exit; double conv_deg, conv_cm; };
// (kPin = false: the fields by name, fetched where the compiler sees fit - the search kernel, whose worklist loop would hold them
// in registers it does not have.  a0, a1: the kernel's two scalar arguments, which lie in another line of the argument block
// than the slot's pointers and would otherwise be fetched where they are first looked at)
template <bool kPin = true>
__device__ __forceinline__ void load_heads(CtxP cp, gptr<DevState> st, int slot, CtxHead& c, StateHead& s, int& a0, int& a1)
{
    c.nblocks = cp->nblocks; c.n_q = cp->n_q; c.wave_table = cp->wave_table; c.partials = cp->partials;
    c.qx = cp->qx; c.qy = cp->qy; c.qz = cp->qz; c.cert = cp->cert; c.plane_cache = cp->plane_cache;
    s.done = st->done; s.n_waves = st->n_waves; s.isDegenerate = st->isDegenerate; s.T_valid = st->T_valid;
#pragma unroll
    for (int k = 0; k < 6; k++) s.pose[k] = st->pose2[slot][k];
    // (the values are wanted here, all at once: without this the compiler moves every load down to its first use)
    if (kPin)
    asm volatile("" : "+s"(c.nblocks), "+s"(c.n_q), "+s"(c.wave_table), "+s"(c.partials), "+s"(c.qx), "+s"(c.qy), "+s"(c.qz),
                      "+s"(c.cert), "+s"(c.plane_cache), "+s"(s.done), "+s"(s.n_waves), "+s"(s.isDegenerate), "+s"(s.T_valid),
                      "+s"(s.pose[0]), "+s"(s.pose[1]), "+s"(s.pose[2]), "+s"(s.pose[3]), "+s"(s.pose[4]), "+s"(s.pose[5]), "+s"(a0), "+s"(a1));
}
__device__ __forceinline__ LmParams lm_params(CtxP cp)
{
    LmParams p;
    p.min_corr = cp->min_corr; p.early_exit = cp->early_exit; p.conv_deg = cp->conv_deg; p.conv_cm = cp->conv_cm;
    return p;
}
__device__ __forceinline__ void swap_if(bool c, float& a, float& b)
{
    float t = a; a = c ? b : a; b = c ? t : b;
}
__device__ __forceinline__ void swap_if(bool c, int& a, int& b)
{
    int t = a; a = c ? b : a; b = c ? t : b;
}

// one workgroup: exclusive scan of parts[] and emission of the wave table {first point, count}.
// The table has room for every chunk unsplit plus a budget of extra waves; if the wishes exceed
// it they are scaled back uniformly (cap 8 -> 4 -> 2 -> 1), so the table never overflows.
// `factor` (optional, consumed and zeroed): extra split asked for by k_wave_density; `st` (optional)
// receives the new wave count as well.
__device__ __forceinline__ void chunk_table_body(const int32_t* __restrict__ parts, int n, int n_chunks, int capacity,
                                                 int2* __restrict__ table, int32_t* __restrict__ n_waves_out,
                                                 int32_t* __restrict__ factor, DevState* __restrict__ st)
{
    __shared__ int32_t wsum[16];
    __shared__ int32_t carry_s, tot_s[3], base_s, pol_s[9];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // One workgroup per CU runs measurably faster than two (steady launch 25 vs 27.7 us at 120k points): the
    // density wishes are dropped if they alone would push the grid over one workgroup on each of the 256 CUs.
    constexpr int kOnePerCu = 256 * (kBlock / 64);
    bool use_factor = factor != nullptr;
    if (use_factor) {
        int tb = 0, tf = 0;
        for (int c = threadIdx.x; c < n_chunks; c += 1024) { tb += min(8, parts[c]); tf += min(8, parts[c] * max(factor[c], 1)); }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { tb += __shfl_xor(tb, off, 64); tf += __shfl_xor(tf, off, 64); }
        if (threadIdx.x == 0) { tot_s[0] = 0; base_s = 0; }
        __syncthreads();
        if (lane == 0) { atomicAdd(&base_s, tb); atomicAdd(&tot_s[0], tf); }
        __syncthreads();
        use_factor = !(base_s <= kOnePerCu && tot_s[0] > kOnePerCu);
        __syncthreads();
    }
    // pass A: total waves wished for under each way of scaling the wishes back, mildest first.  The density wishes are the ones
    // that count - a launch lasts as long as its slowest wave, and the slowest are the waves whose box streams thousands of map
    // points - so the chunks that asked for the finest cut keep it longest: 0 every wish; 1 / 2 density wishes below 4 / below 8
    // dropped; 3..5 as 2 with the other chunks capped at 4, 2, 1; 6..8 as 2 with every chunk capped at 4, 2, 1.
    // (Scaling every wish back alike left the heaviest chunks of a dense map at two parts: dense1m launch 0, slowest wave 223 us.)
    constexpr int kPolicies = 9;
    auto wish_under = [&](int c, int pol) {
        const int f = use_factor ? max(factor[c], 1) : 1;
        const bool heavy = f >= 8;
        const int fe = (pol == 0) ? f : ((pol == 1) ? (f >= 4 ? f : 1) : (heavy ? f : 1));
        const int w = min(8, parts[c] * fe);
        const int cap = (pol <= 2) ? 8 : ((pol <= 5) ? (heavy ? 8 : (32 >> pol)) : (256 >> pol));      // 3,4,5 -> 4,2,1; 6,7,8 -> 4,2,1
        return min(w, cap);
    };
    int tp[kPolicies];
#pragma unroll
    for (int k = 0; k < kPolicies; k++) tp[k] = 0;
    for (int c = threadIdx.x; c < n_chunks; c += 1024) {
#pragma unroll
        for (int k = 0; k < kPolicies; k++) tp[k] += wish_under(c, k);
    }
#pragma unroll
    for (int k = 0; k < kPolicies; k++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) tp[k] += __shfl_xor(tp[k], off, 64);
    }
    if (threadIdx.x == 0) carry_s = 0;
    if (threadIdx.x < kPolicies) pol_s[threadIdx.x] = 0;
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kPolicies; k++) atomicAdd(&pol_s[k], tp[k]);
    }
    __syncthreads();
    // (Until the last session of round 4 a scan whose unsplit chunks fitted the 4 096 co-resident waves gave up every split before
    // it gave up that - measured on the round-2 kernel, 262 144 points = 4 096 chunks exactly: 20.5 k -> 22.2 k LM iterations/s.
    // With the rebuilt search the opposite holds: ouster128's launches 0-3 272 -> 222 us with its scattered and dense chunks split,
    // launch 1 below launch 0 at last, and the 30-launch loop no slower, 0.70 ms either way - the second entry some waves take in
    // a steady launch costs less than the stragglers of the cold ones.  The table's own capacity is the only limit now.)
    const int cap_eff = capacity;
    int pol = kPolicies - 1;
#pragma unroll
    for (int k = kPolicies - 2; k >= 0; k--) if (pol_s[k] <= cap_eff) pol = k;
    auto wish = [&](int c) { return wish_under(c, pol); };
    constexpr int pcap = 8;
    // pass B: scan and emit
    for (int base = 0; base < n_chunks; base += 1024) {
        const int c = base + threadIdx.x;
        const int p = (c < n_chunks) ? min(wish(c), pcap) : 0;
        int incl = p;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; w++) woff += wsum[w];
        const int carry = carry_s;
        const int off0 = carry + woff + incl - p;            // first wave slot of chunk c
        if (c < n_chunks) {
            const int per = 64 / p;
            for (int j = 0; j < p; j++) {
                const int start = c * 64 + j * per;
                if (off0 + j < capacity) table[off0 + j] = make_int2(start, max(0, min(per, n - start)));
            }
        }
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = carry + woff + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int nw = min(carry_s, capacity);
        *n_waves_out = nw;
        if (st) st->n_waves = nw;
    }
    if (factor) for (int c = threadIdx.x; c < n_chunks; c += 1024) factor[c] = 0;   // every wish above was read before the last barrier
}

// per s2m_set_scan: extent-based parts only
__global__ __launch_bounds__(1024) void k_chunk_table(const PrepTable tbl)
{
    const PrepSlot& ps = tbl.s[blockIdx.y];
    if (ps.n <= 0) return;                                // an empty slot of a batch
    chunk_table_body(ps.chunk_parts, ps.n, ps.n_chunks, ps.capacity, ps.wave_table, ps.n_waves, nullptr, nullptr);
    if (ps.stamps) {                                      // ... and ends: every thread has emitted its entries
        __syncthreads();
        if (threadIdx.x == 0) ps.stamps[1] = wall_clock64();
    }
}

// per scan before launch 0, inside the captured loop: everything comes from the DevCtx block
__global__ __launch_bounds__(1024) void k_chunk_table_density(const SlotTable tbl)
{
    DevCtx* __restrict__ cp = const_cast<DevCtx*>(tbl.ctx[blockIdx.y]);
    DevState* __restrict__ st = tbl.st[blockIdx.y];
    if (!cp->density_pending) return;                     // once per scan (the flag is uniform: read before the barrier below)
    __syncthreads();
    if (threadIdx.x == 0) cp->density_pending = 0;
    chunk_table_body(cp->chunk_parts, cp->n_q, cp->n_chunks, cp->table_cap, cp->wave_table_rw, cp->n_waves_rw,
                     cp->chunk_factor, st);
}

// ------------------------------------------------------------------------------------------
// per-correspondence arithmetic
// ------------------------------------------------------------------------------------------
// 5x3 least-squares plane  A x = -1  by column-pivoted Householder QR in fp32: the
// algorithm behind `matA0.colPivHouseholderQr().solve(matB0)` (:1104, Eigen 3.3), with every
// index resolved at compile time so the 5x3 matrix lives in registers.
__device__ __forceinline__ void plane_fit_5x3(float (&qr)[5][3], float (&x)[3])
{
    float hC[3], nU[3], nD[3];
    int perm[3] = { 0, 1, 2 };
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < 5; i++) s += qr[i][k] * qr[i][k];
        nD[k] = sqrtf(s); nU[k] = nD[k];
    }
    float maxn = nU[0];
    if (nU[1] > maxn) maxn = nU[1];
    if (nU[2] > maxn) maxn = nU[2];
    const float th = maxn * FLT_EPSILON;
    const float threshold_helper = (th * th) / 5.0f;
    const float norm_downdate_threshold = sqrtf(FLT_EPSILON);
    int np = 3;

#pragma unroll
    for (int k = 0; k < 3; k++) {
        int big = k; float bign = nU[k];
#pragma unroll
        for (int j = k + 1; j < 3; j++) if (nU[j] > bign) { bign = nU[j]; big = j; }
        const float big_sq = bign * bign;
        if (np == 3 && big_sq < threshold_helper * (float)(5 - k)) np = k;
#pragma unroll
        for (int j = k + 1; j < 3; j++) {
            const bool c = (big == j);
#pragma unroll
            for (int i = 0; i < 5; i++) swap_if(c, qr[i][k], qr[i][j]);
            swap_if(c, nU[k], nU[j]); swap_if(c, nD[k], nD[j]); swap_if(c, perm[k], perm[j]);
        }
        float tailSq = 0.0f;
#pragma unroll
        for (int i = k + 1; i < 5; i++) tailSq += qr[i][k] * qr[i][k];
        const float c0 = qr[k][k];
        float beta, tau;
        if (tailSq <= FLT_MIN) {
            tau = 0.0f; beta = c0;
#pragma unroll
            for (int i = k + 1; i < 5; i++) qr[i][k] = 0.0f;
        } else {
            beta = sqrtf(c0 * c0 + tailSq);
            if (c0 >= 0.0f) beta = -beta;
            const float den = c0 - beta;
#pragma unroll
            for (int i = k + 1; i < 5; i++) qr[i][k] = qr[i][k] / den;
            tau = (beta - c0) / beta;
        }
        qr[k][k] = beta; hC[k] = tau;
        if (tau != 0.0f) {
#pragma unroll
            for (int j = k + 1; j < 3; j++) {
                float tmp = 0.0f;
#pragma unroll
                for (int i = k + 1; i < 5; i++) tmp += qr[i][k] * qr[i][j];
                tmp += qr[k][j];
                qr[k][j] -= tau * tmp;
#pragma unroll
                for (int i = k + 1; i < 5; i++) qr[i][j] -= (tau * qr[i][k]) * tmp;
            }
        }
#pragma unroll
        for (int j = k + 1; j < 3; j++) {
            if (nU[j] != 0.0f) {
                float temp = fabsf(qr[k][j]) / nU[j];
                temp = (1.0f + temp) * (1.0f - temp);
                temp = temp < 0.0f ? 0.0f : temp;
                const float r = nU[j] / nD[j];
                const float temp2 = temp * (r * r);
                if (temp2 <= norm_downdate_threshold) {
                    float s = 0.0f;
#pragma unroll
                    for (int i = k + 1; i < 5; i++) s += qr[i][j] * qr[i][j];
                    nD[j] = sqrtf(s); nU[j] = nD[j];
                } else {
                    nU[j] *= sqrtf(temp);
                }
            }
        }
    }

    x[0] = x[1] = x[2] = 0.0f;
    if (np == 0) return;
    float c[5] = { -1.0f, -1.0f, -1.0f, -1.0f, -1.0f };              // matB0.fill(-1) (:1094)
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (k < np) {
            const float tau = hC[k];
            if (tau != 0.0f) {
                float tmp = 0.0f;
#pragma unroll
                for (int i = k + 1; i < 5; i++) tmp += qr[i][k] * c[i];
                tmp += c[k];
                c[k] -= tau * tmp;
#pragma unroll
                for (int i = k + 1; i < 5; i++) c[i] -= (tau * qr[i][k]) * tmp;
            }
        }
    }
#pragma unroll
    for (int i = 2; i >= 0; i--) {
        if (i < np) {
            if (c[i] != 0.0f) {
                c[i] /= qr[i][i];
#pragma unroll
                for (int r = 0; r < i; r++) c[r] -= c[i] * qr[r][i];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if (i < np) {
#pragma unroll
            for (int t = 0; t < 3; t++) if (perm[i] == t) x[t] = c[i];
        }
    }
}

// one row of matA / matB (:1216-1234); sc = srx,crx,sry,cry,srz,crz (:1170-1175)
__device__ __forceinline__ void jacobian_row(const float (&sc)[6], float px, float py, float pz,
                                             const float (&cf)[4], float (&row)[6], float& rhs)
{
    const float srx = sc[0], crx = sc[1], sry = sc[2], cry = sc[3], srz = sc[4], crz = sc[5];
    const float arx = (-srx * cry * px - (srx * sry * srz + crx * crz) * py + (crx * srz - srx * sry * crz) * pz) * cf[0]
                    + (crx * cry * px - (srx * crz - crx * sry * srz) * py + (crx * sry * crz + srx * srz) * pz) * cf[1];
    const float ary = (-crx * sry * px + crx * cry * srz * py + crx * cry * crz * pz) * cf[0]
                    + (-srx * sry * px + srx * sry * srz * py + srx * cry * crz * pz) * cf[1]
                    + (-cry * px - sry * srz * py - sry * crz * pz) * cf[2];
    const float arz = ((crx * sry * crz + srx * srz) * py + (srx * crz - crx * sry * srz) * pz) * cf[0]
                    + ((-crx * srz + srx * sry * crz) * py + (-srx * sry * srz - crx * crz) * pz) * cf[1]
                    + (cry * crz * py - cry * srz * pz) * cf[2];
    row[0] = arz; row[1] = ary; row[2] = arx; row[3] = cf[0]; row[4] = cf[1]; row[5] = cf[2];
    rhs = -cf[3];
}

// ------------------------------------------------------------------------------------------
// shared constants and wave-level helpers of the registration kernel (s2m_register.hpp)
// ------------------------------------------------------------------------------------------
constexpr int kTilePts = 512;        // points per wave tile (8 KiB) after filtering; a tile slot fits the low 9 bits of a sweep key
constexpr int kTileRaw = 1024;       // unfiltered points of one 64-row group a wave is willing to stream through the filter
constexpr int kRowMax = 256;         // boxes with more rows go straight to the gather path
constexpr float kSlabMargin = 1e-3f; // covers the fp32 rounding of the cell binning of a local map (<= 5e-5 at 200 m extent; s2m_register.hpp adds 1e-6 per metre)
constexpr uint64_t kKeyInf = ((uint64_t)0x7f800000u << 32) | 0x7fffffffu;

// LDS written by this wave is read back by other lanes of the same wave: DS operations of one
// wave execute in order, so only the compiler has to be kept from reordering them.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// (dy,dz) of the 9 rows of a 3x3x3 neighbourhood, centre row first so that the 5th-best bound
// tightens early: (0,0),(-1,0),(1,0),(0,-1),(0,1),(-1,-1),(1,-1),(-1,1),(1,1), 2 bits each
__device__ __forceinline__ constexpr int run_dy(int k) { return (int)((139617u >> (2 * k)) & 3u) - 1; }
__device__ __forceinline__ constexpr int run_dz(int k) { return (int)((164373u >> (2 * k)) & 3u) - 1; }

// ------------------------------------------------------------------------------------------
// 6x6 algebra of LMOptimization (:1237-1271)
// ------------------------------------------------------------------------------------------
// cv::eigen (:1248): max-pivot Jacobi in fp32, eigenvalues descending, eigenvectors as rows.
// A and V are LDS scratch of the calling lane (data-dependent indexing).
__device__ void eigen6_sym(float (*A)[6], float (*V)[6], float* W, int* indR, int* indC)
{
    constexpr int N = 6;
    const float eps = FLT_EPSILON;
    for (int i = 0; i < N; i++) for (int j = 0; j < N; j++) V[i][j] = (i == j) ? 1.0f : 0.0f;
    for (int k = 0; k < N; k++) {
        W[k] = A[k][k];
        if (k < N - 1) {
            int m = k + 1; float mv = fabsf(A[k][m]);
            for (int i = k + 2; i < N; i++) { float v = fabsf(A[k][i]); if (mv < v) { mv = v; m = i; } }
            indR[k] = m;
        }
        if (k > 0) {
            int m = 0; float mv = fabsf(A[0][k]);
            for (int i = 1; i < k; i++) { float v = fabsf(A[i][k]); if (mv < v) { mv = v; m = i; } }
            indC[k] = m;
        }
    }
    for (int it = 0; it < N * N * 30; it++) {
        int k = 0, l; float mv = fabsf(A[0][indR[0]]);
        for (int i = 1; i < N - 1; i++) { float v = fabsf(A[i][indR[i]]); if (mv < v) { mv = v; k = i; } }
        l = indR[k];
        for (int i = 1; i < N; i++) { float v = fabsf(A[indC[i]][i]); if (mv < v) { mv = v; k = indC[i]; l = i; } }
        const float p = A[k][l];
        if (fabsf(p) <= eps) break;
        const float y = (W[l] - W[k]) * 0.5f;
        float t = fabsf(y) + glibc_hypotf(p, y);          // std::hypot of floats on the host: see glibc_hypotf
        float s = glibc_hypotf(p, t);
        const float c = t / s;
        s = p / s; t = (p / t) * p;
        if (y < 0.0f) { s = -s; t = -t; }
        A[k][l] = 0.0f;
        W[k] -= t; W[l] += t;
#define S2M_ROT(v0, v1) do { const float a0 = (v0), b0 = (v1); (v0) = a0 * c - b0 * s; (v1) = a0 * s + b0 * c; } while (0)
        for (int i = 0; i < k; i++)     S2M_ROT(A[i][k], A[i][l]);
        for (int i = k + 1; i < l; i++) S2M_ROT(A[k][i], A[i][l]);
        for (int i = l + 1; i < N; i++) S2M_ROT(A[k][i], A[l][i]);
        for (int i = 0; i < N; i++)     S2M_ROT(V[k][i], V[l][i]);
#undef S2M_ROT
        for (int j = 0; j < 2; j++) {
            const int idx = j == 0 ? k : l;
            if (idx < N - 1) {
                int m = idx + 1; float mv2 = fabsf(A[idx][m]);
                for (int i = idx + 2; i < N; i++) { float v = fabsf(A[idx][i]); if (mv2 < v) { mv2 = v; m = i; } }
                indR[idx] = m;
            }
            if (idx > 0) {
                int m = 0; float mv2 = fabsf(A[0][idx]);
                for (int i = 1; i < idx; i++) { float v = fabsf(A[i][idx]); if (mv2 < v) { mv2 = v; m = i; } }
                indC[idx] = m;
            }
        }
    }
    for (int k = 0; k < N - 1; k++) {
        int m = k;
        for (int i = k + 1; i < N; i++) if (W[m] < W[i]) m = i;
        if (k != m) {
            float tw = W[m]; W[m] = W[k]; W[k] = tw;
            for (int i = 0; i < N; i++) { float tv = V[m][i]; V[m][i] = V[k][i]; V[k][i] = tv; }
        }
    }
}

// cv::Mat::inv() (:1263): LU with partial pivoting applied to [A | I], fp32. A is destroyed.
__device__ bool inv6_lu(float (*A)[6], float (*B)[6])
{
    constexpr int N = 6;
    const float eps = FLT_EPSILON * 10.0f;
    for (int i = 0; i < N; i++) for (int j = 0; j < N; j++) B[i][j] = (i == j) ? 1.0f : 0.0f;
    for (int i = 0; i < N; i++) {
        int k = i;
        for (int j = i + 1; j < N; j++) if (fabsf(A[j][i]) > fabsf(A[k][i])) k = j;
        if (fabsf(A[k][i]) < eps) {
            for (int a = 0; a < N; a++) for (int b = 0; b < N; b++) B[a][b] = 0.0f;
            return false;
        }
        if (k != i) {
            for (int j = i; j < N; j++) { float t = A[i][j]; A[i][j] = A[k][j]; A[k][j] = t; }
            for (int j = 0; j < N; j++) { float t = B[i][j]; B[i][j] = B[k][j]; B[k][j] = t; }
        }
        const float d = -1.0f / A[i][i];
        for (int j = i + 1; j < N; j++) {
            const float alpha = A[j][i] * d;
            for (int m = i + 1; m < N; m++) A[j][m] += alpha * A[i][m];
            for (int m = 0; m < N; m++) B[j][m] += alpha * B[i][m];
        }
    }
    for (int i = N - 1; i >= 0; i--)
        for (int j = 0; j < N; j++) {
            float s = B[i][j];
            for (int k = i + 1; k < N; k++) s -= A[i][k] * B[k][j];
            B[i][j] = s / A[i][i];
        }
    return true;
}

__device__ __forceinline__ void store_trace(gptr<s2m_iter_trace> dst, const s2m_iter_trace& tr)
{
    dst->n_sel = tr.n_sel; dst->stepped = tr.stepped; dst->deltaR = tr.deltaR; dst->deltaT = tr.deltaT;
#pragma unroll
    for (int k = 0; k < 6; k++) { dst->delta[k] = tr.delta[k]; dst->pose[k] = tr.pose[k]; }
}

// cv::solve(matAtA, matAtB, matX, DECOMP_QR) (:1240) spread over 7 lanes of one wave: lane j < 6
// owns column j of AtA, lane 6 the right-hand side.  Every number goes through exactly the operations,
// in the order, of OpenCV's hal::QR32f (un-pivoted Householder QR in fp32 with unit-length reflectors,
// the reflector kept as v/v[0] below the diagonal and re-expanded for the right-hand side, back
// substitution; OpenCV >= 3.3).  The code is branch-free and LDS-free: all lanes run the reflector
// arithmetic on their own column and lane l's result is broadcast with v_readlane.  The chain is bound
// by instruction issue (a wave64 instruction occupies the SIMD for 4 cycles however few lanes matter,
// a correctly rounded fp32 divide is ~10 instructions), so the independent divides of a reflector are
// spread over the lanes - lane i divides element i - and the quotients v[i]/v[0] (needed by lane l for
// storage and by lane 6 for the rhs) are computed once.  Returns x in every lane.
__device__ __forceinline__ float lane_bcast(float v, int src_lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane));
}

// element `idx` (0..5, per lane) of a register array as a select chain.  Left alone, the compiler recognises the chain
// as a dynamically indexed array and goes through scratch memory (a store and a dependent load: ~0.2 us each, twelve of
// them in the solve); the empty asm statements keep the selects apart.
__device__ __forceinline__ float pick6(const float (&a)[6], int idx)
{
    float r = a[0];
#pragma unroll
    for (int i = 1; i < 6; i++) {
        r = (idx == i) ? a[i] : r;
        asm volatile("" : "+v"(r));
    }
    return r;
}

__device__ __forceinline__ bool solve6_qr_lanes(int lane, float (&col)[6], float (&x)[6])
{
    const int li = min(lane, 5);
#pragma unroll
    for (int l = 0; l < 6; l++) {
        // column l lives in lane l: bring its tail and the two norms to every lane
        float vl[6], u[6];
        float nrm = 0.0f;
#pragma unroll
        for (int i = 0; i < 6 - l; i++) { vl[i] = col[l + i]; nrm += vl[i] * vl[i]; }
        const float tmpV = vl[0];
        vl[0] = vl[0] + (vl[0] >= 0.0f ? 1.0f : -1.0f) * sqrtf(nrm);
        nrm = sqrtf(nrm + vl[0] * vl[0] - tmpV * tmpV);
        nrm = lane_bcast(nrm, l);
#pragma unroll
        for (int i = 0; i < 6; i++) vl[i] = (i < 6 - l) ? lane_bcast(vl[i], l) : 0.0f;
        // the 6-l divides by the norm, one per lane, then the 5-l quotients v[i]/v[0], one per lane
        const float q = pick6(vl, li) / nrm;
#pragma unroll
        for (int i = 0; i < 6 - l; i++) vl[i] = lane_bcast(q, i);
        const float hf = vl[0] * vl[0];
        const float qu = pick6(vl, li) / vl[0];
        u[0] = 1.0f;
#pragma unroll
        for (int i = 1; i < 6 - l; i++) u[i] = lane_bcast(qu, i);
        // columns l..5: A -= 2 v (v^T A); the rhs (lane 6) gets the same reflector rebuilt from its stored
        // form, col -= ((2 u) (u^T col)) hf.  One dot product per lane, on the vector that lane needs.
        const bool is_col = lane >= l && lane < 6, is_rhs = lane == 6;
        float w[6], dot = 0.0f;
#pragma unroll
        for (int i = l; i < 6; i++) { w[i - l] = is_rhs ? u[i - l] : vl[i - l]; dot += w[i - l] * col[i]; }
#pragma unroll
        for (int i = l; i < 6; i++) {
            const float t = 2.0f * w[i - l] * dot;
            const float c = col[i] - (is_rhs ? t * hf : t);
            col[i] = (is_col || is_rhs) ? c : col[i];
        }
#pragma unroll
        for (int i = 1; i < 6 - l; i++) col[l + i] = (lane == l) ? u[i] : col[l + i];
    }
    // back substitution on wave-uniform values: R[i][j] = column j's entry i, b = lane 6's column
    bool ok = true;
    float b[6];
#pragma unroll
    for (int i = 0; i < 6; i++) b[i] = lane_bcast(col[i], 6);
#pragma unroll
    for (int i = 5; i >= 0; i--) {
#pragma unroll
        for (int j = 5; j > i; j--) b[i] -= b[j] * lane_bcast(col[i], j);
        const float d = lane_bcast(col[i], i);
        if (fabsf(d) < FLT_EPSILON * 10.0f) ok = false;
        b[i] /= d;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) x[i] = ok ? b[i] : 0.0f;
    return ok;
}

// Is every eigenvalue of the symmetric 6x6 A safely above `thresh`?  Cholesky of A - s*I in
// fp64 with s = thresh + margin, margin = 1e-5 * trace(A) (far above the fp32 Jacobi's error of a
// few ulp of the largest eigenvalue, far below any eigenvalue that matters): if it succeeds,
// cv::eigen would report all six eigenvalues >= thresh and isDegenerate stays false (:1251-1262).
__device__ bool all_eigen_above(const float* A, float thresh)
{
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) tr += (double)A[i * 6 + i];
    if (!(tr > 0.0) || !(tr < 1.0e30)) return false;
    const double sft = (double)thresh + 1e-5 * tr;
    double L[6][6];
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double d = (double)A[j * 6 + j] - sft;
#pragma unroll
        for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k];
        if (!(d > 1e-9 * tr)) return false;
        const double dj = sqrt(d);
        L[j][j] = dj;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double v = (double)A[i * 6 + j];
#pragma unroll
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k];
            L[i][j] = v / dj;
        }
    }
    return true;
}

// ------------------------------------------------------------------------------------------
// The rest of LMOptimization (:1177-1292) after the per-point work: second stage of the
// AtA/AtB reduction (fixed order: bitwise reproducible for a given workgroup partition and
// workgroup size), the 6x6 solve, the iteration-0 degeneracy analysis, the pose update and the
// convergence test.  Two callers share it:
//   * k_finalize (one workgroup of 1024) closes iteration 0, which needs the degeneracy
//     analysis, and the last iteration of a scan;
//   * k_register closes iteration L-1 in the prologue of launch L >= 2: every workgroup reduces
//     the previous launch's partial sums and solves the 6x6 system for itself (same numbers in
//     the same order, so every workgroup arrives at the same pose), and workgroup 0 records
//     the outcome.  That removes a kernel boundary and a single-workgroup kernel from every
//     iteration of the loop (:1304-1315); the few microseconds of redundant algebra overlap
//     with the loads of the scan points and their priors.
// Loop state is double-buffered by launch parity so that nothing read in a launch is written
// in it: launch L uses the pose in pose2[L & 1] and writes its partial sums to slot L & 1.
// ------------------------------------------------------------------------------------------
struct LmShared {
    double part[kFinThreads / 32][32];
    double tot[32];
    float  AtA[36], AtB[6];
    float  eA[6][6], eV[6][6], eVi[6][6], eV2[6][6], eW[6];      // iteration-0 analysis only
    int    eR[6], eC[6];
};

// Closes iteration `iter`: matAtA / matAtB / laserCloudSelNum from the partial sums of launch `iter`
// (:1182-1239), then solve, project, update, test (:1177-1180, :1240-1292).  `pose0` is the pose launch
// `iter` ran with, `nb_act` the number of workgroups that wrote partial sums.  All NT threads of the
// workgroup call it; after the first barrier wave 0 works alone (wave-level LDS ordering only) and
// publishes {pose[6], ended} in `s_out` (8 floats of LDS that outlive `sh`); all threads return the
// updated pose in pose_out and whether the loop has ended (converged with early exit on, or fewer
// than min_corr correspondences).  kFull adds the iteration-0 degeneracy analysis on wave 1.
// `writer` records the outcome in DevState / trace.  ne_only = normal equations only (observation hook).
// `early` / `late`: work of the caller that does not depend on the pose and hides behind the serial part - called by every
// thread once the partial sums are in (everything requested before the call has arrived by then), and again just before
// the last barrier (wave 0: after the solve; the other waves: at once, they would only wait there).
// The partial sums are asked for ahead of the call, as soon as the head of the launch is in (lm_request_rows: the first 16 rows
// of each lane, which is all of them up to 16 * NT / 32 workgroups), so that they travel together with the caller's own first
// requests; `lp`: the parameters of the tests at the end, read with the head as well.
struct LmRows { double v[16]; };
template <int NT>
__device__ __forceinline__ void lm_request_rows(const CtxHead& ch, int nb_act, int iter, LmRows& r)
{
    constexpr int NG = NT / 32;
    const int t = threadIdx.x, col = t & 31, grp = t >> 5;
    const auto P = G((const double*)ch.partials) + (size_t)(iter & 1) * (size_t)ch.nblocks * kAcc;
    const int nb = min(ch.nblocks, nb_act);             // active workgroups
#pragma unroll
    for (int u = 0; u < 16; u++) { const int b = grp + u * NG; r.v[u] = (col < kAcc && b < nb) ? P[(size_t)b * kAcc + col] : 0.0; }
}
struct NoHook { __device__ __forceinline__ void operator()() const {} };
template <int NT, bool kFull, typename Early = NoHook, typename Late = NoHook>
__device__ __forceinline__ bool lm_close_iteration(CtxP cp, gptr<DevState> st, const CtxHead& ch, const LmParams& lp, const LmRows& rows,
                                                   int nb_act, int iter,
                                                   bool writer, bool ne_only, const float (&pose0)[6], int degen0,
                                                   LmShared& sh, float* s_out, float (&pose_out)[6],
                                                   unsigned long long* stamps = nullptr,     // diagnostics: 5 wall-clock stamps
                                                   Early early = Early(), Late late = Late())
{
    constexpr int NG = NT / 32;                         // row groups
    const auto trace = G(cp->trace);
    const int t = threadIdx.x, col = t & 31, grp = t >> 5, lane = t & 63, wave = t >> 6;
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < 16; u++) s += rows.v[u];        // (rows that do not exist, and the columns past kAcc, are 0.0: s stays what it was)
    if (col < kAcc) {
        const int nbk = ch.nblocks;
        const auto P = G((const double*)ch.partials) + (size_t)(iter & 1) * (size_t)nbk * kAcc;
        const int nb = min(nbk, nb_act);                // active workgroups
        for (int b0 = grp + 16 * NG; b0 < nb; b0 += 16 * NG) {    // 16 independent loads in flight per lane
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; u++) { const int b = b0 + u * NG; v[u] = (b < nb) ? P[(size_t)b * kAcc + col] : 0.0; }
#pragma unroll
            for (int u = 0; u < 16; u++) s += v[u];
        }
    }
    sh.part[grp][col] = s;
    __syncthreads();
    if (stamps) stamps[0] = wall_clock64();
    early();

    int n_sel = 0;
    if (wave == 0) {
        if (t < kAcc) {
            double v = 0.0;
#pragma unroll
            for (int g2 = 0; g2 < NG; g2++) v += sh.part[g2][t];
            sh.tot[t] = v;
        }
        wave_lds_sync();
        // fp32 matrices (:1184-1186): entry (a, b), a <= b, is sum number a*6 - a(a-1)/2 + (b-a)
        n_sel = (int)sh.tot[27];
        if (t < 36) {
            const int a = min(t / 6, t % 6), b = max(t / 6, t % 6);
            const float v = (float)sh.tot[a * 6 - (a * (a - 1)) / 2 + (b - a)];
            sh.AtA[t] = v;
            if (writer) st->AtA[t] = v;
        } else if (t < 42) {
            const float v = (float)sh.tot[21 + (t - 36)];
            sh.AtB[t - 36] = v;
            if (writer) st->AtB[t - 36] = v;
        }
        if (writer && t == 0) st->n_sel_last = n_sel;
        wave_lds_sync();
    }
    if (stamps) stamps[1] = wall_clock64();
    if (ne_only) return false;

    if (kFull && iter == 0) {                           // :1242-1264, wave 1 lane 0
        __syncthreads();
        if (wave == 1 && lane == 0 && (int)sh.tot[27] >= lp.min_corr) {
            int degenerate = 0;
            if (!all_eigen_above(sh.AtA, cp->eig_thresh)) {
                // the full restatement: cv::eigen, the row-zeroing loop, matP = matV.inv() * matV2
                for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) sh.eA[i][j] = sh.AtA[i * 6 + j];
                eigen6_sym(sh.eA, sh.eV, sh.eW, sh.eR, sh.eC);
                for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) sh.eV2[i][j] = sh.eV[i][j];
                for (int i = 5; i >= 0; i--) {
                    if (sh.eW[i] < cp->eig_thresh) { for (int j = 0; j < 6; j++) sh.eV2[i][j] = 0.0f; degenerate = 1; }
                    else break;
                }
                for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) sh.eA[i][j] = sh.eV[i][j];
                inv6_lu(sh.eA, sh.eVi);
                for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) {      // matP = matV.inv() * matV2
                    double a = 0.0;
                    for (int k = 0; k < 6; k++) a += (double)sh.eVi[i][k] * (double)sh.eV2[k][j];
                    st->matP[i * 6 + j] = (float)a;
                }
            }
            // not degenerate: matP is never read before the next scan's iteration 0 rewrites it
            st->isDegenerate = degenerate;
            __threadfence_block();
        }
        __syncthreads();                                // thread 0 reads what wave 1 decided
    }

    if (wave == 0) {
        if (n_sel < lp.min_corr) {                     // :1178-1180: false, pose unchanged
            if (t == 0) {
                if (writer) {
                    s2m_iter_trace tr;
                    tr.n_sel = n_sel; tr.stepped = 0; tr.deltaR = 0.0f; tr.deltaT = 0.0f;
#pragma unroll
                    for (int k = 0; k < 6; k++) { tr.pose[k] = pose0[k]; tr.delta[k] = 0.0f; st->pose[k] = pose0[k]; }
                    st->stalled = 1; st->done = 1;      // the remaining iterations repeat this no-op
                    st->iters_run = cp->max_iter;
                    store_trace(trace + iter, tr);
                }
#pragma unroll
                for (int k = 0; k < 6; k++) s_out[k] = pose0[k];
                s_out[6] = 1.0f;
            }
        } else {
            float colv[6], X[6];
#pragma unroll
            for (int i = 0; i < 6; i++) colv[i] = (lane < 6) ? sh.AtA[i * 6 + lane] : ((lane == 6) ? sh.AtB[i] : 0.0f);
            solve6_qr_lanes(lane, colv, X);             // :1240, result in every lane
            if (stamps) stamps[2] = wall_clock64();
            if (t == 0) {                               // projection, pose update, convergence test (:1266-1292)
                float pose[6];
#pragma unroll
                for (int k = 0; k < 6; k++) pose[k] = pose0[k];
                if ((kFull && iter == 0) ? (st->isDegenerate != 0) : (degen0 != 0)) {   // :1266-1271 (iteration 0: just decided by wave 1)
                    float X2[6];
#pragma unroll
                    for (int k = 0; k < 6; k++) X2[k] = X[k];
                    for (int i = 0; i < 6; i++) {
                        double a = 0.0;
                        for (int k = 0; k < 6; k++) a += (double)st->matP[i * 6 + k] * (double)X2[k];
                        X[i] = (float)a;
                    }
                }
#pragma unroll
                for (int k = 0; k < 6; k++) { pose[k] += X[k]; s_out[k] = pose[k]; }        // :1273-1278
                const double r0 = (double)(X[0] * 57.29578f), r1 = (double)(X[1] * 57.29578f), r2 = (double)(X[2] * 57.29578f);
                const float deltaR = (float)sqrt(r0 * r0 + r1 * r1 + r2 * r2);          // :1280-1283
                const double t0 = (double)(X[3] * 100), t1 = (double)(X[4] * 100), t2 = (double)(X[5] * 100);
                const float deltaT = (float)sqrt(t0 * t0 + t1 * t1 + t2 * t2);          // :1284-1287
                const bool conv = ((double)deltaR < lp.conv_deg) && ((double)deltaT < lp.conv_cm);   // :1289
                s_out[6] = (conv && lp.early_exit) ? 1.0f : 0.0f;                      // break (:1313-1314)
                if (writer) {
                    s2m_iter_trace tr;
                    tr.n_sel = n_sel; tr.stepped = 1; tr.deltaR = deltaR; tr.deltaT = deltaT;
#pragma unroll
                    for (int k = 0; k < 6; k++) { tr.delta[k] = X[k]; tr.pose[k] = pose[k]; }
                    // launch iter+1 rebuilds its transform from this pose (k_register prologue)
#pragma unroll
                    for (int k = 0; k < 6; k++) { st->pose[k] = pose[k]; st->pose2[(iter + 1) & 1][k] = pose[k]; }
                    st->T_valid = 0;
                    store_trace(trace + iter, tr);
                    st->iters_run = iter + 1;
                    if (conv) st->converged = 1;           // (no test of the old value: a load here would first drain the stores above)
                    if (conv && lp.early_exit) st->done = 1;
                }
            }
        }
    }
    if (stamps) stamps[3] = wall_clock64();
    late();
    __syncthreads();
    if (stamps) stamps[4] = wall_clock64();
#pragma unroll
    for (int k = 0; k < 6; k++) pose_out[k] = s_out[k];
    return s_out[6] != 0.0f;
}

// ------------------------------------------------------------------------------------------
// Density-aware re-split of the wave table, once per scan before launch 0.  k_chunk_parts can only
// look at the extent of a chunk in the lidar frame; how many map points fall into a wave's box is
// known once the initial guess is.  All workgroups start together, so a launch lasts as long as its
// slowest wave, and the slowest waves are the few whose box covers a dense part of the map (they
// stage and sweep a large tile, or overflow it and fall back to the gather path).  One wave per
// table entry transforms its points with the initial guess and sums the cell ranges of its box rows
// (what launch 0 will stream); only the heavy tail asks for its chunk to be cut 2, 4 or 8 times
// finer (the chunk is sorted along its longest axis, so the parts are compact), and
// k_chunk_table_density rebuilds the table.  Partition only: results do not depend on it beyond the
// summation order of the normal equations.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_wave_density(const SlotTable tbl, int raw_limit)
{
    const CtxP cp = ctx_const(tbl.ctx[blockIdx.y]);
    const auto st = G((const DevState*)tbl.st[blockIdx.y]);
    const int lane = threadIdx.x & 63;
    const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (!cp->density_pending || wv >= st->n_waves) return;   // the table of a scan is re-split once, at its first optimisation
    const auto tb = G((const int2*)cp->wave_table);
    const int2 e = make_int2(tb[wv].x, tb[wv].y);
    const int i = e.x + lane;
    const bool valid = lane < e.y && i < cp->n_q;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    if (valid) {
        const float px = G(cp->qx)[i], py = G(cp->qy)[i], pz = G(cp->qz)[i];
        sx = ((st->T[0] * px + st->T[1] * py) + st->T[2]  * pz) + st->T[3];
        sy = ((st->T[4] * px + st->T[5] * py) + st->T[6]  * pz) + st->T[7];
        sz = ((st->T[8] * px + st->T[9] * py) + st->T[10] * pz) + st->T[11];
    }
    const bool fin = valid && (fabsf(sx) < 3.0e38f) && (fabsf(sy) < 3.0e38f) && (fabsf(sz) < 3.0e38f);
    const float mnx = wave_min_f32(fin ? sx : INFINITY), mxx = wave_max_f32(fin ? sx : -INFINITY);
    const float mny = wave_min_f32(fin ? sy : INFINITY), mxy = wave_max_f32(fin ? sy : -INFINITY);
    const float mnz = wave_min_f32(fin ? sz : INFINITY), mxz = wave_max_f32(fin ? sz : -INFINITY);
    if (!(mnx <= mxx)) return;
    const GridDesc g = grid_of(cp);
    const auto cell_start = G(cp->cell_start);
    const int bx0 = max(cell_coord(mnx, g.ox, g.inv_e, g.nx) - 1, 0), bx1 = min(cell_coord(mxx, g.ox, g.inv_e, g.nx) + 1, g.nx - 1);
    const int by0 = max(cell_coord(mny, g.oy, g.inv_e, g.ny) - 1, 0), by1 = min(cell_coord(mxy, g.oy, g.inv_e, g.ny) + 1, g.ny - 1);
    const int bz0 = max(cell_coord(mnz, g.oz, g.inv_e, g.nz) - 1, 0), bz1 = min(cell_coord(mxz, g.oz, g.inv_e, g.nz) + 1, g.nz - 1);
    const int nyb = by1 - by0 + 1, nzb = bz1 - bz0 + 1;
    if (nyb * nzb > kRowMax) return;                      // scattered points: the gather path's business, a finer cut does not help
    int raw = 0;
    for (int r = lane; r < nyb * nzb; r += 64) {
        const int zq = r / nyb;
        const int gcell = ((bz0 + zq) * g.ny + by0 + (r - zq * nyb)) * g.nx;
        raw += cell_start[gcell + bx1 + 1] - cell_start[gcell + bx0];
    }
    raw = __builtin_amdgcn_readlane(wave_incl_scan_i32(raw), 63);
    int f = raw <= raw_limit ? 1 : (raw <= 2 * raw_limit ? 2 : (raw <= 4 * raw_limit ? 4 : 8));
    f = min(f, max(e.y / 8, 1));                          // at least 8 points per wave
    if (lane == 0 && f > 1) atomicMax(&cp->chunk_factor[e.x >> 6], f);
}

// The same wishes for a single scan's first optimisation, without a wave table in front of it and with the state upload
// folded in (a plain launch ahead of the captured loop: the DevCtx block and the loop state travel as kernel arguments).
//   * One wave per 64-point CHUNK.  The extent-only table k_chunk_table would emit gives chunk c  p = min(parts[c], cap)
//     entries of 64 / p points, cap = the first of 8, 4, 2, 1 under which the wishes fit the table (chunk_table_body without
//     density wishes: policies 0-2, 3 / 6, 4 / 7, 5 / 8); every workgroup adds the four totals up for itself.
//   * A part is a contiguous range of 64 / p lanes: segmented butterflies give every part its box, its row sum and its wish
//     under k_wave_density's rules, and the chunk's wish is the maximum over its parts - what the per-entry atomicMax leaves.
//   * Every wave takes the transform and the context fields from the arguments; one workgroup more than the chunks need (the
//     last) stores both blocks and the start stamp as k_set_ctx_state does, beside the waves that work on chunks (n_waves of
//     the state is set by k_chunk_table_density, the next kernel).
//   * The points are fetched and transformed before the totals are added up: the two round trips overlap.
struct DensityStateArgs {
    DevCtx c; DevState v;
    DevCtx* cdst; DevState* sdst;
    unsigned long long* stamp;    // pinned, may be null
    int32_t raw_limit;
};
__global__ __launch_bounds__(256) void k_wave_density_state(const DensityStateArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == gridDim.x - 1) {                    // (uniform: the workgroup behind the chunks')
        if (threadIdx.x == 0) {
            *a.cdst = a.c;
            DevState v = a.v;
            v.n_waves = 0;
            *a.sdst = v;
            if (a.stamp) *a.stamp = wall_clock64();
        }
        return;
    }
    const int n = a.c.n_q, n_chunks = a.c.n_chunks, capacity = a.c.table_cap;
    const auto parts = G(a.c.chunk_parts);
    const int c = blockIdx.x * 4 + wave;
    const int i = c * 64 + lane;
    const bool valid = c < n_chunks && i < n;
    const int own_parts = c < n_chunks ? parts[c] : 1;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    if (valid) {
        const float px = G(a.c.qx)[i], py = G(a.c.qy)[i], pz = G(a.c.qz)[i];
        sx = ((a.v.T[0] * px + a.v.T[1] * py) + a.v.T[2]  * pz) + a.v.T[3];
        sy = ((a.v.T[4] * px + a.v.T[5] * py) + a.v.T[6]  * pz) + a.v.T[7];
        sz = ((a.v.T[8] * px + a.v.T[9] * py) + a.v.T[10] * pz) + a.v.T[11];
    }
    // the cap of the extent-only table
    __shared__ int32_t tot_s[4][4];
    int t8 = 0, t4 = 0, t2 = 0, t1 = 0;
    for (int k = threadIdx.x; k < n_chunks; k += 256) {
        const int p = parts[k];
        t8 += min(p, 8); t4 += min(p, 4); t2 += min(p, 2); t1 += min(p, 1);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        t8 += __shfl_xor(t8, off, 64); t4 += __shfl_xor(t4, off, 64); t2 += __shfl_xor(t2, off, 64); t1 += __shfl_xor(t1, off, 64);
    }
    if (lane == 0) { tot_s[wave][0] = t8; tot_s[wave][1] = t4; tot_s[wave][2] = t2; tot_s[wave][3] = t1; }
    __syncthreads();
    t8 = tot_s[0][0] + tot_s[1][0] + tot_s[2][0] + tot_s[3][0];
    t4 = tot_s[0][1] + tot_s[1][1] + tot_s[2][1] + tot_s[3][1];
    t2 = tot_s[0][2] + tot_s[1][2] + tot_s[2][2] + tot_s[3][2];
    const int cap = t8 <= capacity ? 8 : (t4 <= capacity ? 4 : (t2 <= capacity ? 2 : 1));
    if (c >= n_chunks) return;
    const int p = min(own_parts, cap);                    // 1, 2, 4 or 8
    const int per = 64 / p;
    const int start = c * 64 + (lane / per) * per;        // the part's table entry: {start, cnt}
    const int cnt = max(0, min(per, n - start));          // (a lane is inside its entry's count  <=>  i < n: valid)
    const bool fin = valid && (fabsf(sx) < 3.0e38f) && (fabsf(sy) < 3.0e38f) && (fabsf(sz) < 3.0e38f);
    float mnx = fin ? sx : INFINITY, mxx = fin ? sx : -INFINITY;
    float mny = fin ? sy : INFINITY, mxy = fin ? sy : -INFINITY;
    float mnz = fin ? sz : INFINITY, mxz = fin ? sz : -INFINITY;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        if (off < per) {                                  // (uniform over the wave)
            mnx = fminf(mnx, __shfl_xor(mnx, off, 64)); mxx = fmaxf(mxx, __shfl_xor(mxx, off, 64));
            mny = fminf(mny, __shfl_xor(mny, off, 64)); mxy = fmaxf(mxy, __shfl_xor(mxy, off, 64));
            mnz = fminf(mnz, __shfl_xor(mnz, off, 64)); mxz = fmaxf(mxz, __shfl_xor(mxz, off, 64));
        }
    }
    bool ok = mnx <= mxx;                                 // the part has a finite point
    GridDesc g;
    g.ox = a.c.g.ox; g.oy = a.c.g.oy; g.oz = a.c.g.oz; g.inv_e = a.c.g.inv_e; g.e = a.c.g.e;
    g.nx = a.c.g.nx; g.ny = a.c.g.ny; g.nz = a.c.g.nz; g.ncells = a.c.g.ncells;
    const auto cell_start = G(a.c.cell_start);
    int raw = 0;
    if (ok) {
        const int bx0 = max(cell_coord(mnx, g.ox, g.inv_e, g.nx) - 1, 0), bx1 = min(cell_coord(mxx, g.ox, g.inv_e, g.nx) + 1, g.nx - 1);
        const int by0 = max(cell_coord(mny, g.oy, g.inv_e, g.ny) - 1, 0), by1 = min(cell_coord(mxy, g.oy, g.inv_e, g.ny) + 1, g.ny - 1);
        const int bz0 = max(cell_coord(mnz, g.oz, g.inv_e, g.nz) - 1, 0), bz1 = min(cell_coord(mxz, g.oz, g.inv_e, g.nz) + 1, g.nz - 1);
        const int nyb = by1 - by0 + 1, nzb = bz1 - bz0 + 1;
        ok = nyb * nzb <= kRowMax;                        // scattered points: the gather path's business, a finer cut does not help
        if (ok) {
            for (int r = lane & (per - 1); r < nyb * nzb; r += per) {
                const int zq = r / nyb;
                const int gcell = ((bz0 + zq) * g.ny + by0 + (r - zq * nyb)) * g.nx;
                raw += cell_start[gcell + bx1 + 1] - cell_start[gcell + bx0];
            }
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        if (off < per) raw += __shfl_xor(raw, off, 64);   // (ok is uniform over a part: its lanes hold the same box)
    }
    const int raw_limit = a.raw_limit;
    int f = raw <= raw_limit ? 1 : (raw <= 2 * raw_limit ? 2 : (raw <= 4 * raw_limit ? 4 : 8));
    f = min(f, max(cnt / 8, 1));                          // at least 8 points per wave
    f = ok ? f : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) f = max(f, __shfl_xor(f, off, 64));
    if (lane == 0 && f > 1) a.c.chunk_factor[c] = f;      // (zero between uses: what atomicMax over the entries would leave)
}

#include "s2m_register.hpp"

// ------------------------------------------------------------------------------------------
// k_finalize: one workgroup closing iteration `iter` on its own (lm_close_iteration above):
// iteration 0 with the degeneracy analysis, and the last iteration of a scan (or every iteration
// when the grid is too large for the fused form).  mode 1 = normal equations only (observation hook).
// The k_finalize that ends a range of launches of a captured single-scan loop is given `out`, the pinned mirror the host reads
// the loop's record from (DevState, then the max_iter trace records that lie behind it on the device as well): all its threads
// copy the record there, also when the loop had ended before this launch - a copy node behind the kernel would be one more
// trip through the queue (as k_sc_detect's result; the kernel's completion makes the stores visible to the host).
// `stamp` (pinned, may be null): the wall clock once every thread has issued its part of the copy, the end of the loop for
// s2m_last_timing.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void finalize_record_out(gptr<DevState> st, DevState* out, int max_iter, unsigned long long* stamp)
{
    static_assert(sizeof(DevState) % 4 == 0 && sizeof(s2m_iter_trace) % 4 == 0, "the record is copied word by word");
    if (out) {
        const auto src = (gptr<const uint32_t>)st;
        const auto dst = G(reinterpret_cast<uint32_t*>(out));
        const int nw = (int)((sizeof(DevState) + sizeof(s2m_iter_trace) * (size_t)max_iter) / 4);
        for (int k = threadIdx.x; k < nw; k += kFinThreads) dst[k] = src[k];
    }
    if (stamp) {
        __syncthreads();                                  // (uniform: a kernel argument)
        if (threadIdx.x == 0) *stamp = wall_clock64();
    }
}

__global__ __launch_bounds__(kFinThreads) void k_finalize(const SlotTable tbl, int iter, int mode, DevState* out, unsigned long long* stamp)
{
    const CtxP cp = ctx_const(tbl.ctx[blockIdx.y]);
    const auto st = G(tbl.st[blockIdx.y]);
    // loop state and the head of DevCtx, fetched up front (the state block is a kernel argument: no pointer chase through DevCtx)
    CtxHead ch; StateHead hs;
    load_heads(cp, st, iter & 1, ch, hs, iter, mode);
    LmParams lp = lm_params(cp);
    const int wpb = cp->wpb, max_iter = cp->max_iter;
    const int done0 = hs.done, degen0 = hs.isDegenerate;
    const int nb_act = (hs.n_waves + wpb - 1) / wpb;
    float pose0[6];
#pragma unroll
    for (int k = 0; k < 6; k++) pose0[k] = hs.pose[k];
    if (mode == 0 && done0) { finalize_record_out(st, out, max_iter, stamp); return; }
    LmRows rows;
    lm_request_rows<kFinThreads>(ch, nb_act, iter, rows);
    asm volatile("" : "+s"(lp.min_corr), "+s"(lp.early_exit), "+s"(lp.conv_deg), "+s"(lp.conv_cm));   // (here, not at the end of the serial part)
    __shared__ LmShared sh;
    __shared__ float s_out[8];
    // the worklists of the search kernel start empty behind every close of its own (the certify kernel of the next launch appends)
    if (mode == 0 && threadIdx.x == 0 && cp->wl_count) { cp->wl_count[0] = 0; cp->wl_count[1] = 0; }
    float pose[6];
    const bool ended = lm_close_iteration<kFinThreads, true>(cp, st, ch, lp, rows, nb_act, iter, true, mode == 1, pose0, degen0, sh, s_out, pose);
    // the transform of the new pose, once, for every workgroup of the next registration launch (which would otherwise
    // rebuild it - a microsecond of dependent trig arithmetic in each of them)
    if (mode == 0 && !ended && threadIdx.x < 64) {
        float T[12], sc6[6];
        build_transform(pose, (int)threadIdx.x, T, sc6);
        if (threadIdx.x == 0 && !st->stalled) {
#pragma unroll
            for (int k = 0; k < 12; k++) st->T[k] = T[k];
#pragma unroll
            for (int k = 0; k < 6; k++) st->sc[k] = sc6[k];
            st->T_valid = 1;
        }
    }
    if (out || stamp) {
        __syncthreads();                                  // what thread 0 and wave 1 stored above is part of the record
        finalize_record_out(st, out, max_iter, stamp);
    }
}

// Parameter blocks travel as kernel arguments (copied at launch), so the host never has to
// keep a staging buffer alive or synchronise to update them.
__global__ void k_set_ctx(DevCtx* dst, DevCtx v) { if (threadIdx.x == 0 && blockIdx.x == 0) *dst = v; }
// The wave count of the resident scan (left by k_chunk_table) is folded into the state block here.
// the DevCtx block and the loop state of a scan in one launch (s2m_optimize: both change with every scan)
// `stamp` (pinned, may be null): the wall clock once the state is stored, the start of the loop for s2m_last_timing
__global__ void k_set_ctx_state(DevCtx* cdst, DevCtx c, DevState* dst, DevState v, const int32_t* n_waves, unsigned long long* stamp)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) { *cdst = c; v.n_waves = n_waves ? *n_waves : 0; *dst = v; if (stamp) *stamp = wall_clock64(); }
}

// the same for the scan slots of a batch: one launch for all of them (blockIdx.x = slot)
__global__ void k_set_ctxs(const CtxTable t) { if (threadIdx.x == 0 && t.dst[blockIdx.x]) *t.dst[blockIdx.x] = t.v[blockIdx.x]; }
__global__ __launch_bounds__(256) void k_init_states(const StateInitTable t)
{
    const StateInit& si = t.s[blockIdx.x];
    if (!si.dst) return;
    float* w = reinterpret_cast<float*>(si.dst);
    for (int k = threadIdx.x; k < (int)(sizeof(DevState) / 4); k += blockDim.x) w[k] = 0.0f;
    __syncthreads();
    if (threadIdx.x == 0) {
        DevState* d = si.dst;
        for (int k = 0; k < 6; k++) { d->pose[k] = si.pose[k]; d->pose2[0][k] = si.pose[k]; d->sc[k] = si.sc[k]; }
        for (int k = 0; k < 12; k++) d->T[k] = si.T[k];
        for (int k = 0; k < 36; k++) d->matP[k] = si.matP[k];
        d->isDegenerate = si.isDegenerate;
        d->T_valid = 1;
        d->n_waves = si.n_waves ? *si.n_waves : 0;
    }
}

__global__ void k_set_state(DevState* dst, DevState v, const int32_t* n_waves, unsigned long long* stamp)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) { v.n_waves = n_waves ? *n_waves : 0; *dst = v; if (stamp) *stamp = wall_clock64(); }
}

}  // namespace s2m
