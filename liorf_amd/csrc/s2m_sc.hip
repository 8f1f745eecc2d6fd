// s2m_sc.hip — ScanContext on the device (SCManager, include/Scancontext.cpp): the descriptor and ring key of a cloud, the
// store by key-frame index, the loop detector and the batched distance, with the host functions that launch them.  The C ABI
// on top is s2m_abi_sc.hip's; the place query is a unit of its own (s2m_sc_query.hip) and shares s2m_sc_dist.hpp.
// Compiled with -ffp-contract=off; the restated atanf is s2m_device.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "s2m_context.hpp"
#include "s2m_device.hpp"
#include "s2m_sc_dist.hpp"          // kScThreads, kScShifts, ScShared, sc_distance_block: shared with the place query (s2m_sc_query.hip)
#include "s2m_sc.hpp"
#include "s2m_sc_keys.hpp"          // sc_ring_key, sc_sector_key: shared with the host add and the session load

using namespace s2m;
using namespace s2m::host;

namespace s2m {

// ------------------------------------------------------------------------------------------
// ScanContext descriptor (include/Scancontext.cpp:151-211): max-z polar histogram, 20 rings x
// 60 sectors, LDS bins per workgroup merged with global atomicMax on an order-preserving
// integer image of fp32 z; ring key = row mean.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sc_polar_max(const unsigned char* __restrict__ pts, size_t stride, int n,
                                                      uint32_t* __restrict__ bins /*[1200], 0 = empty*/)
{
    __shared__ uint32_t lb[S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR];
    for (int k = threadIdx.x; k < S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR; k += blockDim.x) lb[k] = 0u;
    __syncthreads();
    const double kdeg = 180.0 / M_PI;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float* p = reinterpret_cast<const float*>(pts + (size_t)i * stride);
        const float x = p[0], y = p[1];
        const float z = (float)((double)p[2] + 2.0);                       // LIDAR_HEIGHT (:168)
        const float rng = sqrtf(x * x + y * y);                            // :171
        float th;                                                          // xy2theta (:23-36)
        if ((x >= 0) & (y >= 0))      th = (float)(kdeg * (double)glibc_atanf(y / x));
        else if ((x < 0) & (y >= 0))  th = (float)(180.0 - (kdeg * (double)glibc_atanf(y / (-x))));
        else if ((x < 0) & (y < 0))   th = (float)(180.0 + (kdeg * (double)glibc_atanf(y / x)));
        else if ((x >= 0) & (y < 0))  th = (float)(360.0 - (kdeg * (double)glibc_atanf((-y) / x)));
        else th = NAN;
        if ((double)rng > 80.0) continue;                                  // PC_MAX_RADIUS (:175)
        if (!(z == z)) continue;                                           // NaN z never wins desc < z
        const double rv = ceil(((double)rng / 80.0) * 20.0);               // :178
        const double sv = ceil(((double)th / 360.0) * 60.0);               // :179
        int ring = (rv != rv) ? 1 : (int)fmin(fmax(rv, 1.0), 20.0);
        int sect = (sv != sv) ? 1 : (int)fmin(fmax(sv, 1.0), 60.0);
        atomicMax(&lb[(ring - 1) * S2M_SC_NUM_SECTOR + (sect - 1)], f2ord(z));
    }
    __syncthreads();
    for (int k = threadIdx.x; k < S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR; k += blockDim.x)
        if (lb[k]) atomicMax(&bins[k], lb[k]);
}

__global__ __launch_bounds__(64) void k_sc_finish(const uint32_t* __restrict__ bins, double* __restrict__ desc,
                                                  double* __restrict__ ringkey)
{
    // one wave; lane r < 20 owns ring r
    const int r = threadIdx.x;
    if (r >= S2M_SC_NUM_RING) return;
    ringkey[r] = sc_ring_key([&](int k) {                                  // row mean (:198-211) of the values as they are stored
        const uint32_t u = bins[r * S2M_SC_NUM_SECTOR + k];
        double v = 0.0;                                                    // NO_POINT -> 0 (:187-190)
        if (u) {
            const uint32_t b = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
            const float z = __uint_as_float(b);
            // desc starts at -1000 and takes z only if -1000 < z (:182); -1000 -> 0 afterwards
            v = ((double)z > -1000.0) ? (double)z : 0.0;
        }
        desc[r * S2M_SC_NUM_SECTOR + k] = v;
        return v;
    });
}

// ------------------------------------------------------------------------------------------
// ScanContext matching (reference include/Scancontext.cpp:69-148,
// 214-344).  The SCManager's containers live on the device as three arrays indexed by key-frame
// number: descriptors [n][20*60] fp64 (ring-major), ring keys [n][20] fp32 (eig2stdvec, :62-66),
// sector keys [n][60] fp64.  Sizes are tiny (a descriptor is 9.6 KB), so one workgroup does a whole
// detectLoopClosureID(); the batched kernel runs one workgroup per candidate.  All sums run left to
// right in fp64 like the oracle's restatement, so distances are bit-identical to it.
// ------------------------------------------------------------------------------------------

// makeAndSaveScancontextAndKeys (:236-250): descriptor + ring key (as k_sc_finish left them) into slot `idx`
__global__ __launch_bounds__(kScThreads) void k_sc_append(const double* __restrict__ desc_ring, double* __restrict__ store_desc,
                                                          float* __restrict__ store_ring, double* __restrict__ store_sector, int idx)
{
    constexpr int NR = S2M_SC_NUM_RING, NS = S2M_SC_NUM_SECTOR;
    double* d = store_desc + (size_t)idx * NR * NS;
    for (int k = threadIdx.x; k < NR * NS; k += kScThreads) d[k] = desc_ring[k];
    if (threadIdx.x < NR) store_ring[(size_t)idx * NR + threadIdx.x] = (float)desc_ring[NR * NS + threadIdx.x];
    if (threadIdx.x < NS)                                                  // makeSectorkeyFromScancontext (:214-227)
        store_sector[(size_t)idx * NS + threadIdx.x] = sc_sector_key([&](int r) { return desc_ring[r * NS + threadIdx.x]; });
}

// distanceBtnScanContext of descriptor `query` against cand[0..m): one workgroup per candidate
__global__ __launch_bounds__(kScThreads) void k_sc_distance_batch(const double* __restrict__ store_desc, const double* __restrict__ store_sector,
                                                                  int query, const int32_t* __restrict__ cand, double* __restrict__ dist,
                                                                  int32_t* __restrict__ shift)
{
    __shared__ ScShared sh[1];
    __shared__ int s_cand[1];
    if (threadIdx.x == 0) s_cand[0] = cand[blockIdx.x];
    __syncthreads();
    sc_distance_block<1>(store_desc, store_sector, store_desc + (size_t)query * (S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR),
                         store_sector + (size_t)query * S2M_SC_NUM_SECTOR, s_cand, sh);
    if (threadIdx.x == 0) { dist[blockIdx.x] = sh[0].dist_out; shift[blockIdx.x] = sh[0].shift_out; }
}

// detectLoopClosureID (:253-344) for the newest descriptor (index n_total - 1) against the ring keys
// [0, n_search) (the contents of the reference's kd-tree at its last rebuild).  One workgroup: every thread keeps the three
// nearest of its share of the keys, the lists are merged by a butterfly inside each wave and by one thread over the four waves
// (order: distance, then index - the lower index wins a tie, whoever held it), then the three candidates are compared side by
// side.  `out` may be pinned host memory (the result is 48 bytes: written where the host reads it, no copy behind the kernel).
__device__ __forceinline__ bool sc_near_less(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }
__device__ __forceinline__ void sc_near_insert(float (&bd)[3], int (&bi)[3], float d, int i)
{
    if (sc_near_less(d, i, bd[2], bi[2])) {
        bd[2] = d; bi[2] = i;
        if (sc_near_less(bd[2], bi[2], bd[1], bi[1])) { const float a = bd[1]; bd[1] = bd[2]; bd[2] = a; const int b2 = bi[1]; bi[1] = bi[2]; bi[2] = b2; }
        if (sc_near_less(bd[1], bi[1], bd[0], bi[0])) { const float a = bd[0]; bd[0] = bd[1]; bd[1] = a; const int b2 = bi[0]; bi[0] = bi[1]; bi[1] = b2; }
    }
}

__global__ __launch_bounds__(kScThreads) void k_sc_detect(const double* __restrict__ store_desc, const float* __restrict__ store_ring,
                                                          const double* __restrict__ store_sector, int n_total, int n_search,
                                                          ScDetectOut* __restrict__ out)
{
    constexpr int NR = S2M_SC_NUM_RING;
    static_assert(NR % 4 == 0, "ring keys are read four floats at a time");
    __shared__ ScShared sh[3];
    __shared__ float s_d2[kScThreads / 64][3];
    __shared__ int   s_ix[kScThreads / 64][3];
    __shared__ int   s_cand[3];
    const int t = threadIdx.x, q = n_total - 1;
    // exact 3-NN over the fp32 ring keys, accumulation order of nanoflann's L2_Adaptor (groups of four);
    // ties go to the lower index
    float bd[3] = { INFINITY, INFINITY, INFINITY };
    int bi[3] = { 0x7fffffff, 0x7fffffff, 0x7fffffff };
    float4 qk[NR / 4];
#pragma unroll
    for (int g = 0; g < NR / 4; g++) qk[g] = reinterpret_cast<const float4*>(store_ring + (size_t)q * NR)[g];
    for (int i = t; i < n_search; i += kScThreads) {
        const float4* b = reinterpret_cast<const float4*>(store_ring + (size_t)i * NR);      // (rows are 80 bytes: 16-byte aligned)
        float4 bk[NR / 4];
#pragma unroll
        for (int g = 0; g < NR / 4; g++) bk[g] = b[g];
        const float result = sc_ring_d2(qk, bk);
        if (result < bd[2]) {                             // i ascends per thread: an equal distance stays behind
            bd[2] = result; bi[2] = i;
            if (bd[2] < bd[1]) { const float a = bd[1]; bd[1] = bd[2]; bd[2] = a; const int b2 = bi[1]; bi[1] = bi[2]; bi[2] = b2; }
            if (bd[1] < bd[0]) { const float a = bd[0]; bd[0] = bd[1]; bd[1] = a; const int b2 = bi[0]; bi[0] = bi[1]; bi[1] = b2; }
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {              // both partners end with the same three
        float pd[3]; int pi[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { pd[k] = __shfl_xor(bd[k], off, 64); pi[k] = __shfl_xor(bi[k], off, 64); }
#pragma unroll
        for (int k = 0; k < 3; k++) sc_near_insert(bd, bi, pd[k], pi[k]);
    }
    if ((t & 63) == 0)
        for (int k = 0; k < 3; k++) { s_d2[t >> 6][k] = bd[k]; s_ix[t >> 6][k] = bi[k]; }
    __syncthreads();
    if (t == 0) {
        float fd[3] = { INFINITY, INFINITY, INFINITY };
        int fi[3] = { 0x7fffffff, 0x7fffffff, 0x7fffffff };
        for (int u = 0; u < kScThreads / 64; u++)
            for (int k = 0; k < 3; k++) sc_near_insert(fd, fi, s_d2[u][k], s_ix[u][k]);
        for (int k = 0; k < 3; k++) {
            const bool have = fi[k] != 0x7fffffff;        // fewer keys than candidates: index 0 (:289 zero-initialised)
            s_cand[k] = have ? fi[k] : 0;
            out->cand_idx[k] = s_cand[k];
            out->cand_d2[k] = have ? fd[k] : 0.0f;
        }
    }
    __syncthreads();
    sc_distance_block<3>(store_desc, store_sector, store_desc + (size_t)q * (NR * S2M_SC_NUM_SECTOR), store_sector + (size_t)q * S2M_SC_NUM_SECTOR,
                         s_cand, sh);
    if (t == 0) {
        double min_dist = 10000000;
        int nn_align = 0, nn_idx = 0;
        for (int c = 0; c < 3; c++)                        // :302-316
            if (sh[c].dist_out < min_dist) { min_dist = sh[c].dist_out; nn_align = sh[c].shift_out; nn_idx = s_cand[c]; }
        out->min_dist = min_dist; out->nn_idx = nn_idx; out->nn_align = nn_align;
        out->loop_id = (min_dist < 0.3) ? nn_idx : -1;    // SC_DIST_THRES (Scancontext.h:95)
        out->yaw_diff_rad = (float)((double)(float)((double)nn_align * (360.0 / 60.0)) * M_PI / 180.0);   // deg2rad(float) (:17-20, :338)
    }
}

}  // namespace s2m

void s2m::host::sc_launch_detect(hipStream_t stream, const double* store_desc, const float* store_ring, const double* store_sector,
                                 int n_total, int n_search, ScDetectOut* out)
{
    hipLaunchKernelGGL(k_sc_detect, dim3(1), dim3(kScThreads), 0, stream, store_desc, store_ring, store_sector, n_total, n_search, out);
}

void s2m::host::sc_launch_distance_batch(hipStream_t stream, const double* store_desc, const double* store_sector, int query,
                                         const int32_t* cand, int m, double* dist, int32_t* shift)
{
    hipLaunchKernelGGL(k_sc_distance_batch, dim3((unsigned)m), dim3(kScThreads), 0, stream, store_desc, store_sector, query, cand, dist, shift);
}

namespace {

// ---- ScanContext store ---------------------------------------------------------------------------
constexpr size_t kScDesc = (size_t)S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR;

}  // namespace

// grow-with-copy (ensure() alone would drop the contents)
int s2m::host::sc_reserve(s2m_context* h, size_t want)
{
    if (want <= h->sc.cap) return S2M_OK;
    size_t cap = h->sc.cap ? h->sc.cap : 256;
    while (cap < want) cap *= 2;
    struct Part { DevBuf* b; size_t elem; } parts[3] = { { &h->sc.store_desc, sizeof(double) * kScDesc },
                                                         { &h->sc.store_ring, sizeof(float) * S2M_SC_NUM_RING },
                                                         { &h->sc.store_sector, sizeof(double) * S2M_SC_NUM_SECTOR } };
    for (Part& p : parts) {
        void* np = nullptr;
        S2M_HIP(h, hipMalloc(&np, p.elem * cap));
        if (h->sc.n) S2M_HIP(h, hipMemcpyAsync(np, p.b->p, p.elem * h->sc.n, hipMemcpyDeviceToDevice, h->stream));
        S2M_HIP(h, hipStreamSynchronize(h->stream));
        S2M_HIP(h, p.b->reset(np, p.elem * cap));
    }
    h->sc.cap = cap;
    return S2M_OK;
}

// descriptor + ring key are in h->sc.out (device): append them as key frame sc.n
int s2m::host::sc_append_from_out(s2m_context* h)
{
    int rc = sc_reserve(h, h->sc.n + 1);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sc_append, dim3(1), dim3(kScThreads), 0, h->stream, (const double*)h->sc.out.as<double>(),
                       h->sc.store_desc.as<double>(), h->sc.store_ring.as<float>(), h->sc.store_sector.as<double>(), (int)h->sc.n);
    S2M_HIP(h, hipGetLastError());
    h->sc.n++;
    return S2M_OK;
}

// SCManager::makeScancontext + ring key of a host cloud into h->sc.out (device)
int s2m::host::sc_build_descriptor(s2m_context* h, const void* pts, size_t n, size_t stride_bytes, bool on_device)
{
    S2M_HIP(h, hipMemsetAsync(h->sc.bins.p, 0, sizeof(uint32_t) * kScDesc, h->stream));
    if (n > 0) {
        const unsigned char* d_pts = static_cast<const unsigned char*>(pts);
        if (!on_device) {
            int rc = stage_host_records(h, h->reg.raw_scan, pts, n * stride_bytes);
            if (rc) return rc;
            d_pts = h->reg.raw_scan.as<unsigned char>();
        }
        const int blocks = std::min((int)((n + 255) / 256), 1024);
        hipLaunchKernelGGL(k_sc_polar_max, dim3(blocks), dim3(256), 0, h->stream, d_pts, stride_bytes, (int)n, h->sc.bins.as<uint32_t>());
    }
    hipLaunchKernelGGL(k_sc_finish, dim3(1), dim3(64), 0, h->stream, (const uint32_t*)h->sc.bins.as<uint32_t>(),
                       h->sc.out.as<double>(), h->sc.out.as<double>() + kScDesc);
    S2M_HIP(h, hipGetLastError());
    return S2M_OK;
}
