// s2m_session.hip — kernels of the session save, load and append (s2m_session.hpp): k_session_gather, k_session_scatter,
// k_sc_keys_batch, and k_session_place, which moves an appended session's keys by a rigid anchor (one lane per key, the pose
// graph's read-out statements of s2m_pose_readout.hpp).  The first two are plain memory-bound copies: every lane moves 16 bytes, consecutive lanes consecutive addresses; the segment
// of a unit is found by bisection over the offset table, once per workgroup for the tile's two ends and per lane only between
// those two (no step for a tile inside one key frame); the two 64-bit sums are reduced by shuffles and one LDS round, one store
// per workgroup, no atomics.  No scratch.
#include <hip/hip_runtime.h>

#include "s2m_pose_readout.hpp"
#include "s2m_sc_keys.hpp"
#include "s2m_session.hpp"

using namespace s2m;

namespace s2m {

// the largest k in [lo, hi] with off[k] <= r (off[lo] <= r): the segment that holds unit r, empty segments skipped
__device__ __forceinline__ int sess_seg_of(const uint64_t* __restrict__ off, int lo, int hi, uint64_t r)
{
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <bool kScatter>
__device__ __forceinline__ void session_move(unsigned char* const* __restrict__ seg_ptr, const uint64_t* __restrict__ seg_off, int n_seg,
                                             uint64_t r0, uint64_t r1, uint4* __restrict__ stage, SessSum* __restrict__ partial)
{
    __shared__ unsigned long long s_sum[kSessThreads / 64][2];
    const uint64_t t0 = r0 + (uint64_t)blockIdx.x * kSessTile;
    if (t0 >= r1) return;                                   // (the grid is the chunk's tiles: never taken)
    const uint64_t t1 = t0 + kSessTile < r1 ? t0 + kSessTile : r1;
    const int k_lo = sess_seg_of(seg_off, 0, n_seg - 1, t0);
    const int k_hi = sess_seg_of(seg_off, k_lo, n_seg - 1, t1 - 1);
    unsigned long long s1 = 0, s2 = 0;
    const uint32_t halves = (uint32_t)(t1 - t0) * 2;        // 16-byte halves of the tile's units
    for (uint32_t u = threadIdx.x; u < halves; u += kSessThreads) {
        const uint64_t rec = t0 + (u >> 1);
        const uint32_t half = u & 1u;
        const int k = sess_seg_of(seg_off, k_lo, k_hi, rec);
        uint4* at = reinterpret_cast<uint4*>(seg_ptr[k] + (rec - seg_off[k]) * kSessUnit) + half;
        uint4* st = stage + ((rec - r0) * 2 + half);
        uint4 v;
        if (kScatter) { v = *st; *at = v; } else { v = *at; *st = v; }
        const unsigned long long g = rec * 8 + half * 4 + 1;          // 1 + the section index of v.x
        s1 += ((unsigned long long)v.x + v.y) + ((unsigned long long)v.z + v.w);
        s2 += (g * v.x + (g + 1) * v.y) + ((g + 2) * v.z + (g + 3) * v.w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
    }
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6][0] = s1; s_sum[threadIdx.x >> 6][1] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        SessSum o{ 0, 0 };
        for (int w = 0; w < kSessThreads / 64; w++) { o.s1 += s_sum[w][0]; o.s2 += s_sum[w][1]; }
        partial[blockIdx.x] = o;
    }
}

__global__ __launch_bounds__(kSessThreads) void k_session_gather(const unsigned char* const* __restrict__ seg_ptr, const uint64_t* __restrict__ seg_off,
                                                                 int n_seg, uint64_t r0, uint64_t r1, uint4* __restrict__ stage,
                                                                 SessSum* __restrict__ partial)
{
    session_move<false>(const_cast<unsigned char* const*>(seg_ptr), seg_off, n_seg, r0, r1, stage, partial);
}

__global__ __launch_bounds__(kSessThreads) void k_session_scatter(unsigned char* const* __restrict__ seg_ptr, const uint64_t* __restrict__ seg_off,
                                                                  int n_seg, uint64_t r0, uint64_t r1, uint4* __restrict__ stage,
                                                                  SessSum* __restrict__ partial)
{
    session_move<true>(seg_ptr, seg_off, n_seg, r0, r1, stage, partial);
}

// makeAndSaveScancontextAndKeys' two keys (include/Scancontext.cpp:236-250) for descriptor blockIdx.x of the store: what
// k_sc_finish (or the host add) and k_sc_append leave, by the same two functions
__global__ __launch_bounds__(64) void k_sc_keys_batch(const double* __restrict__ store_desc, float* __restrict__ store_ring,
                                                      double* __restrict__ store_sector, int first)
{
    constexpr int NR = S2M_SC_NUM_RING, NS = S2M_SC_NUM_SECTOR;
    const size_t idx = (size_t)first + blockIdx.x;
    const double* d = store_desc + idx * NR * NS;
    const int t = threadIdx.x;
    if (t < NR) store_ring[idx * NR + t] = (float)sc_ring_key([&](int k) { return d[t * NS + k]; });
    if (t < NS) store_sector[idx * NS + t] = sc_sector_key([&](int r) { return d[r * NS + t]; });
}

// A o X (s2m_session.hpp)
__device__ __forceinline__ void sess_compose(const double* A, const double* X, double* O)
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) O[i * 3 + j] = (A[i * 3] * X[j] + A[i * 3 + 1] * X[3 + j]) + A[i * 3 + 2] * X[6 + j];
        O[9 + i] = ((A[i * 3] * X[9] + A[i * 3 + 1] * X[10]) + A[i * 3 + 2] * X[11]) + A[9 + i];
    }
}

// One lane per key of an appended session: the key's estimate moved by A (as fp64 bits; a key without one keeps what came in),
// and from its moved stored-pose state the store's float pose, position record and cached transform, by the pose graph's two
// statements (s2m_pose_readout.hpp).  Everything goes to a staging block; *bad is set if a result is not finite.
__global__ __launch_bounds__(kSessThreads) void k_session_place(SessMove A, const double* __restrict__ state, const double* __restrict__ est,
                                                                const int32_t* __restrict__ has, int count, double* __restrict__ est_out,
                                                                float4* __restrict__ pos, float* __restrict__ T, float* __restrict__ pose,
                                                                int32_t* __restrict__ bad)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    double P[12], X[12];
    bool ok = true;
    if (has[k]) {
        sess_compose(A.a, est + 12 * (size_t)k, X);
        for (int a = 0; a < 12; a++) ok = ok && isfinite(X[a]);
    } else {
        for (int a = 0; a < 12; a++) X[a] = est[12 * (size_t)k + a];
    }
    for (int a = 0; a < 12; a++) est_out[12 * (size_t)k + a] = X[a];
    sess_compose(A.a, state + 12 * (size_t)k, P);
    float o[6], Tk[12];
    pose_readout(P, o);
    for (int a = 0; a < 6; a++) ok = ok && isfinite(o[a]);
    pose_transform(o, Tk);
    for (int a = 0; a < 6; a++) pose[6 * (size_t)k + a] = o[a];
    for (int a = 0; a < 12; a++) T[12 * (size_t)k + a] = Tk[a];
    pos[k] = make_float4(o[0], o[1], o[2], 0.0f);
    if (!ok) *bad = 1;
}

}  // namespace s2m

void s2m::host::session_launch_place(hipStream_t stream, const SessMove& A, const unsigned char* in, int count, unsigned char* out)
{
    const SessPlaced l{ (size_t)count };
    hipLaunchKernelGGL(k_session_place, dim3((unsigned)((count + kSessThreads - 1) / kSessThreads)), dim3(kSessThreads), 0, stream, A,
                       reinterpret_cast<const double*>(in + l.in_state()), reinterpret_cast<const double*>(in + l.in_est()),
                       reinterpret_cast<const int32_t*>(in + l.in_has()), count, reinterpret_cast<double*>(out + l.out_est()),
                       reinterpret_cast<float4*>(out + l.out_pos()), reinterpret_cast<float*>(out + l.out_T()),
                       reinterpret_cast<float*>(out + l.out_pose()), reinterpret_cast<int32_t*>(out + l.out_bad()));
}

void s2m::host::session_launch_gather(hipStream_t stream, const unsigned char* const* seg_ptr, const uint64_t* seg_off, int n_seg, uint64_t r0,
                                      uint64_t r1, unsigned char* stage, SessSum* partial)
{
    hipLaunchKernelGGL(k_session_gather, dim3((unsigned)session_tiles(r1 - r0)), dim3(kSessThreads), 0, stream, seg_ptr, seg_off, n_seg, r0, r1,
                       reinterpret_cast<uint4*>(stage), partial);
}

void s2m::host::session_launch_scatter(hipStream_t stream, unsigned char* const* seg_ptr, const uint64_t* seg_off, int n_seg, uint64_t r0,
                                       uint64_t r1, const unsigned char* stage, SessSum* partial)
{
    hipLaunchKernelGGL(k_session_scatter, dim3((unsigned)session_tiles(r1 - r0)), dim3(kSessThreads), 0, stream, seg_ptr, seg_off, n_seg, r0, r1,
                       reinterpret_cast<uint4*>(const_cast<unsigned char*>(stage)), partial);
}

void s2m::host::session_launch_sc_keys(hipStream_t stream, const double* store_desc, float* store_ring, double* store_sector, int first, int n)
{
    hipLaunchKernelGGL(k_sc_keys_batch, dim3((unsigned)n), dim3(64), 0, stream, store_desc, store_ring, store_sector, first);
}
