// s2m_loop_detect.hip — kernels of the loop detection by position for many keys (s2m_loop_detect.hpp):
// detectLoopClosureDistance() (reference src/mapOptmization.cpp:732-765) for any stored key, any searched set, top_k candidates
// and many queries at once.  k_loop_detect_many holds a tile of stored positions and times in LDS while a block of queries, one
// per lane, passes it, and keeps every query's nearest in registers; k_loop_detect_rows merges a query's lists over the store
// splits and writes its row.  The distance is kf_d2 (s2m_kf_d2.hpp), the statement k_loop_detect uses.  Compiled with
// -ffp-contract=off; no fused multiply-add.  A candidate's word, (bits of d2) << 32 | key, is distinct per key, so the words of a
// query are totally ordered, and membership - the searched set, the radius and the time gate - is a predicate on the pair: the
// top_k smallest words of a set do not depend on how the set was cut, so a row is bit for bit the same for any tile size, split
// count, query block or pass.  No kernel uses atomics, none adds floating-point numbers across lanes, none waits for another.
#include <math.h>

#include "s2m_kf_d2.hpp"
#include "s2m_loop_detect.hpp"

namespace s2m {

namespace {

constexpr int T = kLdTile, B = kLdBlock;
constexpr int kLdThreads = B;                         // one wave a workgroup, so every barrier is the wave's own
constexpr int kRowThreads = 256;                      // k_loop_detect_rows: a query per thread
constexpr unsigned long long kLdNone = ~0ull;         // an empty place of a list: above every word (bits of d2 < 0x7f800000)
static_assert(kLdThreads == 64 && T % kLdThreads == 0, "one wave, whole wave steps over a tile");

// list[0, KC): ascending words, kLdNone behind the ones held; w < list[KC - 1] takes the last place and sinks to its own
template <int KC>
__device__ __forceinline__ void ld_insert(unsigned long long (&list)[KC], unsigned long long w)
{
    list[KC - 1] = w;
#pragma unroll
    for (int j = KC - 1; j > 0; j--) {
        const unsigned long long lo = list[j - 1] < list[j] ? list[j - 1] : list[j];
        const unsigned long long hi = list[j - 1] < list[j] ? list[j] : list[j - 1];
        list[j - 1] = lo; list[j] = hi;
    }
}

// Workgroup (x, y): queries [x * B, x * B + B) of the pass, one per lane, against the tiles of split y.  Every lane reads the
// same item of the tile per step (an LDS broadcast).  d2 >= +0, so the word orders exactly as (d2, key); a NaN on either side of
// a comparison fails it, so a NaN position or time is never a candidate.  part: words [split][j][query].
template <int KC>
__global__ __launch_bounds__(kLdThreads) void k_loop_detect_many(const float4* __restrict__ pos, const double* __restrict__ time,
                                                                 const int32_t* __restrict__ keys, const double* __restrict__ time_cur,
                                                                 int m, ScManySet set, float r2, double time_diff, int tiles_per_split,
                                                                 unsigned long long* __restrict__ part)
{
    __shared__ float4 s_pos[T];
    __shared__ double s_time[T];
    const int lane = threadIdx.x;
    const int q = blockIdx.x * B + lane;
    const bool live = q < m;
    const int qkey = keys[live ? q : m - 1];              // (an idle lane walks along with the pass's last query and writes nothing)
    const float4 qp = pos[qkey];
    const double qt = time_cur ? time_cur[live ? q : m - 1] : time[qkey];
    unsigned long long list[KC];
#pragma unroll
    for (int j = 0; j < KC; j++) list[j] = kLdNone;
    const int n_tiles = (set.end - set.first + T - 1) / T;
    const int tile0 = blockIdx.y * tiles_per_split, tile1 = min(n_tiles, tile0 + tiles_per_split);
    for (int tile = tile0; tile < tile1; tile++) {
        const int c0 = set.first + tile * T, nc = min(T, set.end - c0);
        __syncthreads();                                  // the previous tile is read until here
        for (int i = lane; i < nc; i += kLdThreads) { s_pos[i] = pos[c0 + i]; s_time[i] = time[c0 + i]; }
        __syncthreads();
        for (int k = 0; k < nc; k++) {
            const float d2 = kf_d2(s_pos[k], qp);
            // radiusSearch: d2 < (float)(R*R); then abs(time - timeLaserInfoCur) > historyKeyframeSearchTimeDiff (:755)
            if (d2 < r2 && fabs(s_time[k] - qt) > time_diff && sc_many_in_set(set, qkey, c0 + k)) {
                const unsigned long long w = ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)(c0 + k);
                if (w < list[KC - 1]) ld_insert<KC>(list, w);
            }
        }
    }
    if (live) {
#pragma unroll
        for (int j = 0; j < KC; j++) part[((size_t)blockIdx.y * KC + j) * (size_t)m + q] = list[j];
    }
}

// A thread per query: the top_k smallest of its splits' lists, then the row - keys, distances, count; the places behind the count
// are filled (-1, +inf) on the device, the host copies the count's worth.
template <int KC>
__global__ __launch_bounds__(kRowThreads) void k_loop_detect_rows(const unsigned long long* __restrict__ part, int m, int splits, int top_k,
                                                                  int32_t* __restrict__ out_key, float* __restrict__ out_d2,
                                                                  int32_t* __restrict__ out_n)
{
    const int q = blockIdx.x * kRowThreads + threadIdx.x;
    if (q >= m) return;
    unsigned long long list[KC];
#pragma unroll
    for (int j = 0; j < KC; j++) list[j] = kLdNone;
    for (int s = 0; s < splits; s++) {
#pragma unroll
        for (int j = 0; j < KC; j++) {
            const unsigned long long w = part[((size_t)s * KC + j) * (size_t)m + q];
            if (w < list[KC - 1]) ld_insert<KC>(list, w);
        }
    }
    int n = 0;
#pragma unroll
    for (int j = 0; j < KC; j++) {
        if (j >= top_k) continue;
        const bool have = list[j] != kLdNone;
        out_key[(size_t)q * top_k + j] = have ? (int32_t)(uint32_t)list[j] : -1;
        out_d2[(size_t)q * top_k + j] = have ? __uint_as_float((uint32_t)(list[j] >> 32)) : INFINITY;
        n += have ? 1 : 0;
    }
    out_n[q] = n;
}

template <int KC>
void ld_launch_kc(hipStream_t stream, const LdArgs& a)
{
    const int n_tiles = ld_tiles(a.set.end - a.set.first);
    const int tiles_per_split = (n_tiles + a.splits - 1) / a.splits;
    const dim3 grid((unsigned)((a.m + B - 1) / B), (unsigned)a.splits);
    hipLaunchKernelGGL(k_loop_detect_many<KC>, grid, dim3(kLdThreads), 0, stream, a.pos, a.time, a.keys, a.time_cur, a.m, a.set, a.r2,
                       a.time_diff, tiles_per_split, a.part);
    hipLaunchKernelGGL(k_loop_detect_rows<KC>, dim3((unsigned)((a.m + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads), 0, stream,
                       (const unsigned long long*)a.part, a.m, a.splits, a.top_k, a.out_key, a.out_d2, a.out_n);
}

}  // namespace

hipError_t ld_launch(hipStream_t stream, const LdArgs& a)
{
    if (a.m <= 0 || a.set.first >= a.set.end || a.top_k < 1 || a.top_k > S2M_LOOP_MAX_CANDIDATES || a.splits < 1 || a.splits > kLdMaxSplits)
        return hipErrorInvalidValue;
    switch (ld_list_words(a.top_k)) {
    case 1: ld_launch_kc<1>(stream, a); break;
    case 2: ld_launch_kc<2>(stream, a); break;
    case 4: ld_launch_kc<4>(stream, a); break;
    default: ld_launch_kc<8>(stream, a); break;
    }
    return hipGetLastError();
}

}  // namespace s2m
