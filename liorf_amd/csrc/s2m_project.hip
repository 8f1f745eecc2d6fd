// s2m_project.hip — imageProjection's point filter and IMU deskew (reference src/imageProjection.cpp:493-598) as three HIP
// kernels for gfx950 (wave64). Compiled with -ffp-contract=off like the rest of the library: every fp32 / fp64 expression
// that restates the reference is evaluated as written, one rounding per operation.
//
//   k_proj_flag      one lane per raw record: x, y, z (one 16-byte load where the layout allows it) and the ring through
//                    the layout, the four tests of projectPointCloud() (:581-592), one ballot per (wave, round) kept as the
//                    survivor mask; per workgroup the survivor count and the lowest surviving index.
//   k_proj_prefix    one workgroup: exclusive prefix of the counts, the total (to pinned host memory), the first survivor
//                    (minimum of the workgroups' lowest indices: no atomics, no order) and, with deskew on, from that record
//                    S = transStartInverse (:551) - 48 bytes every workgroup of the next kernel reads by scalar loads.
//   k_proj_scatter   a survivor's place = survivors of the workgroups before + of the waves before + of the rounds before + of
//                    the lanes before (the stored ballots): index order whatever the launch order, as k_kf_radius_write. Per
//                    survivor findRotation() by bisection over the IMU table in global memory (<= 2 000 x 4 doubles, hot in
//                    L1/L2: a real scan has about 50 entries), getTransformation, B = S * R, the point.
//
// k_proj_prefix and k_proj_scatter are templates over MOTION: <false> is findPosition() as the reference ships it (zeros,
// :520-534) and is what s2m_project_scan launches; <true> is findPosition() with its commented lines live (:526-533) -
// the position ratio * odomIncre enters both getTransformation calls (:551, :556) - and is launched by
// s2m_project_scan_motion when motion->enabled. time_scan_end and the increments are kernel arguments (scalar loads).
//
// The stage moves stride * n + 32 * n_out bytes and does a few hundred flops per survivor: it is launch- and PCIe-bound.
#include "s2m_project.hpp"

#include <climits>
#include <cstring>

#include "s2m_glibc_trig.hpp"       // glibc_sincosf_both: tests/test_project_gpu.py compares every deskewed coordinate with a libm build

namespace s2m {

namespace {

// ---- reading one raw record through the layout ---------------------------------------------------------------------
__device__ __forceinline__ void proj_load_xyz(const unsigned char* rec, uint32_t off_x, int vec, float& x, float& y, float& z)
{
    if (vec) {
        const float4 v = *reinterpret_cast<const float4*>(rec + off_x);
        x = v.x; y = v.y; z = v.z;
    } else {
        const float* p = reinterpret_cast<const float*>(rec + off_x);
        x = p[0]; y = p[1]; z = p[2];
    }
}

__device__ __forceinline__ int proj_load_ring(const unsigned char* rec, uint32_t off, int type)
{
    if (type == S2M_RING_U8) return (int)rec[off];
    if (type == S2M_RING_U16) return (int)*reinterpret_cast<const uint16_t*>(rec + off);
    return *reinterpret_cast<const int32_t*>(rec + off);
}

// the record's time as the reference's conversion loops leave it in laserCloudIn->points[i].time (:216-274)
__device__ __forceinline__ float proj_load_time(const unsigned char* rec, const unsigned char* rec0, uint32_t off, int type)
{
    if (type == S2M_TIME_F32) return *reinterpret_cast<const float*>(rec + off);
    if (type == S2M_TIME_U32_NS) return (float)*reinterpret_cast<const uint32_t*>(rec + off) * 1e-9f;      // src.t * 1e-9f (:235)
    if (type == S2M_TIME_U32) return (float)*reinterpret_cast<const uint32_t*>(rec + off);                 // static_cast<float>(src.t) (:253)
    return (float)(*reinterpret_cast<const double*>(rec + off) - *reinterpret_cast<const double*>(rec0 + off));   // :263, :272
}

// findRotation() (:493-518). The linear walk stops at the first front in [0, cur) with pointTime < imuTime[front]; the
// table times are non-decreasing (checked at the boundary), so the bisection with the same predicate finds the same index.
__device__ __forceinline__ void proj_find_rotation(const double* __restrict__ tab, int cur, double pointTime, float& rx, float& ry, float& rz)
{
    const double* t = tab;
    const double* X = tab + S2M_IMU_QUEUE_LENGTH;
    const double* Y = tab + 2 * S2M_IMU_QUEUE_LENGTH;
    const double* Z = tab + 3 * S2M_IMU_QUEUE_LENGTH;
    int lo = 0, hi = cur;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pointTime < t[mid]) hi = mid; else lo = mid + 1;
    }
    const int front = lo;
    const double tf = t[front];
    if (pointTime > tf || front == 0) {                                   // :505-509
        rx = (float)X[front]; ry = (float)Y[front]; rz = (float)Z[front];
    } else {                                                              // :511-516
        const int back = front - 1;
        const double tb = t[back];
        const double ratioFront = (pointTime - tb) / (tf - tb);
        const double ratioBack = (tf - pointTime) / (tf - tb);
        rx = (float)(X[front] * ratioFront + X[back] * ratioBack);
        ry = (float)(Y[front] * ratioFront + Y[back] * ratioBack);
        rz = (float)(Z[front] * ratioFront + Z[back] * ratioBack);
    }
}

// pcl::getTransformation(0, 0, 0, roll, pitch, yaw): the linear part in host_pose_to_transform's term order (A = cos yaw,
// B = sin yaw, C = cos pitch, D = sin pitch, E = cos roll, F = sin roll), row-major 3x3; the translation is (0, 0, 0).
__device__ __forceinline__ void proj_rotation(float roll, float pitch, float yaw, float R[9])
{
    float A, B, C, D, E, F;
    glibc_sincosf_both(yaw, B, A);
    glibc_sincosf_both(pitch, D, C);
    glibc_sincosf_both(roll, F, E);
    const float DE = D * E, DF = D * F;
    R[0] = A * C; R[1] = A * DF - B * E; R[2] = B * F + A * DE;
    R[3] = B * C; R[4] = A * E + B * DF; R[5] = B * DE - A * F;
    R[6] = -D;    R[7] = C * F;          R[8] = C * E;
}

// findPosition() with its commented lines live (:529-533): ratio = relTime / (timeScanEnd - timeScanCur), the division in
// double (relTime is the record's float time widened, :594 -> :536), narrowed once to float; the three products in float.
// timeScanEnd == timeScanCur gives an infinite or NaN ratio, as the reference's arithmetic would.
struct ProjMotion { double time_scan_end; float incre_x, incre_y, incre_z; };
struct ProjNoMotion {};
template <bool MOTION> struct ProjMotionArg { using type = ProjNoMotion; };
template <> struct ProjMotionArg<true> { using type = ProjMotion; };
__device__ __forceinline__ void proj_find_position(const ProjMotion& mo, double time_scan_cur, float relTime, float t[3])
{
    const float ratio = (float)((double)relTime / (mo.time_scan_end - time_scan_cur));
    t[0] = ratio * mo.incre_x; t[1] = ratio * mo.incre_y; t[2] = ratio * mo.incre_z;
}

// Eigen 3.3 Transform<float,3,Affine>::inverse() [ext]: S row-major 3x4 from the linear part m and the translation t
// ((0, 0, 0) without MOTION)
__device__ __forceinline__ float proj_cof(const float m[9], int i, int j)
{
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1];
}
template <bool MOTION>
__device__ inline void proj_affine_inverse(const float m[9], const float t[3], float S[12])
{
    const float c0 = proj_cof(m, 0, 0), c1 = proj_cof(m, 1, 0), c2 = proj_cof(m, 2, 0);
    const float det = (c0 * m[0] + c1 * m[3]) + c2 * m[6];
    const float invdet = 1.0f / det;
    float L[9];
    L[0] = c0 * invdet; L[1] = c1 * invdet; L[2] = c2 * invdet;
    for (int c = 0; c < 3; c++) { L[3 + c] = proj_cof(m, c, 1) * invdet; L[6 + c] = proj_cof(m, c, 2) * invdet; }
    const float t0 = MOTION ? t[0] : 0.0f, t1 = MOTION ? t[1] : 0.0f, t2 = MOTION ? t[2] : 0.0f;
    for (int r = 0; r < 3; r++) {
        S[r * 4 + 0] = L[r * 3 + 0]; S[r * 4 + 1] = L[r * 3 + 1]; S[r * 4 + 2] = L[r * 3 + 2];
        S[r * 4 + 3] = -((L[r * 3 + 0] * t0 + L[r * 3 + 1] * t1) + L[r * 3 + 2] * t2);
    }
}

// ---- kernel 1: the four tests, the survivor masks, per-workgroup count and lowest surviving index -----------------------
__global__ __launch_bounds__(256) void k_proj_flag(const unsigned char* __restrict__ in, int n, s2m_scan_layout lay, s2m_project_params prm,
                                                   int vec, unsigned long long* __restrict__ mask, int32_t* __restrict__ part)
{
    __shared__ int32_t s_cnt[4], s_first[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int base = blockIdx.x * kProjTile + wave * (kProjTile / 4);
    int32_t cnt = 0, first = INT_MAX;
#pragma unroll
    for (int r = 0; r < kProjRounds; r++) {
        const int i = base + r * 64 + lane;
        bool keep = false;
        if (i < n) {
            const unsigned char* rec = in + (size_t)i * lay.stride;
            float x, y, z;
            proj_load_xyz(rec, lay.off_x, vec, x, y, z);
            const float range = sqrtf((x * x + y * y) + z * z);                           // pointDistance (lib/common_lib.cpp:28-31)
            const int ring = proj_load_ring(rec, lay.off_ring, lay.ring_type);
            keep = !(range < prm.lidar_min_range || range > prm.lidar_max_range)          // :581
                   && !(ring < 0 || ring >= prm.n_scan)                                   // :585
                   && (ring % prm.downsample_rate == 0)                                   // :588
                   && (i % prm.point_filter_num == 0);                                    // :591
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) mask[(size_t)blockIdx.x * 16 + wave * 4 + r] = m;
        if (m != 0ull && first == INT_MAX) first = base + r * 64 + (int)__ffsll((long long)m) - 1;
        cnt += __popcll(m);
    }
    if (lane == 0) { s_cnt[wave] = cnt; s_first[wave] = first; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        part[2 * blockIdx.x + 1] = min(min(s_first[0], s_first[1]), min(s_first[2], s_first[3]));
    }
}

// ---- kernel 2: exclusive prefix over the workgroups, the count, the first survivor and S -----------------------------------
template <bool MOTION>
__global__ __launch_bounds__(1024) void k_proj_prefix(int32_t* __restrict__ part, int nblk, const unsigned char* __restrict__ in, s2m_scan_layout lay,
                                                      int deskew, int cur, double time_scan_cur, const double* __restrict__ tab,
                                                      float* __restrict__ start, ProjCount* __restrict__ h_count,
                                                      typename ProjMotionArg<MOTION>::type mo)
{
    __shared__ int32_t s_w[16], s_f[16];
    __shared__ int32_t s_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_base = 0;
    int32_t first = INT_MAX;
    __syncthreads();
    for (int j0 = 0; j0 < nblk; j0 += 1024) {
        const int j = j0 + (int)threadIdx.x;
        const int32_t v = j < nblk ? part[2 * j] : 0;
        if (j < nblk) first = min(first, part[2 * j + 1]);
        int32_t inc = v;                                                  // inclusive scan inside the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t o = __shfl_up(inc, off, 64);
            if (lane >= off) inc += o;
        }
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        int32_t before = s_base;
        for (int w = 0; w < wave; w++) before += s_w[w];
        if (j < nblk) part[2 * j] = before + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) s_base = before + inc;
        __syncthreads();
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) first = min(first, __shfl_xor(first, off, 64));
    if (lane == 0) s_f[wave] = first;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; w++) first = min(first, s_f[w]);
        const int32_t total = s_base;
        part[2 * nblk] = total;
        h_count->n_out = total;
        h_count->first = total > 0 ? first : -1;
        if (deskew && total > 0) {                                        // transStartInverse from the first survivor (:549-553)
            const unsigned char* rec = in + (size_t)first * lay.stride;
            const float relTime = proj_load_time(rec, in, lay.off_time, lay.time_type);
            const double pointTime = time_scan_cur + (double)relTime;                                                  // :541
            float rx, ry, rz, R[9], S[12], t[3] = { 0.0f, 0.0f, 0.0f };
            proj_find_rotation(tab, cur, pointTime, rx, ry, rz);
            if constexpr (MOTION) proj_find_position(mo, time_scan_cur, relTime, t);                                   // :547
            proj_rotation(rx, ry, rz, R);
            proj_affine_inverse<MOTION>(R, t, S);
            for (int k = 0; k < 12; k++) start[k] = S[k];
        }
    }
}

// ---- kernel 3: survivors to their places, deskewed ----------------------------------------------------------------------
template <bool MOTION>
__global__ __launch_bounds__(256) void k_proj_scatter(const unsigned char* __restrict__ in, s2m_scan_layout lay, int vec, int deskew, int cur,
                                                      double time_scan_cur, const double* __restrict__ tab, const float* __restrict__ start,
                                                      const unsigned long long* __restrict__ mask, const int32_t* __restrict__ part,
                                                      unsigned char* __restrict__ out, typename ProjMotionArg<MOTION>::type mo)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int base = blockIdx.x * kProjTile + wave * (kProjTile / 4);
    const unsigned long long* bm = mask + (size_t)blockIdx.x * 16;
    int32_t off = part[2 * blockIdx.x];                                   // survivors of the workgroups before
    for (int k = 0; k < wave * 4; k++) off += __popcll(bm[k]);            // ... of the waves before (wave-uniform loads)
    float S[12];
    if (deskew) {
#pragma unroll
        for (int k = 0; k < 12; k++) S[k] = start[k];
    }
    for (int r = 0; r < kProjRounds; r++) {
        const unsigned long long m = bm[wave * 4 + r];
        if ((m >> lane) & 1ull) {
            const int i = base + r * 64 + lane;
            const int32_t at = off + __popcll(m & ((1ull << lane) - 1ull));
            const unsigned char* rec = in + (size_t)i * lay.stride;
            float x, y, z;
            proj_load_xyz(rec, lay.off_x, vec, x, y, z);
            const float inten = *reinterpret_cast<const float*>(rec + lay.off_intensity);
            float ox = x, oy = y, oz = z;                                 // deskewFlag == -1 || !imuAvailable: return *point (:538-539)
            if (deskew) {
                const float relTime = proj_load_time(rec, in, lay.off_time, lay.time_type);
                const double pointTime = time_scan_cur + (double)relTime;                                               // :541
                float rx, ry, rz, R[9];
                proj_find_rotation(tab, cur, pointTime, rx, ry, rz);      // :544
                proj_rotation(rx, ry, rz, R);                             // transFinal (:556); without MOTION findPosition() returns zeros (:520-534)
                // transBt = transStartInverse * transFinal (:557) as a 4x4 product [ext]; row 3 of both is (0, 0, 0, 1), column 3 of
                // transFinal is (0, 0, 0, 1) without MOTION and (posX, posY, posZ, 1) with it
                float Bm[12];
                if constexpr (MOTION) {
                    float t[3];
                    proj_find_position(mo, time_scan_cur, relTime, t);    // :547
#pragma unroll
                    for (int a = 0; a < 3; a++) {
#pragma unroll
                        for (int b = 0; b < 3; b++)
                            Bm[a * 4 + b] = ((S[a * 4 + 0] * R[0 * 3 + b] + S[a * 4 + 1] * R[1 * 3 + b]) + S[a * 4 + 2] * R[2 * 3 + b]) + S[a * 4 + 3] * 0.0f;
                        Bm[a * 4 + 3] = ((S[a * 4 + 0] * t[0] + S[a * 4 + 1] * t[1]) + S[a * 4 + 2] * t[2]) + S[a * 4 + 3] * 1.0f;
                    }
                } else {
#pragma unroll
                    for (int a = 0; a < 3; a++) {
#pragma unroll
                        for (int b = 0; b < 3; b++)
                            Bm[a * 4 + b] = ((S[a * 4 + 0] * R[0 * 3 + b] + S[a * 4 + 1] * R[1 * 3 + b]) + S[a * 4 + 2] * R[2 * 3 + b]) + S[a * 4 + 3] * 0.0f;
                        Bm[a * 4 + 3] = ((S[a * 4 + 0] * 0.0f + S[a * 4 + 1] * 0.0f) + S[a * 4 + 2] * 0.0f) + S[a * 4 + 3] * 1.0f;
                    }
                }
                ox = ((Bm[0] * x + Bm[1] * y) + Bm[2] * z) + Bm[3];       // :560-562
                oy = ((Bm[4] * x + Bm[5] * y) + Bm[6] * z) + Bm[7];
                oz = ((Bm[8] * x + Bm[9] * y) + Bm[10] * z) + Bm[11];
            }
            float4* o = reinterpret_cast<float4*>(out + (size_t)at * kProjOutStride);
            o[0] = make_float4(ox, oy, oz, 0.0f);
            o[1] = make_float4(inten, 0.0f, 0.0f, 0.0f);
        }
        off += __popcll(m);
    }
}

}  // namespace

hipError_t proj_launch(hipStream_t stream, const ProjArgs& a)
{
    const int nblk = proj_blocks(a.n);
    const s2m_scan_layout& l = a.lay;
    const int vec = (l.stride % 16 == 0 && l.off_x % 16 == 0 && (uint64_t)l.off_x + 16 <= l.stride &&
                     (reinterpret_cast<uintptr_t>(a.d_in) & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(k_proj_flag, dim3(nblk), dim3(256), 0, stream, a.d_in, (int)a.n, a.lay, a.prm, vec, a.d_mask, a.d_part);
    if (a.motion && a.deskew) {                                           // deskew == 0 copies whatever motion says (:538-539)
        const ProjMotion mo{ a.time_scan_end, a.odom_incre[0], a.odom_incre[1], a.odom_incre[2] };
        hipLaunchKernelGGL(k_proj_prefix<true>, dim3(1), dim3(1024), 0, stream, a.d_part, nblk, a.d_in, a.lay, a.deskew, a.imu_pointer_cur,
                           a.time_scan_cur, a.d_table, a.d_start, a.h_count, mo);
        hipLaunchKernelGGL(k_proj_scatter<true>, dim3(nblk), dim3(256), 0, stream, a.d_in, a.lay, vec, a.deskew, a.imu_pointer_cur, a.time_scan_cur,
                           a.d_table, (const float*)a.d_start, (const unsigned long long*)a.d_mask, (const int32_t*)a.d_part, a.d_out, mo);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_proj_prefix<false>, dim3(1), dim3(1024), 0, stream, a.d_part, nblk, a.d_in, a.lay, a.deskew, a.imu_pointer_cur,
                       a.time_scan_cur, a.d_table, a.d_start, a.h_count, ProjNoMotion{});
    hipLaunchKernelGGL(k_proj_scatter<false>, dim3(nblk), dim3(256), 0, stream, a.d_in, a.lay, vec, a.deskew, a.imu_pointer_cur, a.time_scan_cur,
                       a.d_table, (const float*)a.d_start, (const unsigned long long*)a.d_mask, (const int32_t*)a.d_part, a.d_out, ProjNoMotion{});
    return hipGetLastError();
}

}  // namespace s2m
