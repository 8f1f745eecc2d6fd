// s2m_prep.hpp — the kernels in front of the LM loop: the map's uniform-grid index (bounding box, cell histogram, exclusive
// scan, scatter) and the scan's locality order with the split wish of every chunk.  Included by s2m_prep.hip alone, which
// launches them; the helpers shared with the loop's kernels (s2m_kernels.hpp) are s2m_device.hpp's.  The wave table itself is
// emitted by k_chunk_table, which stays in s2m_kernels.hpp beside k_chunk_table_density: the two share chunk_table_body and its
// LDS, and k_chunk_table compiles to other code in a module without its twin.
//
// Reference citations are file:line into jimmyshe/liorf (src/mapOptmization.cpp unless named).
#pragma once
#include "s2m_device.hpp"

namespace s2m {

// ------------------------------------------------------------------------------------------
// index build: bounding box, cell histogram with per-point rank, exclusive scan, scatter
// ------------------------------------------------------------------------------------------
// Bounding box of the finite coordinates, as ordered uints (min x, y, z, max x, y, z).  Every workgroup leaves its own box in
// `part` (8 words each), k_bbox_fold puts them together: adds from every workgroup on one address are served one after the other on
// this part (~6 ns each) - six of them from each of 782 workgroups were 15 of this kernel's 20 us at 200 k points.
__global__ __launch_bounds__(256) void k_bbox(const unsigned char* __restrict__ pts, size_t stride, int n, uint32_t* __restrict__ part)
{
    __shared__ float smn[4][3], smx[4][3];
    float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float* p = reinterpret_cast<const float*>(pts + (size_t)i * stride);
#pragma unroll
        for (int d = 0; d < 3; d++) {
            float v = p[d];
            if (isfinite(v)) { mn[d] = fminf(mn[d], v); mx[d] = fmaxf(mx[d], v); }
        }
    }
#pragma unroll
    for (int d = 0; d < 3; d++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mn[d] = fminf(mn[d], __shfl_down(mn[d], off, 64));
            mx[d] = fmaxf(mx[d], __shfl_down(mx[d], off, 64));
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < 3; d++) { smn[wave][d] = mn[d]; smx[wave][d] = mx[d]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int d = threadIdx.x;
        const float a = fminf(fminf(smn[0][d], smn[1][d]), fminf(smn[2][d], smn[3][d]));
        const float b = fmaxf(fmaxf(smx[0][d], smx[1][d]), fmaxf(smx[2][d], smx[3][d]));
        part[8 * blockIdx.x + d] = a <= b ? f2ord(a) : 0xffffffffu;          // (no finite value: the neutral elements)
        part[8 * blockIdx.x + 3 + d] = a <= b ? f2ord(b) : 0u;
    }
}
// mm[0..2] = min, mm[3..5] = max over the workgroups' boxes (0xffffffff / 0 where no coordinate was finite)
__global__ __launch_bounds__(256) void k_bbox_fold(const uint32_t* __restrict__ part, int nparts, uint32_t* __restrict__ mm)
{
    __shared__ uint32_t slo[4][3], shi[4][3];
    uint32_t lo[3] = { 0xffffffffu, 0xffffffffu, 0xffffffffu }, hi[3] = { 0u, 0u, 0u };
    for (int b = threadIdx.x; b < nparts; b += 256) {
#pragma unroll
        for (int d = 0; d < 3; d++) { lo[d] = min(lo[d], part[8 * b + d]); hi[d] = max(hi[d], part[8 * b + 3 + d]); }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int d = 0; d < 3; d++) {
            lo[d] = min(lo[d], (uint32_t)__shfl_down((int)lo[d], off, 64));
            hi[d] = max(hi[d], (uint32_t)__shfl_down((int)hi[d], off, 64));
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < 3; d++) { slo[wave][d] = lo[d]; shi[wave][d] = hi[d]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int d = threadIdx.x;
        mm[d] = min(min(slo[0][d], slo[1][d]), min(slo[2][d], slo[3][d]));
        mm[3 + d] = max(max(shi[0][d], shi[1][d]), max(shi[2][d], shi[3][d]));
    }
}

// linear cell id: x-fastest rows (map grid: a query's 3 x-neighbours are one contiguous run)
__device__ __forceinline__ int lin_rows(const GridDesc& g, int cx, int cy, int cz)
{
    return (cz * g.ny + cy) * g.nx + cx;
}
// Scan locality order (ordering only, never results): lidar returns are binned on a
// log-polar grid around the sensor (128 azimuth x 128 log-range bins; cell size grows with
// range like the return spacing does, so cells hold a few points each and the rank atomics
// do not pile up on the dense near-field cells), numbered along a Hilbert curve so that 64
// consecutive sorted points form a compact patch; a rigid transform keeps it compact.
// (kPolarCells, the number of cells, is s2m_types.h's: s2m_create sizes the cell counts by it.)
// Hilbert curve index of (x, y) on a 128 x 128 grid: consecutive indices are always adjacent
// cells (a Z-order curve jumps across the grid at every power-of-two boundary, and a wave that
// straddles a jump gets a huge bounding box).
__device__ __forceinline__ uint32_t hilbert128(uint32_t x, uint32_t y)
{
    uint32_t d = 0;
#pragma unroll
    for (uint32_t s = 64; s > 0; s >>= 1) {
        const uint32_t rx = (x & s) ? 1u : 0u, ry = (y & s) ? 1u : 0u;
        d += s * s * ((3u * rx) ^ ry);
        if (ry == 0) {
            if (rx == 1) { x = 127u - x; y = 127u - y; }
            const uint32_t t = x; x = y; y = t;
        }
    }
    return d;
}
__device__ __forceinline__ int polar_cell(float x, float y)
{
    const float rho = sqrtf(x * x + y * y);
    float az = atan2f(y, x);                                  // [-pi, pi]
    int ab = (int)((az + 3.14159265f) * (128.0f / 6.2831853f));
    ab = min(max(ab, 0), 127);
    float lr = (__log2f(fmaxf(rho, 0.5f)) + 1.0f) * (128.0f / 9.23f);   // 0.5 m .. 300 m
    int rb = (rho == rho) ? min(max((int)lr, 0), 127) : 0;
    if (!(az == az)) ab = 0;
    return (int)hilbert128((uint32_t)ab, (uint32_t)rb);
}

// Histogram with per-point rank, DETERMINISTIC: the position of a scan point in the locality order depends on the
// input alone, never on the order in which atomics happen to arrive - so the wave partition, the summation order of the
// normal equations and with them every bit of a registration's result are reproducible from run to run.
//   * inside a wave, points of the same cell are ranked by lane (match loop over the distinct cells of the wave);
//   * the 16 waves of a workgroup add their cell counts to the workgroup's LDS histogram one after the other;
//   * workgroup b writes its histogram as row b of a table; k_polar_prefix turns every column into an exclusive prefix
//     over the workgroups (rank of the workgroup's first point in that cell) and the cell totals.
// (Device-scope returning atomics, the obvious alternative, are also served memory-side on this multi-die part: 120 k
// of them cost 27 us.)
constexpr int kPolarBlock = 1024;
__global__ __launch_bounds__(kPolarBlock) void k_polar_count(const PrepTable tbl)
{
    const PrepSlot& ps = tbl.s[blockIdx.y];
    if ((int)blockIdx.x >= ps.npb) return;
    if (ps.stamps && blockIdx.x == 0 && threadIdx.x == 0) ps.stamps[0] = wall_clock64();      // the scan preparation starts (s2m_last_timing)
    const unsigned char* __restrict__ pts = ps.pts; const size_t stride = ps.stride; const int n = ps.n;
    int32_t* __restrict__ cell_of = ps.cell_of; int32_t* __restrict__ rank_of = ps.rank_of; int32_t* __restrict__ block_hist = ps.block_hist;
    __shared__ int32_t hist[kPolarCells];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int k = t; k < kPolarCells; k += kPolarBlock) hist[k] = 0;
    const int i = blockIdx.x * kPolarBlock + t;
    int c = -1;
    if (i < n) {
        const float* p = reinterpret_cast<const float*>(pts + (size_t)i * stride);
        c = polar_cell(p[0], p[1]);
    }
    // rank among the lanes of this wave that share the cell, the group's size and its first lane
    int r_in = 0, cnt = 0, leader = lane;
    unsigned long long todo = __ballot(c >= 0);
    while (todo) {
        const int first = (int)__builtin_ctzll(todo);
        const int v = __builtin_amdgcn_readlane(c, first);
        const unsigned long long same = __ballot(c == v);
        if (c == v) { r_in = __popcll(same & ((1ull << lane) - 1ull)); cnt = __popcll(same); leader = first; }
        todo &= ~same;
    }
    int base = 0;
    for (int w = 0; w < kPolarBlock / 64; w++) {
        __syncthreads();
        if (wave == w && c >= 0 && leader == lane) { base = hist[c]; hist[c] = base + cnt; }     // distinct cells per leader: no conflict
    }
    base = __shfl(base, leader, 64);
    __syncthreads();
    if (i < n) { cell_of[i] = c; rank_of[i] = base + r_in; }
    int32_t* row = block_hist + (size_t)blockIdx.x * kPolarCells;
    for (int k = t; k < kPolarCells; k += kPolarBlock) row[k] = hist[k];
}

// Column-wise exclusive prefix of the workgroup histograms over the workgroups, in place, and the cell totals.
// 64 columns x 16 segments of workgroups per 1024 threads: consecutive lanes read consecutive columns.
__global__ __launch_bounds__(1024) void k_polar_prefix(const PrepTable tbl)
{
    const PrepSlot& ps = tbl.s[blockIdx.y];
    if (ps.n <= 0) return;                                // an empty slot of a batch (its row of the table holds no buffers)
    int32_t* __restrict__ H = ps.block_hist; const int nb = ps.npb; int32_t* __restrict__ counts = ps.counts;
    __shared__ int32_t seg[16][64];
    const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    const int per = (nb + 15) / 16, b0 = min(s * per, nb), b1 = min(b0 + per, nb);
    int32_t sum = 0;
    for (int b = b0; b < b1; b++) sum += H[(size_t)b * kPolarCells + col];
    seg[s][lane] = sum;
    __syncthreads();
    int32_t run = 0, total = 0;
#pragma unroll
    for (int q = 0; q < 16; q++) { const int32_t v = seg[q][lane]; run += (q < s) ? v : 0; total += v; }
    if (s == 0) counts[col] = total;
    for (int b = b0; b < b1; b++) {
        const size_t at = (size_t)b * kPolarCells + col;
        const int32_t v = H[at];
        H[at] = run;
        run += v;
    }
}

// exclusive scan of the 16384 polar cell counts by one workgroup (16 per thread); the counts are
// zeroed as they are read, ready for the next scan
__global__ __launch_bounds__(1024) void k_polar_scan(const PrepTable tbl)
{
    const PrepSlot& ps = tbl.s[blockIdx.y];
    if (ps.n <= 0) return;                                // an empty slot of a batch
    int32_t* __restrict__ counts = ps.counts; int32_t* __restrict__ start = ps.cell_start;
    __shared__ int32_t wsum[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int32_t v[16];
    int32_t sum = 0;
    int4* c4 = reinterpret_cast<int4*>(counts + t * 16);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int4 q = c4[k];
        c4[k] = make_int4(0, 0, 0, 0);
        v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
        sum += q.x + q.y + q.z + q.w;
    }
    int32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        int32_t o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int32_t woff = 0;
    for (int w = 0; w < wave; w++) woff += wsum[w];
    int32_t run = woff + incl - sum;
    int4* s4 = reinterpret_cast<int4*>(start + t * 16);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int4 q;
        q.x = run; run += v[4 * k];
        q.y = run; run += v[4 * k + 1];
        q.z = run; run += v[4 * k + 2];
        q.w = run; run += v[4 * k + 3];
        s4[k] = q;
    }
}

__global__ void k_bin_count(const unsigned char* __restrict__ pts, size_t stride, int n, GridDesc g,
                            int32_t* __restrict__ cell_of, int32_t* __restrict__ rank_of,
                            int32_t* __restrict__ counts)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = reinterpret_cast<const float*>(pts + (size_t)i * stride);
    int cx = cell_coord(p[0], g.ox, g.inv_e, g.nx);
    int cy = cell_coord(p[1], g.oy, g.inv_e, g.ny);
    int cz = cell_coord(p[2], g.oz, g.inv_e, g.nz);
    int c = lin_rows(g, cx, cy, cz);
    cell_of[i] = c;
    rank_of[i] = atomicAdd(&counts[c], 1);
}

// exclusive scan, 1024 elements per 256-thread workgroup
__global__ __launch_bounds__(256) void k_scan_local(const int32_t* __restrict__ in, int32_t* __restrict__ out,
                                                    int32_t* __restrict__ block_sums, int n)
{
    __shared__ int32_t wsum[4];
    const int base = blockIdx.x * 1024 + threadIdx.x * 4;
    int32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = (base + k < n) ? in[base + k] : 0;
    int32_t t = v[0] + v[1] + v[2] + v[3];
    int32_t incl = t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        int32_t o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int32_t woff = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) if (w < wave) woff += wsum[w];
    int32_t excl = woff + incl - t;
#pragma unroll
    for (int k = 0; k < 4; k++) { if (base + k < n) out[base + k] = excl; excl += v[k]; }
    if (threadIdx.x == 255) block_sums[blockIdx.x] = woff + incl;
}

// in-place exclusive scan of the block sums by one workgroup (any nb)
__global__ __launch_bounds__(1024) void k_scan_sums(int32_t* __restrict__ sums, int nb)
{
    __shared__ int32_t wsum[16];
    __shared__ int32_t carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int base = 0; base < nb; base += 1024) {
        int i = base + threadIdx.x;
        int32_t t = (i < nb) ? sums[i] : 0;
        int32_t incl = t;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            int32_t o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int32_t woff = 0;
        for (int w = 0; w < wave; w++) woff += wsum[w];
        int32_t carry = carry_s;
        if (i < nb) sums[i] = carry + woff + incl - t;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = carry + woff + incl;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_scan_add(int32_t* __restrict__ out, const int32_t* __restrict__ block_sums,
                                                  int n, int total)
{
    const int base = blockIdx.x * 1024 + threadIdx.x * 4;
    const int32_t off = block_sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < 4; k++) if (base + k < n) out[base + k] += off;
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = total;
}

// k_scan_sums and k_scan_add in one launch for grids of up to a few thousand workgroups: every workgroup adds up the sums of the
// workgroups before it for itself (block_sums as k_scan_local left them)
__global__ __launch_bounds__(256) void k_scan_add_fold(int32_t* __restrict__ out, const int32_t* __restrict__ block_sums, int n, int total)
{
    __shared__ int32_t wsum[4];
    int32_t before = 0;
    for (int j = threadIdx.x; j < (int)blockIdx.x; j += 256) before += block_sums[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = before;
    __syncthreads();
    const int32_t off = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    const int base = blockIdx.x * 1024 + threadIdx.x * 4;
#pragma unroll
    for (int k = 0; k < 4; k++) if (base + k < n) out[base + k] += off;
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = total;
}

__global__ void k_scatter_map(const unsigned char* __restrict__ pts, size_t stride, int n,
                              const int32_t* __restrict__ cell_of, const int32_t* __restrict__ rank_of,
                              const int32_t* __restrict__ cell_start, float4* __restrict__ map_sorted)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = reinterpret_cast<const float*>(pts + (size_t)i * stride);
    int pos = cell_start[cell_of[i]] + rank_of[i];
    map_sorted[pos] = make_float4(p[0], p[1], p[2], __int_as_float(i));
}

__global__ void k_scatter_scan(const PrepTable tbl)
{
    const PrepSlot& ps = tbl.s[blockIdx.y];
    const unsigned char* __restrict__ pts = ps.pts; const size_t stride = ps.stride; const int n = ps.n;
    const int32_t* __restrict__ cell_of = ps.cell_of; const int32_t* __restrict__ rank_of = ps.rank_of;
    const int32_t* __restrict__ cell_start = ps.cell_start; const int32_t* __restrict__ block_hist = ps.block_hist;
    float* __restrict__ qx = ps.qx; float* __restrict__ qy = ps.qy; float* __restrict__ qz = ps.qz;
    int32_t* __restrict__ qperm = ps.qperm; float4* __restrict__ cert = ps.cert; int4* __restrict__ aux = ps.aux;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = reinterpret_cast<const float*>(pts + (size_t)i * stride);
    const int c = cell_of[i];
    // first point of the cell + points of the cell in earlier workgroups of k_polar_count + rank inside the workgroup
    int pos = cell_start[c] + block_hist[(size_t)(i / kPolarBlock) * kPolarCells + c] + rank_of[i];
    if ((unsigned)pos >= (unsigned)n) return;            // cannot happen while the histogram is consistent
    qx[pos] = p[0]; qy[pos] = p[1]; qz[pos] = p[2]; qperm[pos] = i;
    cert[pos] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);     // a new scan: no certificate (slack 0), no neighbour tuple, no plane
    aux[pos] = make_int4(0, 0, 0, 0);
}

// k_polar_scan and k_scatter_scan in one launch (a single scan): every 1024-point workgroup builds the exclusive scan of the
// 16384 cell totals for itself in LDS - k_polar_scan's integer arithmetic, 16 counts per thread, a wave scan, 16 wave sums -
// and places its points as k_scatter_scan does, with cell_start[c] taken from LDS.  Nothing else reads q_cell_start, and
// k_polar_prefix rewrites every count, so neither the scan's result nor zeroed counts are left in memory.
// (The 16 wave sums pass through the first words of the 64 KB array before the scan overwrites them.)
__global__ __launch_bounds__(1024) void k_scatter_scan_fold(const PrepTable tbl)
{
    const PrepSlot& ps = tbl.s[blockIdx.y];
    const int n = ps.n;
    if (n <= 0 || (int)blockIdx.x * 1024 >= n) return;    // (uniform per workgroup)
    const unsigned char* __restrict__ pts = ps.pts; const size_t stride = ps.stride;
    const int32_t* __restrict__ cell_of = ps.cell_of; const int32_t* __restrict__ rank_of = ps.rank_of;
    const int32_t* __restrict__ counts = ps.counts; const int32_t* __restrict__ block_hist = ps.block_hist;
    float* __restrict__ qx = ps.qx; float* __restrict__ qy = ps.qy; float* __restrict__ qz = ps.qz;
    int32_t* __restrict__ qperm = ps.qperm; float4* __restrict__ cert = ps.cert; int4* __restrict__ aux = ps.aux;
    __shared__ int32_t start[kPolarCells];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i = blockIdx.x * 1024 + t;
    // the point's own loads first: they are in flight while the scan is built
    int c = 0, rank = 0, before = 0;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (i < n) {
        const float* p = reinterpret_cast<const float*>(pts + (size_t)i * stride);
        c = cell_of[i]; rank = rank_of[i];
        px = p[0]; py = p[1]; pz = p[2];
        before = block_hist[(size_t)blockIdx.x * kPolarCells + c];     // (i / kPolarBlock == blockIdx.x: both are 1024)
    }
    int32_t v[16];
    int32_t sum = 0;
    const int4* c4 = reinterpret_cast<const int4*>(counts + t * 16);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int4 q = c4[k];
        v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
        sum += q.x + q.y + q.z + q.w;
    }
    int32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        int32_t o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) start[wave] = incl;
    __syncthreads();
    int32_t woff = 0;
    for (int w = 0; w < wave; w++) woff += start[w];
    __syncthreads();
    int32_t run = woff + incl - sum;
    int4* s4 = reinterpret_cast<int4*>(start + t * 16);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int4 q;
        q.x = run; run += v[4 * k];
        q.y = run; run += v[4 * k + 1];
        q.z = run; run += v[4 * k + 2];
        q.w = run; run += v[4 * k + 3];
        s4[k] = q;
    }
    __syncthreads();
    if (i >= n) return;
    // first point of the cell + points of the cell in earlier workgroups of k_polar_count + rank inside the workgroup
    const int pos = start[c] + before + rank;
    if ((unsigned)pos >= (unsigned)n) return;            // cannot happen while the histogram is consistent
    qx[pos] = px; qy[pos] = py; qz[pos] = pz; qperm[pos] = i;
    cert[pos] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);     // a new scan: no certificate (slack 0), no neighbour tuple, no plane
    aux[pos] = make_int4(0, 0, 0, 0);
}

// Work-proportional wave assignment.  The sorted scan is cut into chunks of 64 points; a chunk
// whose points spread over a large box (sparse far field, tall structures) would make its wave
// stage and sweep a large map tile, and the slowest wave sets the kernel time.  Such chunks are
// given to 2, 4 or 8 waves (32 / 16 / 8 points each: tighter boxes, run in parallel).  The extent is
// measured in the lidar frame - a rigid transform does not change it.
__global__ __launch_bounds__(256) void k_chunk_parts(const PrepTable tbl)
{
    const PrepSlot& ps = tbl.s[blockIdx.y];
    float* __restrict__ qx = ps.qx; float* __restrict__ qy = ps.qy; float* __restrict__ qz = ps.qz; int32_t* __restrict__ qperm = ps.qperm;
    const int n = ps.n, n_chunks = ps.n_chunks, base_parts = ps.base_parts; int32_t* __restrict__ parts = ps.chunk_parts;
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= n_chunks) return;
    const int i = c * 64 + lane;
    const bool v = i < n;
    float x = v ? qx[i] : 0.0f, y = v ? qy[i] : 0.0f, z = v ? qz[i] : 0.0f;
    int perm = v ? qperm[i] : 0;
    const bool f = v && fabsf(x) < 3.0e38f && fabsf(y) < 3.0e38f && fabsf(z) < 3.0e38f;
    float mn[3] = { f ? x : INFINITY, f ? y : INFINITY, f ? z : INFINITY };
    float mx[3] = { f ? x : -INFINITY, f ? y : -INFINITY, f ? z : -INFINITY };
#pragma unroll
    for (int d = 0; d < 3; d++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mn[d] = fminf(mn[d], __shfl_xor(mn[d], off, 64));
            mx[d] = fmaxf(mx[d], __shfl_xor(mx[d], off, 64));
        }
    }
    // Order inside the chunk: the polar cells ignore height and the rank inside a cell is arbitrary, so
    // the 64 points of a chunk are in no useful order, and cutting the chunk into 2..8 waves would leave
    // every part as large as the whole.  Sort the chunk along a 3-D Morton curve over its own bounding
    // box (cubic cells, 16 along the longest axis; bitonic network over the wave, ties by scan index:
    // deterministic), so that every part is a compact blob whatever the sensor's heading is.  Lanes past
    // the end of the scan and non-finite points sort last.
    if (mn[0] <= mx[0]) {
        const float emax = fmaxf(fmaxf(mx[0] - mn[0], mx[1] - mn[1]), mx[2] - mn[2]);
        const float sc = emax > 0.0f ? 15.99f / emax : 0.0f;
        auto spread4 = [](uint32_t b) { return (b & 1u) | ((b & 2u) << 2) | ((b & 4u) << 4) | ((b & 8u) << 6); };   // bit k -> bit 3k
        uint32_t key = 0x7fffffffu;
        if (f) {
            const uint32_t ix = (uint32_t)((x - mn[0]) * sc), iy = (uint32_t)((y - mn[1]) * sc), iz = (uint32_t)((z - mn[2]) * sc);
            key = spread4(min(ix, 15u)) | (spread4(min(iy, 15u)) << 1) | (spread4(min(iz, 15u)) << 2);
        }
        int ord = v ? perm : 0x7fffffff;
#pragma unroll
        for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) {
                const uint32_t okey = (uint32_t)__shfl_xor((int)key, j, 64);
                const int oord = __shfl_xor(ord, j, 64), operm = __shfl_xor(perm, j, 64);
                const float ox = __shfl_xor(x, j, 64), oy = __shfl_xor(y, j, 64), oz = __shfl_xor(z, j, 64);
                const bool lower = (lane & j) == 0, asc = (lane & k) == 0;
                const bool mine_first = (key < okey) || (key == okey && ord < oord);     // (key, ord) pairs of real points are distinct
                const bool keep = (lower == asc) ? mine_first : !mine_first;
                if (!keep) { key = okey; ord = oord; perm = operm; x = ox; y = oy; z = oz; }
            }
        }
        if (v) { qx[i] = x; qy[i] = y; qz[i] = z; qperm[i] = perm; }
    }
    if (lane == 0) {
        int p = 1;
        if (mn[0] <= mx[0]) {
            // cells a wave's box would span (1 m cells, +1 halo each side, bound radius)
            const float vol = (mx[0] - mn[0] + 3.0f) * (mx[1] - mn[1] + 3.0f) * (mx[2] - mn[2] + 3.0f);
            p = vol > 700.0f ? 4 : (vol > 180.0f ? 2 : 1);
        }
        // a small scan leaves most of the GPU idle: cut every chunk finer (base_parts) and large ones finer still
        parts[c] = min(8, max(p, base_parts) * ((p > 1 && base_parts > 1) ? 2 : 1));
    }
    // the last ordering kernel of a single scan: its last chunk's wave stamps the end of the preparation (s2m_last_timing)
    if (ps.stamps && c == n_chunks - 1 && lane == 0) ps.stamps[1] = wall_clock64();
}

}  // namespace s2m
