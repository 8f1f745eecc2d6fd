// s2m_icp.hip — pcl::IterativeClosestPoint (PCL 1.10 [ext]: registration/impl/icp.hpp,
// correspondence_estimation.hpp, transformation_estimation_svd.hpp -> Eigen::umeyama,
// default_convergence_criteria.hpp, Registration::getFitnessScore) on gfx950, see s2m_icp.hpp.
//
// Per iteration: (1) exact nearest target point of every (already transformed) source point - a tiled
// brute force, target slices staged through LDS, the winner of each source point settled across slices
// by one 64-bit atomicMin on (d2 bits << 32 | target index), i.e. ties go to the lower index like the
// oracle; loop-closure submaps are 1e3..1e5 points, so the whole search is a few 1e8..1e9 distance
// evaluations spread over ~1000 workgroups; (2) one pass over the correspondences within the distance
// limit accumulates count, sum d2, the two centroids and the raw cross moments in fp64 (17 numbers): every
// workgroup writes its partial row, one workgroup folds the rows in workgroup order (no atomics, so the sums
// and everything after them are the same bits from run to run - fp64 adds in arrival order were not, at
// 20 km from the origin one fp32 ulp of the covariance); the host turns them into Eigen::umeyama's mean / covariance, does the 3x3 SVD, the pose composition and
// the convergence state machine exactly as PCL does; (3) the source cloud is transformed in place by the
// incremental transform, as PCL transforms input_transformed.  fp32 distances use the operation order
// of the oracle ((dx*dx + dy*dy) + dz*dz, -ffp-contract=off), so correspondences are identical to it.
//
// The device loop (icp_dev_*, what s2m_loop_*_launch and s2m_loop_verify_launch queue) is the same alignment without the host in
// it: (1) becomes an exact 1-NN through a uniform grid over the target, built once per alignment, with a brute-force worklist for
// the points the grid does not settle (same keys); the host's part of (2) becomes k_icp_close, which runs the host loop's own
// source (s2m_icp_close.hpp); iterations are queued in ranges and every kernel behind the end of the alignment returns at entry.
// The loop carries up to kIcpMaxSlots alignments of one source at once, the slot a grid dimension of every kernel; the single
// alignment is its one-slot case. Every slot owns its moving copy of the source, so each may start from a guess of its own
// (align(output, guess): IcpGuesses, the source moved as it is loaded, the state's T started at the guess).
// A second layout beside the slots carries up to kIcpMaxPairs alignments that each have a source of their own (IcpForm::kTable, what
// s2m_loop_verify_many queues): the pairs' descriptions are a table in device memory, uploaded once per alignment set. The host
// starts and advances either form through one driver over one layout (s2m_icp_layout.hpp); the caller names the form. The kernels
// of the loop are written once over "the view of slot s" and instantiated for both layouts; what a kernel derives from the launch
// where all slots share n_src (the partial rows, the stride over the source) is the pair's own in the table form.
// The kernels are one set but for two. The host loop (icp_align) launches the loop's load, reset, sums and fold on the one-slot
// layout and differs in who closes an iteration (the host, after a wait), in the search (always the brute force, through k_icp_nn:
// k_icp_nn_list over every source computes the same keys but cost the loop 2-3 % of its time) and in k_icp_transform, which takes
// the step from the host.
// DESIGN.md section 12 has the stopping rule of the grid search and its derivation, and the slot layout.
#include "s2m_icp.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <new>
#include <type_traits>

#include "s2m_icp_close.hpp"

namespace s2m {

namespace {

constexpr unsigned long long kNoMatch = ~0ull;      // (kNnThreads, kNnTile, kSumBlocks: s2m_icp_layout.hpp)

struct Buf {
    void*  p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        const size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// the tile loop of the brute-force search: target points [j0, j1) staged through LDS in tiles of kNnTile, the nearest of them to p
// (lowest index among equals) left in bd / bi. Every thread of the workgroup calls it (the staging is collective).
__device__ __forceinline__ void nn_tiles(const float4 p, const bool fin, const float4* __restrict__ tgt, const int j0, const int j1,
                                         float4* tile, float& bd, int& bi)
{
    for (int base = j0; base < j1; base += kNnTile) {
        const int m = min(kNnTile, j1 - base);
        __syncthreads();
        for (int k = threadIdx.x; k < m; k += kNnThreads) tile[k] = tgt[base + k];
        __syncthreads();
        if (fin) {
            int k = 0;
            for (; k + 4 <= m; k += 4) {
                const float4 a = tile[k], b = tile[k + 1], c = tile[k + 2], d = tile[k + 3];
                const float ax = p.x - a.x, ay = p.y - a.y, az = p.z - a.z, bx = p.x - b.x, by = p.y - b.y, bz = p.z - b.z;
                const float cx = p.x - c.x, cy = p.y - c.y, cz = p.z - c.z, dx = p.x - d.x, dy = p.y - d.y, dz = p.z - d.z;
                const float da = (ax * ax + ay * ay) + az * az, db = (bx * bx + by * by) + bz * bz;
                const float dc = (cx * cx + cy * cy) + cz * cz, dd = (dx * dx + dy * dy) + dz * dz;
                if (da < bd) { bd = da; bi = base + k; }
                if (db < bd) { bd = db; bi = base + k + 1; }
                if (dc < bd) { bd = dc; bi = base + k + 2; }
                if (dd < bd) { bd = dd; bi = base + k + 3; }
            }
            for (; k < m; k++) {
                const float4 a = tile[k];
                const float ax = p.x - a.x, ay = p.y - a.y, az = p.z - a.z;
                const float da = (ax * ax + ay * ay) + az * az;
                if (da < bd) { bd = da; bi = base + k; }
            }
        }
    }
}

// The host loop's search: grid (source blocks, target slices), 256 source points against target points [slice*len, (slice+1)*len).
// It is k_icp_nn_list without list, slot and guard, kept as a kernel of its own because it is measurably faster there (DESIGN.md
// section 12): the loop waits for every iteration, and this kernel reaches its six arguments in one round trip.
__global__ __launch_bounds__(kNnThreads) void k_icp_nn(const float4* __restrict__ cur, int n_src, const float4* __restrict__ tgt, int n_tgt,
                                                       int slice_len, unsigned long long* __restrict__ best)
{
    __shared__ float4 tile[kNnTile];
    const int i = blockIdx.x * kNnThreads + threadIdx.x;
    const bool valid = i < n_src;
    const float4 p = valid ? cur[i] : make_float4(0, 0, 0, 0);
    const bool fin = valid && isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    float bd = INFINITY;
    int bi = -1;
    const int j0 = blockIdx.y * slice_len, j1 = min(j0 + slice_len, n_tgt);
    nn_tiles(p, fin, tgt, j0, j1, tile, bd, bi);
    if (fin && bi >= 0)       // d2 >= 0: its bit pattern orders like the value; NaN distances (non-finite targets) never win above
        atomicMin(&best[i], ((unsigned long long)__float_as_uint(bd) << 32) | (unsigned)bi);
}

struct Mat34 { float m[12]; };
__device__ __forceinline__ void transform_body(float4* __restrict__ cur, int n, const float* m)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = cur[i];
    cur[i] = make_float4(m[0] * p.x + m[1] * p.y + m[2]  * p.z + m[3],
                         m[4] * p.x + m[5] * p.y + m[6]  * p.z + m[7],
                         m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11], 0.0f);
}

__global__ __launch_bounds__(256) void k_icp_transform(float4* __restrict__ cur, int n, Mat34 T)
{
    transform_body(cur, n, T.m);
}


// ---- the device loop (icp_dev_*): an alignment that is queued and left alone ------------------------------------------------
// Everything the loop carries lives in one device block, copied to the host in one piece at the end of a range of iterations.
// phase 0 = a kernel of the iteration loop: it returns at entry once st.done is set (the idiom of k_pg_cg_*: no kernel waits on
// another, the launches queued behind the end of an alignment are idle); phase 1 = the fitness pass, which runs after it, and
// every launch of the host loop, which keeps its state on the host.

struct IcpGrid {
    float lo[3];           // least finite target coordinate per axis: the grid's origin
    float inv, cell;       // cell edge and 1.0f / cell (the edge asked for, or a larger one where the box needs more than kGridMaxCells)
    int   n[3];            // cells per axis; a target's cell is floor((x - lo) * inv) per axis, x fastest
    int   n_fin;           // finite targets (0: no source has a match)
    int   usable;          // 0: no grid was built (an extent that overflows fp32) - every source goes to the brute force
};

struct IcpDevBlock {
    IcpLoopState st;
    IcpGrid      g;
    unsigned     bbox[6];  // ordered-integer images of the finite targets' min (0..2) and max (3..5)
    int          wl_count; // sources on the fallback list of the search in flight; k_icp_fold_dev zeroes it
    int          n_fallback;   // wl_count of the search closed last
    double       sums[17];
    double       pad;
};

constexpr int kGridMaxCells = 1 << 18;
constexpr int kGridThreads = 64;                    // one wave per workgroup: a few thousand source points reach ~50 CUs
constexpr double kFaceSlack = 0x1p-22;              // 4 fp32 roundings: (x - lo) * inv with inv = 1 / cell rounds three times
constexpr double kBoundSlack = 1e-6;                // > 6 fp32 roundings of d2 = (dx*dx + dy*dy) + dz*dz from the exact distance

__device__ __forceinline__ unsigned ord_of(float f) { const unsigned b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float ord_to(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }
__device__ __forceinline__ bool done_guard(const IcpDevBlock* blk, int phase) { return phase == 0 && blk->st.done != 0; }
// the cell coordinate along one axis before floor and clamp: non-decreasing in x (a subtraction of and a product with constants)
__device__ __forceinline__ float cell_coord(float x, float lo, float inv) { return (x - lo) * inv; }

// The view of slot s: what a kernel of the loop reads about the alignment it works on. The kernels are written once over it and
// instantiated twice: for IcpSlots by value, which builds the view from its arrays (n_src shared, rows and guess not in it: the
// launch carries them), and for the pair table (IcpPairs), whose entries are views in device memory with every field the pair's own.
struct IcpView {
    float4*             cur;                     // the moving source, n_src points
    const float4*       tgt;
    unsigned long long* best;
    double*             part;
    int*                list;                    // the fallback list of the grid search
    float4*             gsorted;                 // the targets sorted by cell
    IcpDevBlock*        blk;
    int*                gcount;                  // kGridMaxCells ints, as gstart and gend
    int*                gstart;
    int*                gend;
    const unsigned char* d_src;                  // (table only) the records the source and the target are loaded from
    const unsigned char* d_tgt;
    int                 n_tgt;
    int                 slice_len;               // the brute force's target slice (nn_shape of this slot)
    int                 n_src;
    int                 rows;                    // (table only) partial rows: min(ceil(n_src / 256), kSumBlocks)
    int                 guess_set;               // (table only) the guess, as IcpGuesses holds it
    float               guess[16];
};

// The slots of the loop: one source against K <= kIcpMaxSlots targets, K independent alignments advanced by the same launches.
// Every kernel of the loop takes this struct by value (as k_icp_transform takes Mat34: nothing is uploaded per launch) and its
// slot from blockIdx.z; grids are sized by the largest slot and a workgroup beyond its own slot's extent returns at entry.
// Inside a slot nothing differs from the single alignment, which is the K = 1 case: the same per-point arithmetic, the same
// (d2, original index) minimum, the same number of partial rows (it depends on n_src only), the same fold, the same close.
struct IcpSlots {
    static constexpr bool kPerPair = false;      // one n_src: every slot has the launch's rows, no workgroup is beyond them
    float4*             cur[kIcpMaxSlots];       // the moving source, n_src points each
    const float4*       tgt[kIcpMaxSlots];
    unsigned long long* best[kIcpMaxSlots];
    double*             part[kIcpMaxSlots];
    int*                list[kIcpMaxSlots];      // the fallback list of the grid search
    float4*             gsorted[kIcpMaxSlots];   // the targets sorted by cell
    int                 n_tgt[kIcpMaxSlots];
    int                 slice_len[kIcpMaxSlots]; // the brute force's target slice (nn_shape of this slot)
    IcpDevBlock*        blk;                     // K blocks back to back: one copy per range brings them all
    int*                gcount;                  // kGridMaxCells ints per slot, as gstart and gend
    int*                gstart;
    int*                gend;
    int                 n_src;
    // the view of slot s: each field read from the kernel's arguments where the kernel asks for it
    struct Ref {
        const IcpSlots& S;
        const int s;
        __device__ __forceinline__ float4* cur() const { return S.cur[s]; }
        __device__ __forceinline__ const float4* tgt() const { return S.tgt[s]; }
        __device__ __forceinline__ unsigned long long* best() const { return S.best[s]; }
        __device__ __forceinline__ double* part() const { return S.part[s]; }
        __device__ __forceinline__ int* list() const { return S.list[s]; }
        __device__ __forceinline__ float4* gsorted() const { return S.gsorted[s]; }
        __device__ __forceinline__ IcpDevBlock* blk() const { return S.blk + s; }
        __device__ __forceinline__ int* gcount() const { return S.gcount + (size_t)s * kGridMaxCells; }
        __device__ __forceinline__ int* gstart() const { return S.gstart + (size_t)s * kGridMaxCells; }
        __device__ __forceinline__ int* gend() const { return S.gend + (size_t)s * kGridMaxCells; }
        __device__ __forceinline__ int n_tgt() const { return S.n_tgt[s]; }
        __device__ __forceinline__ int slice_len() const { return S.slice_len[s]; }
        __device__ __forceinline__ int n_src() const { return S.n_src; }
        __device__ __forceinline__ int rows() const { return 0; }             // (kPerPair only: the launch carries the rows)
    };
    __device__ __forceinline__ Ref view(int s) const { return Ref{ *this, s }; }
    __device__ __forceinline__ const IcpView* table() const { return nullptr; }
};

// The pairs of the loop: P <= kIcpMaxPairs alignments, each with its own source, target and guess. The table is an array of views
// in device memory, written in pinned host memory and uploaded once per alignment set ahead of the first kernel; a kernel takes
// its address and finds its pair by blockIdx.z. Grids are sized by the largest pair; what a slot's kernels derive from the launch
// (the partial rows and their stride) is here the pair's own, so that a pair computes what it computes alone.
struct IcpPairs {
    static constexpr bool kPerPair = true;
    const IcpView* t;
    struct Ref {
        const IcpView& p;
        __device__ __forceinline__ float4* cur() const { return p.cur; }
        __device__ __forceinline__ const float4* tgt() const { return p.tgt; }
        __device__ __forceinline__ unsigned long long* best() const { return p.best; }
        __device__ __forceinline__ double* part() const { return p.part; }
        __device__ __forceinline__ int* list() const { return p.list; }
        __device__ __forceinline__ float4* gsorted() const { return p.gsorted; }
        __device__ __forceinline__ IcpDevBlock* blk() const { return p.blk; }
        __device__ __forceinline__ int* gcount() const { return p.gcount; }
        __device__ __forceinline__ int* gstart() const { return p.gstart; }
        __device__ __forceinline__ int* gend() const { return p.gend; }
        __device__ __forceinline__ int n_tgt() const { return p.n_tgt; }
        __device__ __forceinline__ int slice_len() const { return p.slice_len; }
        __device__ __forceinline__ int n_src() const { return p.n_src; }
        __device__ __forceinline__ int rows() const { return p.rows; }
    };
    __device__ __forceinline__ Ref view(int s) const { return Ref{ t[s] }; }
    __device__ __forceinline__ const IcpView* table() const { return t; }
};

// The initial guesses of the slots (pcl::IterativeClosestPoint::align(output, guess)): slot s with set[s] starts its
// final_transformation_ at T[s] (row-major 4x4) and its moving source at T[s] * source; a slot without one starts at the identity
// with the source as it is (PCL: `if (guess != Matrix4::Identity())`), which is the loop as it was before there were guesses.
struct IcpGuesses {
    float T[kIcpMaxSlots][16];
    int   set[kIcpMaxSlots];
    __device__ __forceinline__ const float* of(int s, const IcpView*) const { return set[s] ? T[s] : nullptr; }
};
// the table form: the guess is in the pair's view
struct IcpPairGuesses {
    int unused;
    __device__ __forceinline__ const float* of(int s, const IcpView* t) const { return t[s].guess_set ? t[s].guess : nullptr; }
};

// one load: n records at src to float4 at dst, moved by the 3x4 m where move is set
struct IcpLoadItem { const unsigned char* src; float4* dst; int n; int move; const float* m; };

// records to float4 per slot: the K targets, or the one source into every slot's moving copy - there moved by the slot's guess
// where it has one (move[s]; m[s]: the guess's 3x4), in transform_body's arithmetic
struct IcpLoad {
    const unsigned char* src[kIcpMaxSlots];
    float4*              dst[kIcpMaxSlots];
    int                  n[kIcpMaxSlots];
    int                  move[kIcpMaxSlots];
    float                m[kIcpMaxSlots][12];
    __device__ __forceinline__ IcpLoadItem item(int s) const { return IcpLoadItem{ src[s], dst[s], n[s], move[s], m[s] }; }
};
// the table form. what: 0 the targets, 1 the sources as they are (the fitness pass), 2 the sources moved by their guesses
struct IcpPairLoad {
    const IcpView* t;
    int what;
    __device__ __forceinline__ IcpLoadItem item(int s) const
    {
        const IcpView& v = t[s];
        if (what == 0) return IcpLoadItem{ v.d_tgt, const_cast<float4*>(v.tgt), v.n_tgt, 0, v.guess };
        return IcpLoadItem{ v.d_src, v.cur, v.n_src, what == 2 ? v.guess_set : 0, v.guess };
    }
};

template <class L>
__global__ __launch_bounds__(256) void k_icp_load_slots(L ld, size_t stride)
{
    const IcpLoadItem it = ld.item(blockIdx.z);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= it.n) return;
    const float* p = reinterpret_cast<const float*>(it.src + (size_t)i * stride);
    const float x = p[0], y = p[1], z = p[2];
    if (!it.move) { it.dst[i] = make_float4(x, y, z, 0.0f); return; }
    const float* m = it.m;
    it.dst[i] = make_float4(m[0] * x + m[1] * y + m[2]  * z + m[3],
                            m[4] * x + m[5] * y + m[6]  * z + m[7],
                            m[8] * x + m[9] * y + m[10] * z + m[11], 0.0f);
}

template <class V, class GV>
__global__ __launch_bounds__(64) void k_icp_begin(V S, GV G)
{
    if (threadIdx.x != 0) return;
    IcpDevBlock* blk = S.view(blockIdx.z).blk();
    icp_state_init(&blk->st, G.of(blockIdx.z, S.table()));
    for (int a = 0; a < 3; a++) { blk->bbox[a] = 0xffffffffu; blk->bbox[3 + a] = 0u; }
    blk->wl_count = 0; blk->n_fallback = 0;
    blk->g.n_fin = 0; blk->g.usable = 0;
}

template <class V>
__global__ __launch_bounds__(256) void k_icp_grid_bbox(V S)
{
    __shared__ unsigned sh[4][6];
    const auto v = S.view(blockIdx.z);
    const int n = v.n_tgt();
    if ((int)(blockIdx.x * blockDim.x) >= n) return;
    const float4* __restrict__ tgt = v.tgt();
    IcpDevBlock* blk = v.blk();
    unsigned lo[3] = { 0xffffffffu, 0xffffffffu, 0xffffffffu }, hi[3] = { 0u, 0u, 0u };
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 t = tgt[i];
        if (!(isfinite(t.x) && isfinite(t.y) && isfinite(t.z))) continue;
        const unsigned o[3] = { ord_of(t.x), ord_of(t.y), ord_of(t.z) };
#pragma unroll
        for (int a = 0; a < 3; a++) { lo[a] = min(lo[a], o[a]); hi[a] = max(hi[a], o[a]); }
    }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo[a] = min(lo[a], (unsigned)__shfl_down((int)lo[a], off, 64));
            hi[a] = max(hi[a], (unsigned)__shfl_down((int)hi[a], off, 64));
        }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int a = 0; a < 3; a++) { sh[wave][a] = lo[a]; sh[wave][3 + a] = hi[a]; }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&blk->bbox[threadIdx.x], min(min(sh[0][threadIdx.x], sh[1][threadIdx.x]), min(sh[2][threadIdx.x], sh[3][threadIdx.x])));
    else if (threadIdx.x < 6) atomicMax(&blk->bbox[threadIdx.x], max(max(sh[0][threadIdx.x], sh[1][threadIdx.x]), max(sh[2][threadIdx.x], sh[3][threadIdx.x])));
}

// the grid's shape from the box: the edge asked for, enlarged until the box needs no more than kGridMaxCells cells
template <class V>
__global__ __launch_bounds__(64) void k_icp_grid_setup(V S, float cell_req)
{
    if (threadIdx.x != 0) return;
    IcpDevBlock* blk = S.view(blockIdx.z).blk();
    IcpGrid g{};
    if (blk->bbox[0] == 0xffffffffu) { blk->g = g; return; }             // no finite target: n_fin stays 0
    float hi[3];
    bool ok = true;
    for (int a = 0; a < 3; a++) {
        g.lo[a] = ord_to(blk->bbox[a]); hi[a] = ord_to(blk->bbox[3 + a]);
        ok = ok && isfinite(hi[a] - g.lo[a]);
    }
    float cell = cell_req;
    for (int tries = 0; ok && tries < 96; tries++) {
        const float inv = 1.0f / cell;
        double prod = 1.0;
        float fn[3];
        for (int a = 0; a < 3; a++) { fn[a] = floorf(cell_coord(hi[a], g.lo[a], inv)) + 1.0f; prod *= (double)fn[a]; }
        if (isfinite(inv) && inv > 0.0f && prod <= (double)kGridMaxCells) {
            g.cell = cell; g.inv = inv;
            for (int a = 0; a < 3; a++) g.n[a] = (int)fn[a];
            g.usable = 1;
            break;
        }
        if (!isfinite(cell) || !(prod == prod)) break;
        cell *= fmaxf(1.1f, cbrtf((float)(prod / (double)kGridMaxCells)) * 1.02f);
    }
    g.n_fin = 1;                                                          // counted by k_icp_grid_count; > 0 here
    blk->g = g;
}

__device__ __forceinline__ int cell_of(const IcpGrid& g, const float4 t)
{
    const int cx = (int)floorf(cell_coord(t.x, g.lo[0], g.inv)), cy = (int)floorf(cell_coord(t.y, g.lo[1], g.inv));
    const int cz = (int)floorf(cell_coord(t.z, g.lo[2], g.inv));
    // inside by construction (n = cell of the box's upper corner + 1 by the same expression); the clamp only guards the stores
    return (min(max(cz, 0), g.n[2] - 1) * g.n[1] + min(max(cy, 0), g.n[1] - 1)) * g.n[0] + min(max(cx, 0), g.n[0] - 1);
}

template <class V>
__global__ __launch_bounds__(256) void k_icp_grid_count(V S)
{
    const auto v = S.view(blockIdx.z);
    const IcpDevBlock* blk = v.blk();
    int* __restrict__ counts = v.gcount();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.n_tgt() || !blk->g.usable) return;
    const float4 t = v.tgt()[i];
    if (!(isfinite(t.x) && isfinite(t.y) && isfinite(t.z))) return;
    atomicAdd(&counts[cell_of(blk->g, t)], 1);
}

// exclusive scan of the cell counts in one workgroup: cstart[c] = first slot of cell c, cursor[c] the same (k_icp_grid_scatter
// advances it to the cell's end, which is the next cell's start)
template <class V>
__global__ __launch_bounds__(1024) void k_icp_grid_scan(V S)
{
    __shared__ int sh[1024];
    const auto v = S.view(blockIdx.z);
    IcpDevBlock* blk = v.blk();
    if (!blk->g.usable) return;
    const int* __restrict__ counts = v.gcount();
    int* __restrict__ cstart = v.gstart();
    int* __restrict__ cursor = v.gend();
    const int ncells = blk->g.n[0] * blk->g.n[1] * blk->g.n[2];
    const int per = (ncells + 1023) / 1024;
    const int c0 = min(threadIdx.x * per, ncells), c1 = min(c0 + per, ncells);
    int sum = 0;
    for (int c = c0; c < c1; c++) sum += counts[c];
    sh[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
        __syncthreads();
        sh[threadIdx.x] += v;
        __syncthreads();
    }
    int run = sh[threadIdx.x] - sum;
    for (int c = c0; c < c1; c++) { cstart[c] = run; cursor[c] = run; run += counts[c]; }
    if (threadIdx.x == 1023) blk->g.n_fin = sh[1023];
}

template <class V>
__global__ __launch_bounds__(256) void k_icp_grid_scatter(V S)
{
    const auto v = S.view(blockIdx.z);
    const int n = v.n_tgt();
    const IcpDevBlock* blk = v.blk();
    int* __restrict__ cursor = v.gend();
    float4* __restrict__ sorted = v.gsorted();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !blk->g.usable) return;
    const float4 t = v.tgt()[i];
    if (!(isfinite(t.x) && isfinite(t.y) && isfinite(t.z))) return;
    const int pos = atomicAdd(&cursor[cell_of(blk->g, t)], 1);             // the order inside a cell is arbitrary: the search takes a minimum
    if (pos >= 0 && pos < n) sorted[pos] = make_float4(t.x, t.y, t.z, __int_as_float(i));
}

// the points of cells [x0, x1] of one grid row against p: the minimum of (d2, original index)
__device__ __forceinline__ void grid_visit(const float4 p, const float4* __restrict__ sorted, int a, int b, float& bd, int& bi)
{
    for (int k = a; k < b; k++) {
        const float4 t = sorted[k];
        const float dx = p.x - t.x, dy = p.y - t.y, dz = p.z - t.z;
        const float d = (dx * dx + dy * dy) + dz * dz;
        const int idx = __float_as_int(t.w);
        if (d < bd || (d == bd && idx < bi)) { bd = d; bi = idx; }
    }
}

// A lower bound on the fp32 d2 of every target outside the cube of cells [q - r, q + r], or "none is outside" (returns true
// with *all_in set). A target in a cell with index >= k along an axis has x - lo >= k * cell * (1 - kFaceSlack), one in a cell
// with index < k has x - lo < k * cell * (1 + kFaceSlack); both sides are measured from the grid origin in
// fp64, 1e-12 of their size is taken off for the fp64 roundings, and a gap below 1e-15 m counts as none (its square would be
// subnormal in fp32).
__device__ __forceinline__ bool grid_settled(const IcpGrid& g, const float4 p, const int q[3], int r, float bd, int bi)
{
    const float pc[3] = { p.x, p.y, p.z };
    double bound = DBL_MAX;
    bool all_in = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double off = (double)pc[a] - (double)g.lo[a];
        const int hk = q[a] + r + 1, lk = q[a] - r;
        if (hk <= g.n[a] - 1) {
            all_in = false;
            const double face = (double)hk * (double)g.cell;
            double gap = face * (1.0 - kFaceSlack) - off;
            gap -= 1e-12 * (fabs(off) + face);
            if (!(gap >= 1e-15)) gap = 0.0;
            bound = fmin(bound, gap * gap);
        }
        if (lk >= 1) {
            all_in = false;
            const double face = (double)lk * (double)g.cell;
            double gap = off - face * (1.0 + kFaceSlack);
            gap -= 1e-12 * (fabs(off) + face);
            if (!(gap >= 1e-15)) gap = 0.0;
            bound = fmin(bound, gap * gap);
        }
    }
    if (all_in) return true;
    return bi >= 0 && (double)bd < bound * (1.0 - kBoundSlack);
}

// exact 1-NN through the grid: one lane per source point. First the 3 x 3 x 3 cells around the (clamped) cell of the point, their
// nine row ranges fetched before any point is read; then shells of growing Chebyshev radius up to shell_cap. A point that is not
// settled by then, or lies more than shell_cap cells outside the box, goes to the fallback list.
template <class V>
__global__ __launch_bounds__(kGridThreads) void k_icp_nn_grid(V S, int shell_cap, int phase)
{
    const auto v = S.view(blockIdx.z);
    IcpDevBlock* blk = v.blk();
    if (done_guard(blk, phase)) return;
    const int n_src = v.n_src();
    const int i = blockIdx.x * kGridThreads + threadIdx.x;
    if (i >= n_src) return;
    const int* __restrict__ cstart = v.gstart();
    const int* __restrict__ cend = v.gend();
    const float4* __restrict__ sorted = v.gsorted();
    unsigned long long* __restrict__ best = v.best();
    int* __restrict__ list = v.list();
    const float4 p = v.cur()[i];
    const IcpGrid g = blk->g;
    if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) || g.n_fin == 0) { best[i] = kNoMatch; return; }
    const float f[3] = { cell_coord(p.x, g.lo[0], g.inv), cell_coord(p.y, g.lo[1], g.inv), cell_coord(p.z, g.lo[2], g.inv) };
    const float reach = (float)shell_cap;
    bool settled = false;
    float bd = INFINITY;
    int bi = -1;
    bool near_box = g.usable != 0;
#pragma unroll
    for (int a = 0; a < 3; a++) near_box = near_box && (f[a] >= -reach) && (f[a] <= (float)g.n[a] + reach);
    if (near_box) {
        int q[3];
#pragma unroll
        for (int a = 0; a < 3; a++) q[a] = (int)fminf(fmaxf(floorf(f[a]), 0.0f), (float)(g.n[a] - 1));
        const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
        {
            const int x0 = max(q[0] - 1, 0), x1 = min(q[0] + 1, nx - 1);
            int ra[9], rb[9];
#pragma unroll
            for (int j = 0; j < 9; j++) {
                const int y = q[1] + (j % 3) - 1, z = q[2] + (j / 3) - 1;
                const bool in = y >= 0 && y < ny && z >= 0 && z < nz;
                const int row = in ? (z * ny + y) * nx : 0;
                ra[j] = in ? cstart[row + x0] : 0;
                rb[j] = in ? cend[row + x1] : 0;
            }
#pragma unroll
            for (int j = 0; j < 9; j++) grid_visit(p, sorted, ra[j], rb[j], bd, bi);
            settled = grid_settled(g, p, q, 1, bd, bi);
        }
        for (int r = 2; !settled && r <= shell_cap; r++) {
            const int xl = q[0] - r, xh = q[0] + r;
            const int x0 = max(xl, 0), x1 = min(xh, nx - 1);
            for (int dz = -r; dz <= r; dz++) {
                const int z = q[2] + dz;
                if (z < 0 || z >= nz) continue;
                for (int dy = -r; dy <= r; dy++) {
                    const int y = q[1] + dy;
                    if (y < 0 || y >= ny) continue;
                    const int row = (z * ny + y) * nx;
                    if (max(abs(dy), abs(dz)) == r) {
                        grid_visit(p, sorted, cstart[row + x0], cend[row + x1], bd, bi);
                    } else {
                        if (xl >= 0) grid_visit(p, sorted, cstart[row + xl], cend[row + xl], bd, bi);
                        if (xh < nx) grid_visit(p, sorted, cstart[row + xh], cend[row + xh], bd, bi);
                    }
                }
            }
            settled = grid_settled(g, p, q, r, bd, bi);
        }
    }
    if (settled) {
        best[i] = bi >= 0 ? (((unsigned long long)__float_as_uint(bd) << 32) | (unsigned)bi) : kNoMatch;
    } else {
        best[i] = kNoMatch;
        const int k = atomicAdd(&blk->wl_count, 1);
        if (k < n_src) list[k] = i;
    }
}

template <class V>
__global__ __launch_bounds__(256) void k_icp_reset_dev(V S, int phase)
{
    const auto v = S.view(blockIdx.z);
    if (done_guard(v.blk(), phase)) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < v.n_src()) v.best()[i] = kNoMatch;
}

// the brute force of the device loop: 256 sources - those a slot's list names, or with use_list == 0 all of them (the search with
// the grid off: k_icp_nn with a slot) - against target points [slice * len, (slice + 1) * len), the winner settled across slices by
// atomicMin. Grid (source blocks, target slices of the slot with most, slots); workgroups past the end of the list or of their
// slot's slices return at entry
template <class V>
__global__ __launch_bounds__(kNnThreads) void k_icp_nn_list(V S, int use_list, int phase)
{
    __shared__ float4 tile[kNnTile];
    const auto v = S.view(blockIdx.z);
    const IcpDevBlock* blk = v.blk();
    if (done_guard(blk, phase)) return;
    const int n_src = v.n_src(), n_tgt = v.n_tgt(), slice_len = v.slice_len();
    const int j0 = blockIdx.y * slice_len, j1 = min(j0 + slice_len, n_tgt);
    if (j0 >= n_tgt) return;
    const int* __restrict__ list = use_list ? v.list() : nullptr;
    const int count = list ? min(blk->wl_count, n_src) : n_src;
    if ((int)(blockIdx.x * kNnThreads) >= count) return;
    const float4* __restrict__ cur = v.cur();
    unsigned long long* __restrict__ best = v.best();
    const int w = blockIdx.x * kNnThreads + threadIdx.x;
    const bool valid = w < count;
    const int i = valid ? (list ? list[w] : w) : 0;
    const float4 p = valid ? cur[i] : make_float4(0, 0, 0, 0);
    const bool fin = valid && isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    float bd = INFINITY;
    int bi = -1;
    nn_tiles(p, fin, v.tgt(), j0, j1, tile, bd, bi);
    if (fin && bi >= 0)
        atomicMin(&best[i], ((unsigned long long)__float_as_uint(bd) << 32) | (unsigned)bi);
}

// count, sum d2, centroids and raw cross moments of the correspondences with d2 <= max_d2 (fp64): this workgroup's row of `part`
// (a function of its own for the __restrict__ of its parameters, which a kernel's locals would not carry). The stride is the threads
// of all rows of this alignment: the launch's where every slot has the launch's rows, own_rows * 256 in the table form (kOwnRows:
// a grid sized by a larger pair must not change which points a row sums)
template <bool kOwnRows>
__device__ __forceinline__ void sums_body(const float4* __restrict__ cur, int n_src, const float4* __restrict__ tgt,
                                          const unsigned long long* __restrict__ best, double max_d2, double* __restrict__ part,
                                          double (*sh)[17], const int own_rows)
{
    double a[17];
#pragma unroll
    for (int k = 0; k < 17; k++) a[k] = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_src; i += (kOwnRows ? own_rows : gridDim.x) * blockDim.x) {
        const unsigned long long key = best[i];
        if (key == kNoMatch) continue;
        const float d2 = __uint_as_float((unsigned)(key >> 32));
        if (!((double)d2 <= max_d2)) continue;                       // determineCorrespondences: distance[0] > max_dist_sqr -> skip
        const float4 s = cur[i], t = tgt[(unsigned)key];
        a[0] += 1.0; a[1] += (double)d2;
        a[2] += s.x; a[3] += s.y; a[4] += s.z; a[5] += t.x; a[6] += t.y; a[7] += t.z;
        a[8]  += (double)t.x * s.x; a[9]  += (double)t.x * s.y; a[10] += (double)t.x * s.z;
        a[11] += (double)t.y * s.x; a[12] += (double)t.y * s.y; a[13] += (double)t.y * s.z;
        a[14] += (double)t.z * s.x; a[15] += (double)t.z * s.y; a[16] += (double)t.z * s.z;
    }
#pragma unroll
    for (int k = 0; k < 17; k++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a[k] += __shfl_down(a[k], off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 17; k++) sh[wave][k] = a[k];
    }
    __syncthreads();
    if (threadIdx.x < 17) part[17 * blockIdx.x + threadIdx.x] = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
}

template <class V>
__global__ __launch_bounds__(256) void k_icp_sums_dev(V S, double max_d2, int phase)
{
    __shared__ double sh[4][17];
    const auto v = S.view(blockIdx.z);
    if (done_guard(v.blk(), phase)) return;
    if constexpr (V::kPerPair) {
        if ((int)blockIdx.x >= v.rows()) return;
    }
    sums_body<V::kPerPair>(v.cur(), v.n_src(), v.tgt(), v.best(), max_d2, v.part(), sh, v.rows());
}

// the rows of k_icp_sums_dev folded in workgroup order into the slot's block, and the fallback list closed. The host loop
// (icp_align) runs this kernel too and has no list: it never runs beside a flight, so the two counts it rewrites are nobody's.
template <class V>
__global__ __launch_bounds__(64) void k_icp_fold_dev(V S, int rows, int phase)
{
    const auto v = S.view(blockIdx.z);
    IcpDevBlock* blk = v.blk();
    if (done_guard(blk, phase)) return;
    if constexpr (V::kPerPair) rows = v.rows();                              // (the launch names the most of any pair)
    const int k = threadIdx.x;
    if (k < 17) {
        const double* __restrict__ part = v.part();
        double a = 0.0;
        for (int b = 0; b < rows; b++) a += part[17 * b + k];
        blk->sums[k] = a;
    }
    if (k == 0) { blk->n_fallback = blk->wl_count; blk->wl_count = 0; }
}

// closes the iteration on the folded sums: one lane per slot runs icp_close_step, the host loop's own source
template <class V>
__global__ __launch_bounds__(64) void k_icp_close(V S, IcpCloseParams prm)
{
    IcpDevBlock* blk = S.view(blockIdx.z).blk();
    if (threadIdx.x != 0 || blk->st.done) return;
    double sums[17];
    for (int k = 0; k < 17; k++) sums[k] = blk->sums[k];
    IcpLoopState st = blk->st;
    icp_close_step(sums, prm, &st);
    blk->st = st;
}

// phase 0: the source moves by the step of the iteration just closed (not once the alignment has ended); phase 1: the reloaded
// source moves by the final transformation
template <class V>
__global__ __launch_bounds__(256) void k_icp_transform_dev(V S, int phase)
{
    const auto v = S.view(blockIdx.z);
    const IcpDevBlock* blk = v.blk();
    if (done_guard(blk, phase)) return;
    transform_body(v.cur(), v.n_src(), phase == 0 ? blk->st.T_step : blk->st.T);
}

}  // namespace

struct IcpWorkspace {
    Buf cur, tgt, best, part;
    double* h_sums = nullptr;            // pinned, 17 doubles: slot 0's folded sums, what the host loop closes an iteration on
    // the device loop: its block with a pinned mirror, the grid (cell counts, starts, ends, the targets sorted by cell), the
    // fallback list, the event behind the work queued last, and what the host keeps about the alignment in flight
    Buf blk, gcount, gstart, gend, gsorted, list;
    IcpDevBlock* h_blk = nullptr;        // pinned, h_blk_n blocks: kIcpMaxSlots, kIcpMaxPairs from the first pair table on
    int h_blk_n = 0;
    // the pair table: its device copy and the pinned host array it is written in (kIcpMaxPairs views). Both, and the larger
    // block arrays, come with the first table (pairs_room): a handle that never aligns pairs allocates what it always did
    Buf tab;
    IcpView* h_tab = nullptr;
    hipEvent_t ev = nullptr;
    struct Flight {
        int phase = 0;                   // 0 none, 1 a range of iterations is queued, 2 the fitness pass is queued
        int queued = 0;
        IcpParams prm{};
        IcpTuning tune{};
    } fl;
    // The set the buffers are laid out for (dev_layout): its form, the stride of its records and a view per alignment - the
    // table's in h_tab, the slots' in slot_view, with the records each is loaded from (the fitness pass loads the sources again).
    IcpForm form = IcpForm::kSlots;
    size_t stride = 0;
    IcpView slot_view[kIcpMaxSlots]{};
    // what the kernels of the loop take: the slots by value with their guesses, made from the views, or the table's address
    IcpSlots S{};
    IcpGuesses G{};
    IcpPairs P{};
    // what the launches are sized by: the alignments, and the most of any of them (the slots share n_src and its rows)
    int K = 0, n_tgt_max = 0, slices_max = 0, n_src_max = 0, rows_max = 0;
};

IcpWorkspace* icp_create()
{
    IcpWorkspace* w = new (std::nothrow) IcpWorkspace();
    if (!w) return nullptr;
    w->h_blk_n = kIcpMaxSlots;
    if (hipHostMalloc((void**)&w->h_sums, sizeof(double) * 17) != hipSuccess ||
        w->blk.ensure(sizeof(IcpDevBlock) * kIcpMaxSlots) != hipSuccess ||
        hipHostMalloc((void**)&w->h_blk, sizeof(IcpDevBlock) * kIcpMaxSlots) != hipSuccess ||
        hipEventCreateWithFlags(&w->ev, hipEventDisableTiming) != hipSuccess) {
        icp_destroy(w);
        return nullptr;
    }
    return w;
}

void icp_destroy(IcpWorkspace* w)
{
    if (!w) return;
    Buf* bufs[] = { &w->cur, &w->tgt, &w->best, &w->part, &w->blk, &w->gcount, &w->gstart, &w->gend, &w->gsorted, &w->list, &w->tab };
    for (Buf* b : bufs) if (b->p) (void)hipFree(b->p);
    if (w->h_sums) (void)hipHostFree(w->h_sums);
    if (w->h_blk) (void)hipHostFree(w->h_blk);
    if (w->h_tab) (void)hipHostFree(w->h_tab);
    if (w->ev) (void)hipEventDestroy(w->ev);
    delete w;
}

#define ICP_TRY(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return e__; } while (0)

namespace {

bool guess_is_identity(const float* g)
{
    for (int i = 0; i < 16; i++) if (g[i] != ((i % 5 == 0) ? 1.0f : 0.0f)) return false;
    return true;
}

// what only the table form needs, once: blocks and their pinned mirror for kIcpMaxPairs, the table and its pinned image
// (nothing is in flight: the old blocks hold nothing that is still wanted)
hipError_t pairs_room(IcpWorkspace* w)
{
    ICP_TRY(w->blk.ensure(sizeof(IcpDevBlock) * kIcpMaxPairs));
    if (w->h_blk_n < kIcpMaxPairs) {
        IcpDevBlock* q = nullptr;
        ICP_TRY(hipHostMalloc((void**)&q, sizeof(IcpDevBlock) * kIcpMaxPairs));
        if (w->h_blk) (void)hipHostFree(w->h_blk);
        w->h_blk = q; w->h_blk_n = kIcpMaxPairs;
    }
    ICP_TRY(w->tab.ensure(sizeof(IcpView) * kIcpMaxPairs));
    if (!w->h_tab) ICP_TRY(hipHostMalloc((void**)&w->h_tab, sizeof(IcpView) * kIcpMaxPairs));
    return hipSuccess;
}

IcpView* views(IcpWorkspace* w) { return w->form == IcpForm::kTable ? w->h_tab : w->slot_view; }

// The buffers of a set and its views: the buffers are one set for both forms, an alignment's stretch of each starting where the
// one before ends (icp_layout: cur, best, list by sources; tgt, gsorted by targets; part by rows), the blocks and the cell arrays
// one per alignment; alignment 0 starts every buffer. An alignment's rows and slices are those of the single alignment of its
// sizes. A guess that is null or the identity leaves its alignment without one (`guess != Identity`, as PCL tests it), so that it
// runs what it ran before there were guesses. The slots and their guesses are then filled from the views; the table is the views
// themselves, in h_tab, and still has to be uploaded (dev_set_up). The host loop (icp_align) runs on the one-slot layout.
// tune: the device loop's list and, with the grid on, its cell arrays are laid out too (nullptr: the host loop, which has neither).
hipError_t dev_layout(IcpWorkspace* w, const IcpSet& a, const IcpTuning* tune)
{
    const bool table = a.form == IcpForm::kTable;
    IcpLayout L;
    if (!icp_layout(a.n, !table, a.n_src, a.n_tgt, &L)) return hipErrorInvalidValue;
    if (table) ICP_TRY(pairs_room(w));
    const size_t K = (size_t)a.n;
    ICP_TRY(w->cur.ensure(sizeof(float4) * L.tot_src)); ICP_TRY(w->tgt.ensure(sizeof(float4) * L.tot_tgt));
    ICP_TRY(w->best.ensure(sizeof(unsigned long long) * L.tot_src));
    ICP_TRY(w->part.ensure(sizeof(double) * 17 * L.tot_rows));
    const bool grid = tune && tune->use_grid;
    if (tune) ICP_TRY(w->list.ensure(sizeof(int) * L.tot_src));
    if (grid) {
        ICP_TRY(w->gcount.ensure(sizeof(int) * kGridMaxCells * K)); ICP_TRY(w->gstart.ensure(sizeof(int) * kGridMaxCells * K));
        ICP_TRY(w->gend.ensure(sizeof(int) * kGridMaxCells * K)); ICP_TRY(w->gsorted.ensure(sizeof(float4) * L.tot_tgt));
    }
    w->form = a.form; w->stride = a.stride;
    IcpView* view = views(w);
    for (int k = 0; k < a.n; k++) {
        const IcpLayoutItem& at = L.at[k];
        IcpView v{};
        v.cur = w->cur.as<float4>() + at.src_off; v.tgt = w->tgt.as<float4>() + at.tgt_off;
        v.best = w->best.as<unsigned long long>() + at.src_off; v.part = w->part.as<double>() + 17 * at.row_off;
        v.list = tune ? w->list.as<int>() + at.src_off : nullptr;
        v.gsorted = grid ? w->gsorted.as<float4>() + at.tgt_off : nullptr;
        v.blk = w->blk.as<IcpDevBlock>() + k;
        v.gcount = grid ? w->gcount.as<int>() + (size_t)k * kGridMaxCells : nullptr;
        v.gstart = grid ? w->gstart.as<int>() + (size_t)k * kGridMaxCells : nullptr;
        v.gend = grid ? w->gend.as<int>() + (size_t)k * kGridMaxCells : nullptr;
        v.d_src = a.d_src ? a.d_src[table ? k : 0] : nullptr; v.d_tgt = a.d_tgt[k];
        v.n_src = at.n_src; v.n_tgt = at.n_tgt; v.rows = at.rows; v.slice_len = at.slice_len;
        if (a.guess && a.guess[k] && !guess_is_identity(a.guess[k])) { v.guess_set = 1; memcpy(v.guess, a.guess[k], sizeof(v.guess)); }
        view[k] = v;
    }
    if (table) {
        w->P = IcpPairs{ w->tab.as<IcpView>() };
    } else {
        IcpSlots S{};
        IcpGuesses G{};
        for (int k = 0; k < a.n; k++) {
            const IcpView& v = view[k];
            S.cur[k] = v.cur; S.tgt[k] = v.tgt; S.best[k] = v.best; S.part[k] = v.part; S.list[k] = v.list; S.gsorted[k] = v.gsorted;
            S.n_tgt[k] = v.n_tgt; S.slice_len[k] = v.slice_len;
            if (v.guess_set) { G.set[k] = 1; memcpy(G.T[k], v.guess, sizeof(G.T[k])); }
        }
        S.blk = w->blk.as<IcpDevBlock>();
        S.gcount = w->gcount.as<int>(); S.gstart = w->gstart.as<int>(); S.gend = w->gend.as<int>();
        S.n_src = L.n_src_max;
        w->S = S; w->G = G;
    }
    w->K = a.n; w->n_tgt_max = L.n_tgt_max; w->slices_max = L.slices_max; w->n_src_max = L.n_src_max; w->rows_max = L.rows_max;
    return hipSuccess;
}

// The one dispatch from the layout's form to what its kernels take: the slots by value with their guesses, or the table's
// address, whose guesses are in the views. f: a generic lambda (S, G); a kernel is instantiated for the type of S it is given.
template <class F>
hipError_t with_form(IcpWorkspace* w, F&& f)
{
    return w->form == IcpForm::kTable ? f(w->P, IcpPairGuesses{ 0 }) : f(w->S, w->G);
}

// records -> float4 for every alignment of the layout. what (IcpPairLoad's codes): the targets, the sources as they are (the
// fitness pass) or the sources moved by their guesses, each slot's into its own moving copy
enum { kLoadTargets = 0, kLoadSources = 1, kLoadSourcesMoved = 2 };
hipError_t load(IcpWorkspace* w, hipStream_t stream, int what)
{
    const int most = what == kLoadTargets ? w->n_tgt_max : w->n_src_max;
    const dim3 grid((most + 255) / 256, 1, w->K);
    if (w->form == IcpForm::kTable) {
        hipLaunchKernelGGL(k_icp_load_slots<IcpPairLoad>, grid, dim3(256), 0, stream, IcpPairLoad{ w->P.t, what }, w->stride);
        return hipGetLastError();
    }
    IcpLoad L{};
    for (int k = 0; k < w->K; k++) {
        const IcpView& v = w->slot_view[k];
        L.src[k] = what == kLoadTargets ? v.d_tgt : v.d_src;
        L.dst[k] = what == kLoadTargets ? const_cast<float4*>(v.tgt) : v.cur;
        L.n[k] = what == kLoadTargets ? v.n_tgt : v.n_src;
        if (what == kLoadSourcesMoved && v.guess_set) { L.move[k] = 1; memcpy(L.m[k], v.guess, sizeof(L.m[k])); }
    }
    hipLaunchKernelGGL(k_icp_load_slots<IcpLoad>, grid, dim3(256), 0, stream, L, w->stride);
    return hipGetLastError();
}

// the block reset of every alignment of the layout and, with the grid on: box, shape, counts, scan, scatter - once per set
hipError_t dev_prepare(IcpWorkspace* w, hipStream_t stream, const IcpTuning& tune)
{
    return with_form(w, [&](const auto& S, const auto& G) -> hipError_t {
        using V = std::decay_t<decltype(S)>;
        using GV = std::decay_t<decltype(G)>;
        const unsigned K = (unsigned)w->K;
        hipLaunchKernelGGL((k_icp_begin<V, GV>), dim3(1, 1, K), dim3(64), 0, stream, S, G);
        if (tune.use_grid) {
            ICP_TRY(hipMemsetAsync(w->gcount.p, 0, sizeof(int) * kGridMaxCells * (size_t)K, stream));
            const int tb = (w->n_tgt_max + 255) / 256;
            hipLaunchKernelGGL(k_icp_grid_bbox<V>, dim3(std::min(tb, 256), 1, K), dim3(256), 0, stream, S);
            hipLaunchKernelGGL(k_icp_grid_setup<V>, dim3(1, 1, K), dim3(64), 0, stream, S, tune.cell);
            hipLaunchKernelGGL(k_icp_grid_count<V>, dim3(tb, 1, K), dim3(256), 0, stream, S);
            hipLaunchKernelGGL(k_icp_grid_scan<V>, dim3(1, 1, K), dim3(1024), 0, stream, S);
            hipLaunchKernelGGL(k_icp_grid_scatter<V>, dim3(tb, 1, K), dim3(256), 0, stream, S);
        }
        return hipGetLastError();
    });
}

// one search of the device loop in every alignment: the grid with its fallback, or (use_grid off) the brute force over every source
hipError_t dev_nearest(IcpWorkspace* w, hipStream_t stream, const IcpTuning& tune, int phase)
{
    return with_form(w, [&](const auto& S, const auto&) -> hipError_t {
        using V = std::decay_t<decltype(S)>;
        const unsigned K = (unsigned)w->K;
        const int n_src = w->n_src_max, sb = (n_src + kNnThreads - 1) / kNnThreads;
        if (tune.use_grid) {
            hipLaunchKernelGGL(k_icp_nn_grid<V>, dim3((n_src + kGridThreads - 1) / kGridThreads, 1, K), dim3(kGridThreads), 0, stream, S,
                               std::max(1, tune.shell_cap), phase);
            hipLaunchKernelGGL(k_icp_nn_list<V>, dim3(sb, w->slices_max, K), dim3(kNnThreads), 0, stream, S, 1, phase);
        } else {
            hipLaunchKernelGGL(k_icp_reset_dev<V>, dim3((n_src + 255) / 256, 1, K), dim3(256), 0, stream, S, phase);
            hipLaunchKernelGGL(k_icp_nn_list<V>, dim3(sb, w->slices_max, K), dim3(kNnThreads), 0, stream, S, 0, phase);
        }
        return hipGetLastError();
    });
}

hipError_t dev_sums(IcpWorkspace* w, hipStream_t stream, double max_d2, int phase)
{
    return with_form(w, [&](const auto& S, const auto&) -> hipError_t {
        using V = std::decay_t<decltype(S)>;
        const int rows = w->rows_max;
        hipLaunchKernelGGL(k_icp_sums_dev<V>, dim3(rows, 1, w->K), dim3(256), 0, stream, S, max_d2, phase);
        hipLaunchKernelGGL(k_icp_fold_dev<V>, dim3(1, 1, w->K), dim3(64), 0, stream, S, rows, phase);
        return hipGetLastError();
    });
}

// Everything of a set up to and including the preparation: the layout with its guesses, the table's upload, the sources moved by
// their guesses, the targets, the blocks and the grids. Every cloud of the set holds a point.
hipError_t dev_set_up(IcpWorkspace* w, hipStream_t stream, const IcpSet& a, const IcpTuning& tune)
{
    const bool table = a.form == IcpForm::kTable;
    if (a.n < 1 || a.n > kIcpMaxPairs) return hipErrorInvalidValue;
    for (int k = 0; k < a.n; k++) if (a.n_src[table ? k : 0] == 0 || a.n_tgt[k] == 0) return hipErrorInvalidValue;
    ICP_TRY(dev_layout(w, a, &tune));
    if (table) ICP_TRY(hipMemcpyAsync(w->tab.p, w->h_tab, sizeof(IcpView) * (size_t)w->K, hipMemcpyHostToDevice, stream));
    ICP_TRY(load(w, stream, kLoadSourcesMoved));
    ICP_TRY(load(w, stream, kLoadTargets));
    return dev_prepare(w, stream, tune);
}

// What the host loop (icp_align) asks per iteration, on the one-slot layout: the brute-force search, then the sums with slot 0's
// folded sums brought to h_sums and one wait. phase 1: the host closes the iteration, so no kernel looks at the block's `done`.
hipError_t host_nearest(IcpWorkspace* w, hipStream_t stream)
{
    const IcpSlots& S = w->S;
    hipLaunchKernelGGL(k_icp_reset_dev<IcpSlots>, dim3((S.n_src + 255) / 256), dim3(256), 0, stream, S, 1);
    hipLaunchKernelGGL(k_icp_nn, dim3((S.n_src + kNnThreads - 1) / kNnThreads, w->slices_max), dim3(kNnThreads), 0, stream,
                       (const float4*)S.cur[0], S.n_src, S.tgt[0], S.n_tgt[0], S.slice_len[0], S.best[0]);
    return hipGetLastError();
}

hipError_t host_sums(IcpWorkspace* w, hipStream_t stream, double max_d2)
{
    ICP_TRY(host_nearest(w, stream));
    ICP_TRY(dev_sums(w, stream, max_d2, 1));
    ICP_TRY(hipMemcpyAsync(w->h_sums, w->S.blk->sums, sizeof(double) * 17, hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

// the blocks of all alignments to the host in one copy, and the event the host tests: the end of everything queued so far
hipError_t dev_mark(IcpWorkspace* w, hipStream_t stream)
{
    ICP_TRY(hipMemcpyAsync(w->h_blk, w->blk.p, sizeof(IcpDevBlock) * (size_t)w->K, hipMemcpyDeviceToHost, stream));
    return hipEventRecord(w->ev, stream);
}

hipError_t dev_queue_range(IcpWorkspace* w, hipStream_t stream)
{
    IcpWorkspace::Flight& f = w->fl;
    const int n = std::min(kIcpRange, f.prm.max_iter - f.queued);
    const IcpCloseParams cp = icp_close_params(f.prm.max_iter, f.prm.trans_eps, f.prm.fit_eps);
    const double max_d2 = f.prm.max_corr_dist * f.prm.max_corr_dist;
    for (int k = 0; k < n; k++) {
        ICP_TRY(dev_nearest(w, stream, f.tune, 0));
        ICP_TRY(dev_sums(w, stream, max_d2, 0));
        ICP_TRY(with_form(w, [&](const auto& S, const auto&) -> hipError_t {
            using V = std::decay_t<decltype(S)>;
            hipLaunchKernelGGL(k_icp_close<V>, dim3(1, 1, w->K), dim3(64), 0, stream, S, cp);
            hipLaunchKernelGGL(k_icp_transform_dev<V>, dim3((w->n_src_max + 255) / 256, 1, w->K), dim3(256), 0, stream, S, 0);
            return hipGetLastError();
        }));
    }
    f.queued += n;
    return dev_mark(w, stream);
}

// getFitnessScore() of every alignment: the original source under its final transformation, nearest distances with no limit
hipError_t dev_queue_fitness(IcpWorkspace* w, hipStream_t stream)
{
    ICP_TRY(load(w, stream, kLoadSources));
    ICP_TRY(with_form(w, [&](const auto& S, const auto&) -> hipError_t {
        using V = std::decay_t<decltype(S)>;
        hipLaunchKernelGGL(k_icp_transform_dev<V>, dim3((w->n_src_max + 255) / 256, 1, w->K), dim3(256), 0, stream, S, 1);
        return hipSuccess;
    }));
    ICP_TRY(dev_nearest(w, stream, w->fl.tune, 1));
    ICP_TRY(dev_sums(w, stream, DBL_MAX, 1));
    return dev_mark(w, stream);
}

}  // namespace

void icp_dev_cancel(IcpWorkspace* w) { w->fl.phase = 0; }

hipError_t icp_dev_begin(IcpWorkspace* w, hipStream_t stream, const IcpSet& set, const IcpParams& prm, const IcpTuning& tune)
{
    if (w->fl.phase != 0 || prm.max_iter < 1) return hipErrorInvalidValue;
    ICP_TRY(dev_set_up(w, stream, set, tune));
    IcpWorkspace::Flight& f = w->fl;
    f = IcpWorkspace::Flight{};
    f.prm = prm; f.tune = tune;
    ICP_TRY(dev_queue_range(w, stream));
    f.phase = 1;
    return hipSuccess;
}

hipError_t icp_dev_advance(IcpWorkspace* w, hipStream_t stream, bool wait, bool* done, IcpResult* res, int res_cap)
{
    IcpWorkspace::Flight& f = w->fl;
    *done = false;
    if (f.phase == 0 || w->K > res_cap) return hipErrorInvalidValue;
    for (;;) {
        if (wait) {
            const hipError_t e = hipEventSynchronize(w->ev);
            if (e != hipSuccess) { f.phase = 0; return e; }
        } else {
            const hipError_t e = hipEventQuery(w->ev);
            if (e == hipErrorNotReady) { (void)hipGetLastError(); return hipSuccess; }
            if (e != hipSuccess) { f.phase = 0; return e; }
        }
        hipError_t e = hipSuccess;
        if (f.phase == 1) {
            bool all_done = true;
            for (int k = 0; k < w->K; k++) all_done = all_done && w->h_blk[k].st.done != 0;
            if (all_done) { e = dev_queue_fitness(w, stream); f.phase = 2; }
            else if (f.queued >= f.prm.max_iter) e = hipErrorUnknown;     // max_iter closes end every alignment: not reached
            else e = dev_queue_range(w, stream);
            if (e != hipSuccess) { f.phase = 0; return e; }
            if (!wait) return hipSuccess;
            continue;
        }
        for (int k = 0; k < w->K; k++) {
            const IcpDevBlock& b = w->h_blk[k];
            memcpy(res[k].T, b.st.T, sizeof(res[k].T));
            res[k].converged = b.st.conv; res[k].iterations = b.st.it;
            res[k].fitness = b.sums[0] > 0 ? b.sums[1] / b.sums[0] : DBL_MAX;
        }
        f.phase = 0;
        *done = true;
        return hipSuccess;
    }
}

hipError_t icp_dev_nearest(IcpWorkspace* w, hipStream_t stream, const unsigned char* d_src, size_t n_src_, const unsigned char* d_tgt,
                           size_t n_tgt_, size_t stride, int mode, const IcpTuning& tune, unsigned long long* keys, int* n_fallback,
                           int reps, float* us_build, float* us_search)
{
    const int n_src = (int)n_src_, n_tgt = (int)n_tgt_;
    if (w->fl.phase != 0 || n_src <= 0 || n_tgt <= 0) return hipErrorInvalidValue;
    const bool grid = mode != 0 && tune.use_grid != 0;
    ICP_TRY(dev_layout(w, IcpSet{ IcpForm::kSlots, 1, &d_src, &n_src_, &d_tgt, &n_tgt_, nullptr, stride }, mode != 0 ? &tune : nullptr));
    ICP_TRY(load(w, stream, kLoadSources));
    ICP_TRY(load(w, stream, kLoadTargets));
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
    const bool timed = reps > 0;
    hipError_t e = hipSuccess;
    if (timed) {
        e = hipEventCreate(&e0);
        if (e == hipSuccess) e = hipEventCreate(&e1);
        if (e == hipSuccess) e = hipEventCreate(&e2);
        if (e == hipSuccess) e = hipEventRecord(e0, stream);
    }
    if (e == hipSuccess && mode != 0) e = dev_prepare(w, stream, tune);
    if (e == hipSuccess && timed) e = hipEventRecord(e1, stream);
    for (int r = 0; e == hipSuccess && r < std::max(1, reps); r++) {
        if (mode != 0 && r > 0) hipLaunchKernelGGL(k_icp_fold_dev<IcpSlots>, dim3(1), dim3(64), 0, stream, w->S, 0, 1);   // (zeroes the list count)
        e = mode != 0 ? dev_nearest(w, stream, tune, 1) : host_nearest(w, stream);
    }
    if (e == hipSuccess && timed) e = hipEventRecord(e2, stream);
    if (e == hipSuccess && mode != 0) e = hipMemcpyAsync(w->h_blk, w->blk.p, sizeof(IcpDevBlock), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && keys) e = hipMemcpyAsync(keys, w->best.p, sizeof(unsigned long long) * n_src_, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess && timed) {
        float a = 0, b = 0;
        e = hipEventElapsedTime(&a, e0, e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&b, e1, e2);
        if (us_build) *us_build = a * 1000.0f;
        if (us_search) *us_search = b * 1000.0f / (float)reps;
    }
    for (hipEvent_t ev : { e0, e1, e2 }) if (ev) (void)hipEventDestroy(ev);
    if (n_fallback) *n_fallback = (grid && e == hipSuccess) ? w->h_blk->wl_count : 0;
    return e;
}

hipError_t icp_dev_grid(IcpWorkspace* w, hipStream_t stream, const unsigned char* const* d_tgt, const size_t* n_tgt, int n_slots, size_t stride,
                        const IcpTuning& tune, IcpGridInfo* info, int* const* cell_start, int* const* cell_end, int* const* order)
{
    static_assert(kIcpGridMaxCells == kGridMaxCells, "the hook's callers size their cell arrays by it");
    if (w->fl.phase != 0 || n_slots < 1 || n_slots > kIcpMaxSlots) return hipErrorInvalidValue;
    for (int k = 0; k < n_slots; k++) if (n_tgt[k] == 0) return hipErrorInvalidValue;
    IcpTuning t = tune;
    t.use_grid = 1;
    const size_t no_src = 0;                                              // (no source: nothing here reads a slot's source arrays)
    ICP_TRY(dev_layout(w, IcpSet{ IcpForm::kSlots, n_slots, nullptr, &no_src, d_tgt, n_tgt, nullptr, stride }, &t));
    ICP_TRY(load(w, stream, kLoadTargets));
    ICP_TRY(dev_prepare(w, stream, t));
    ICP_TRY(hipMemcpyAsync(w->h_blk, w->blk.p, sizeof(IcpDevBlock) * (size_t)n_slots, hipMemcpyDeviceToHost, stream));
    ICP_TRY(hipStreamSynchronize(stream));
    for (int k = 0; k < n_slots; k++) {
        const IcpGrid& g = w->h_blk[k].g;
        const IcpView& v = w->slot_view[k];
        IcpGridInfo& o = info[k];
        for (int a = 0; a < 3; a++) { o.lo[a] = g.lo[a]; o.n[a] = g.n[a]; }
        o.cell = g.cell; o.inv = g.inv; o.n_fin = g.n_fin; o.usable = g.usable;
        if (!g.usable) continue;
        const size_t ncells = (size_t)g.n[0] * (size_t)g.n[1] * (size_t)g.n[2];
        if (ncells > (size_t)kGridMaxCells || g.n_fin < 0 || (size_t)g.n_fin > n_tgt[k]) return hipErrorUnknown;   // not reached
        if (cell_start && cell_start[k]) ICP_TRY(hipMemcpyAsync(cell_start[k], v.gstart, sizeof(int) * ncells, hipMemcpyDeviceToHost, stream));
        if (cell_end && cell_end[k]) ICP_TRY(hipMemcpyAsync(cell_end[k], v.gend, sizeof(int) * ncells, hipMemcpyDeviceToHost, stream));
        if (order && order[k] && g.n_fin > 0)                             // the .w of every sorted entry: one int out of each float4
            ICP_TRY(hipMemcpy2DAsync(order[k], sizeof(int), reinterpret_cast<const unsigned char*>(v.gsorted) + 3 * sizeof(float),
                                     sizeof(float4), sizeof(int), (size_t)g.n_fin, hipMemcpyDeviceToHost, stream));
    }
    return hipStreamSynchronize(stream);
}

hipError_t icp_dev_close(IcpWorkspace* w, hipStream_t stream, int n, const double* sums, const IcpLoopState* in, const IcpParams& prm,
                         IcpLoopState* out)
{
    if (w->fl.phase != 0 || n < 1 || n > kIcpMaxPairs || prm.max_iter < 1) return hipErrorInvalidValue;
    ICP_TRY(pairs_room(w));
    for (int k = 0; k < n; k++) {                                         // a table of blocks: the close reads nothing else of a view
        IcpView v{};
        v.blk = w->blk.as<IcpDevBlock>() + k;
        w->h_tab[k] = v;
        IcpDevBlock b{};
        b.st = in[k];
        memcpy(b.sums, sums + 17 * (size_t)k, sizeof(b.sums));
        w->h_blk[k] = b;
    }
    w->form = IcpForm::kTable;
    w->P = IcpPairs{ w->tab.as<IcpView>() };
    w->K = n;
    ICP_TRY(hipMemcpyAsync(w->tab.p, w->h_tab, sizeof(IcpView) * (size_t)n, hipMemcpyHostToDevice, stream));
    ICP_TRY(hipMemcpyAsync(w->blk.p, w->h_blk, sizeof(IcpDevBlock) * (size_t)n, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_icp_close<IcpPairs>, dim3(1, 1, n), dim3(64), 0, stream, w->P, icp_close_params(prm.max_iter, prm.trans_eps, prm.fit_eps));
    ICP_TRY(hipGetLastError());
    ICP_TRY(hipMemcpyAsync(w->h_blk, w->blk.p, sizeof(IcpDevBlock) * (size_t)n, hipMemcpyDeviceToHost, stream));
    ICP_TRY(hipStreamSynchronize(stream));
    for (int k = 0; k < n; k++) out[k] = w->h_blk[k].st;
    return hipSuccess;
}

hipError_t icp_dev_sums(IcpWorkspace* w, hipStream_t stream, const IcpSet& set, double max_corr_dist, const IcpTuning& tune, double* sums,
                        int* n_rows, double* const* parts, unsigned long long* const* keys)
{
    if (w->fl.phase != 0) return hipErrorInvalidValue;
    ICP_TRY(dev_set_up(w, stream, set, tune));
    ICP_TRY(dev_nearest(w, stream, tune, 0));
    ICP_TRY(dev_sums(w, stream, max_corr_dist * max_corr_dist, 0));
    const int n = set.n;
    ICP_TRY(hipMemcpyAsync(w->h_blk, w->blk.p, sizeof(IcpDevBlock) * (size_t)n, hipMemcpyDeviceToHost, stream));
    for (int k = 0; k < n; k++) {
        const IcpView& v = views(w)[k];
        n_rows[k] = v.rows;
        if (parts && parts[k]) ICP_TRY(hipMemcpyAsync(parts[k], v.part, sizeof(double) * 17 * (size_t)v.rows, hipMemcpyDeviceToHost, stream));
        if (keys && keys[k]) ICP_TRY(hipMemcpyAsync(keys[k], v.best, sizeof(unsigned long long) * (size_t)v.n_src, hipMemcpyDeviceToHost, stream));
    }
    ICP_TRY(hipStreamSynchronize(stream));
    for (int k = 0; k < n; k++) memcpy(sums + 17 * (size_t)k, w->h_blk[k].sums, sizeof(double) * 17);
    return hipSuccess;
}

hipError_t icp_align(IcpWorkspace* w, hipStream_t stream, const unsigned char* d_src, size_t n_src_, const unsigned char* d_tgt,
                     size_t n_tgt_, size_t stride, const IcpParams& prm, IcpResult* res, const float* guess)
{
    const int n_src = (int)n_src_;
    *res = icp_result_none();
    if (n_src_ == 0 || n_tgt_ == 0) return hipSuccess;
    if (w->fl.phase != 0) return hipErrorInvalidValue;                    // (the layout is the flight's: the callers answer BUSY before)
    ICP_TRY(dev_layout(w, IcpSet{ IcpForm::kSlots, 1, &d_src, &n_src_, &d_tgt, &n_tgt_, &guess, stride }, nullptr));
    ICP_TRY(load(w, stream, kLoadSourcesMoved));
    ICP_TRY(load(w, stream, kLoadTargets));

    // icp.hpp computeTransformation + default_convergence_criteria.hpp hasConverged: icp_close_step, between two synchronisations
    const double max_d2 = prm.max_corr_dist * prm.max_corr_dist;
    const IcpCloseParams cp = icp_close_params(prm.max_iter, prm.trans_eps, prm.fit_eps);
    IcpLoopState st;
    icp_state_init(&st, w->G.set[0] ? w->G.T[0] : nullptr);       // final_transformation_ = guess
    for (;;) {
        ICP_TRY(host_sums(w, stream, max_d2));
        const int it_before = st.it;
        icp_close_step(w->h_sums, cp, &st);
        if (st.it != it_before) {                                         // (not on the `fewer than 3 correspondences` exit)
            Mat34 T34;
            memcpy(T34.m, st.T_step, sizeof(float) * 12);
            hipLaunchKernelGGL(k_icp_transform, dim3((n_src + 255) / 256), dim3(256), 0, stream, w->cur.as<float4>(), n_src, T34);
            ICP_TRY(hipGetLastError());
        }
        if (st.done) break;
    }
    memcpy(res->T, st.T, sizeof(res->T));
    const int conv = st.conv, it = st.it;
    // getFitnessScore(): the original source under the final transform, mean squared nearest distance
    ICP_TRY(load(w, stream, kLoadSources));
    Mat34 F34;
    memcpy(F34.m, res->T, sizeof(float) * 12);
    hipLaunchKernelGGL(k_icp_transform, dim3((n_src + 255) / 256), dim3(256), 0, stream, w->cur.as<float4>(), n_src, F34);
    ICP_TRY(host_sums(w, stream, DBL_MAX));
    res->fitness = w->h_sums[0] > 0 ? w->h_sums[1] / w->h_sums[0] : DBL_MAX;
    res->converged = conv; res->iterations = it;
    return hipSuccess;
}

}  // namespace s2m
