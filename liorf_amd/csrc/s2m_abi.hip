// s2m_abi.hip — host side of the gfx950 scan-to-map path and the part of the C ABI (include/liorf_s2m.h) that launches its
// kernels: create / destroy / params, the map index and the scan preparation, the LM loop and its graphs, batches and slots,
// the debug and timing entry points, ScanContext.  The only translation unit that includes s2m_kernels.hpp / s2m_register.hpp.
//
// Builds the map's uniform-grid index and the scan's locality order on the device (memory grow-only, sized by the actual
// point counts), and runs the whole <= max_iter LM loop as one captured hipGraph (enqueue_loop) so that a scan costs one graph
// launch and one synchronisation.  The handle is s2m_context.hpp's; the entry points that only orchestrate other units' stages
// live in s2m_abi_voxel.hip, s2m_abi_keyframes.hip, s2m_abi_loop.hip and s2m_abi_front_end.hip.  There is no CPU fallback:
// without a gfx950 device every entry point fails with S2M_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <limits>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "s2m_context.hpp"
#include "s2m_kernels.hpp"

using namespace s2m;
using namespace s2m::host;

namespace {

inline uint32_t host_f2ord(float f) { uint32_t u; memcpy(&u, &f, 4); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
inline float host_ord2f(uint32_t o) { uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o; float f; memcpy(&f, &u, 4); return f; }

// milliseconds between two device stamps of the pinned block (valid once the stream has been synchronised behind the kernels
// that wrote them)
inline float stamps_ms(const s2m_context* h, int from, int to)
{
    const unsigned long long a = h->reg.h_stamps[from], b = h->reg.h_stamps[to];
    return (b > a && h->reg.wall_clock_khz > 0) ? (float)((double)(b - a) / (double)h->reg.wall_clock_khz) : 0.0f;
}

// the partial rows of a launch (two slots, by launch parity) and, behind them, the search kernel's worklist
int ensure_rows(s2m_context* h, int nblocks)
{
    const size_t rows = sizeof(double) * 2 * kAcc * (size_t)nblocks;
    int rc = ensure(h, h->reg.partials, rows + 64 + sizeof(int32_t) * 2 * (size_t)nblocks);
    if (rc) return rc;
    h->hctx.partials = h->reg.partials.as<double>();
    h->hctx.wl_count = reinterpret_cast<int32_t*>(h->reg.partials.as<unsigned char>() + rows);
    h->hctx.wl_items = h->hctx.wl_count + 16;
    h->ctx_dirty = true;
    return S2M_OK;
}

int upload_ctx(s2m_context* h)
{
    if (!h->ctx_dirty) return S2M_OK;
    hipLaunchKernelGGL(k_set_ctx, dim3(1), dim3(64), 0, h->stream, h->reg.dctx.as<DevCtx>(), h->hctx);
    S2M_HIP(h, hipGetLastError());
    h->ctx_dirty = false;
    return S2M_OK;
}

// exclusive scan of counts[0..n) into out[0..n], out[n] = total
int device_exclusive_scan(s2m_context* h, const int32_t* counts, int32_t* out, int n, int total)
{
    const int nb = (n + 1023) / 1024;
    int rc = ensure(h, h->reg.block_sums, sizeof(int32_t) * (size_t)(nb + 1));
    if (rc) return rc;
    int32_t* sums = h->reg.block_sums.as<int32_t>();
    hipLaunchKernelGGL(k_scan_local, dim3(nb), dim3(256), 0, h->stream, counts, out, sums, n);
    if (nb <= 4096) hipLaunchKernelGGL(k_scan_add_fold, dim3(nb), dim3(256), 0, h->stream, out, (const int32_t*)sums, n, total);
    else {
        hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, h->stream, sums, nb);
        hipLaunchKernelGGL(k_scan_add, dim3(nb), dim3(256), 0, h->stream, out, (const int32_t*)sums, n, total);
    }
    S2M_HIP(h, hipGetLastError());
    return S2M_OK;
}

// bounding box of the finite points (device reduction + 24-byte readback)
int device_bbox(s2m_context* h, const unsigned char* d_pts, size_t stride, int n, float mn[3], float mx[3])
{
    const int blocks = std::min((n + 255) / 256, 1024);
    int rc = ensure(h, h->reg.mm, 64 + sizeof(uint32_t) * 8 * 1024);          // mm[0..5], then 8 words per workgroup from word 16 on
    if (rc) return rc;
    uint32_t* part = h->reg.mm.as<uint32_t>() + 16;
    hipLaunchKernelGGL(k_bbox, dim3(blocks), dim3(256), 0, h->stream, d_pts, stride, n, part);
    hipLaunchKernelGGL(k_bbox_fold, dim3(1), dim3(256), 0, h->stream, (const uint32_t*)part, blocks, h->reg.mm.as<uint32_t>());
    S2M_HIP(h, hipGetLastError());
    S2M_HIP(h, hipMemcpyAsync(h->reg.h_mm, h->reg.mm.p, 24, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    for (int d = 0; d < 3; d++) {
        if (h->reg.h_mm[d] == 0xffffffffu || h->reg.h_mm[3 + d] == 0u) { mn[d] = 0.0f; mx[d] = 0.0f; }   // no finite value
        else { mn[d] = host_ord2f(h->reg.h_mm[d]); mx[d] = host_ord2f(h->reg.h_mm[3 + d]); }
    }
    return S2M_OK;
}

int set_map_build(s2m_context* h, const void* pts, size_t n, size_t stride, bool on_device);

}  // namespace

// The index is rebuilt in place: once the rebuild has started the old index is gone, so a failure on the way leaves the handle
// with NO map (n_m = 0, the reference's "no key poses yet" state, :1297), a new map epoch (batch slots drop what they adopted)
// and no certificates - never the old point count over half-rewritten buffers.
int s2m::host::set_map_impl(s2m_context* h, const void* pts, size_t n, size_t stride, bool on_device)
{
    int rc = check_records(h, pts, n, stride);
    if (rc) return rc;
    rc = set_map_build(h, pts, n, stride, on_device);
    if (rc != S2M_OK && n > 0) {
        const std::string why = h->err;
        h->batch.map_epoch++;
        h->reg.n_m = 0; h->hctx.n_m = 0; h->ctx_dirty = true;
        if (h->reg.have_scan && h->reg.n_q > 0 && h->reg.cert.p) {
            (void)hipMemsetAsync(h->reg.cert.p, 0, sizeof(float4) * h->reg.n_q, h->stream);
            (void)hipMemsetAsync(h->reg.aux.p, 0, sizeof(int4) * h->reg.n_q, h->stream);
        }
        (void)upload_ctx(h);
        (void)hipStreamSynchronize(h->stream);
        h->err = why;
    }
    return rc;
}

namespace {

int set_map_build(s2m_context* h, const void* pts, size_t n, size_t stride, bool on_device)
{
    int rc;
    S2M_HIP(h, hipSetDevice(h->device));
    S2M_HIP(h, hipEventRecord(h->reg.ev_c, h->stream));
    if (n == 0) { h->batch.map_epoch++; h->reg.n_m = 0; h->hctx.n_m = 0; h->ctx_dirty = true; h->reg.t_set_map_ms = 0; return upload_ctx(h); }

    const unsigned char* d_pts;
    if (on_device) d_pts = static_cast<const unsigned char*>(pts);
    else {
        if ((rc = stage_host_records(h, h->reg.raw_map, pts, n * stride))) return rc;
        d_pts = h->reg.raw_map.as<unsigned char>();
    }
    float mn[3], mx[3];
    if ((rc = device_bbox(h, d_pts, stride, (int)n, mn, mx))) return rc;

    // cell edge: every map point with fp32 d2 < gate_sq of a query lies in the 3x3x3 block
    // around the query's cell once E >= sqrt(gate_sq) plus a margin that covers the fp32
    // rounding of (v - o) * inv_e (<= 2.4e-5 cells at |v - o| <= 200).
    // The edge is 2.5 % above the gate: a query's 3x3x3 cells then cover a ball of that much more than the gate around it,
    // which is what lets a point with fewer than 5 neighbours inside the gate prove "and none just outside it either" and
    // keep that verdict over the following launches (s2m_register.hpp, tier A) instead of searching again.
    double E = std::sqrt(h->prm.gate_sq) * 1.025;
    GridDesc g{};
    for (int attempt = 0; attempt < 32; attempt++) {
        const float Ef = (float)E;
        g.inv_e = 1.0f / Ef; g.e = Ef;
        g.ox = mn[0] - Ef; g.oy = mn[1] - Ef; g.oz = mn[2] - Ef;
        double nx = std::floor(((double)mx[0] - g.ox) * g.inv_e) + 2.0;
        double ny = std::floor(((double)mx[1] - g.oy) * g.inv_e) + 2.0;
        double nz = std::floor(((double)mx[2] - g.oz) * g.inv_e) + 2.0;
        if (nx * ny * nz <= (double)(1 << 27) && nx < 65536 && ny < 65536 && nz < 65536) {
            g.nx = (int)nx; g.ny = (int)ny; g.nz = (int)nz; g.ncells = g.nx * g.ny * g.nz;
            break;
        }
        E *= 2.0;     // coarser cells stay correct (only more candidates per query)
        g.ncells = 0;
    }
    if (g.ncells <= 0) return fail(h, S2M_ERR_CAPACITY, "map extent too large for the search grid");

    if ((rc = ensure(h, h->reg.map_sorted, sizeof(float4) * n))) return rc;
    if ((rc = ensure(h, h->reg.m_counts, sizeof(int32_t) * ((size_t)g.ncells + 1)))) return rc;
    if ((rc = ensure(h, h->reg.m_cell_start, sizeof(int32_t) * ((size_t)g.ncells + 1)))) return rc;
    if ((rc = ensure(h, h->reg.m_cell_of, sizeof(int32_t) * n))) return rc;
    if ((rc = ensure(h, h->reg.m_rank_of, sizeof(int32_t) * n))) return rc;

    S2M_HIP(h, hipMemsetAsync(h->reg.m_counts.p, 0, sizeof(int32_t) * ((size_t)g.ncells + 1), h->stream));
    const int nb = ((int)n + 255) / 256;
    hipLaunchKernelGGL(k_bin_count, dim3(nb), dim3(256), 0, h->stream, d_pts, stride, (int)n, g,
                       h->reg.m_cell_of.as<int32_t>(), h->reg.m_rank_of.as<int32_t>(), h->reg.m_counts.as<int32_t>());
    S2M_HIP(h, hipGetLastError());
    if ((rc = device_exclusive_scan(h, h->reg.m_counts.as<int32_t>(), h->reg.m_cell_start.as<int32_t>(), g.ncells, (int)n))) return rc;
    hipLaunchKernelGGL(k_scatter_map, dim3(nb), dim3(256), 0, h->stream, d_pts, stride, (int)n,
                       (const int32_t*)h->reg.m_cell_of.as<int32_t>(), (const int32_t*)h->reg.m_rank_of.as<int32_t>(),
                       (const int32_t*)h->reg.m_cell_start.as<int32_t>(), h->reg.map_sorted.as<float4>());
    S2M_HIP(h, hipGetLastError());

    if (h->reg.have_scan && h->reg.n_q > 0 && h->reg.cert.p) {           // tuples and certificates of the old map are meaningless now
        S2M_HIP(h, hipMemsetAsync(h->reg.cert.p, 0, sizeof(float4) * h->reg.n_q, h->stream));
        S2M_HIP(h, hipMemsetAsync(h->reg.aux.p, 0, sizeof(int4) * h->reg.n_q, h->stream));
    }
    h->batch.map_epoch++;
    h->reg.n_m = n;                                       // committed only now; a failure above leaves no map at all (set_map_impl)
    h->hctx.n_m = (int32_t)n;
    h->hctx.g = g;
    h->hctx.map_sorted = h->reg.map_sorted.as<float4>();
    h->hctx.cell_start = h->reg.m_cell_start.as<int32_t>();
    h->ctx_dirty = true;
    S2M_HIP(h, hipEventRecord(h->reg.ev_d, h->stream));
    if ((rc = upload_ctx(h))) return rc;
    S2M_HIP(h, hipStreamSynchronize(h->stream));     // the caller's buffer is free again
    S2M_HIP(h, hipEventElapsedTime(&h->reg.t_set_map_ms, h->reg.ev_c, h->reg.ev_d));
    return S2M_OK;
}

// s2m_set_scan in three steps, so that the scan slots of a batch share the launches of the middle one:
//   scan_slot_prepare   host side: sizes, buffers, the upload of a host source, the DevCtx fields - and the slot's row of the table
//   launch_scan_prep    the ordering kernels, one grid row per slot (blockIdx.y): six for the slots of a batch, four for a single
//                       scan (the cell scan inside the scatter; the wave table left to the scan's first optimisation)
//   scan_slot_finish    bookkeeping
int scan_slot_prepare(s2m_context* h, const void* pts, size_t n, size_t stride, bool on_device, PrepSlot* ps)
{
    int rc = check_records(h, pts, n, stride);
    if (rc) return rc;
    memset(ps, 0, sizeof(*ps));
    h->reg.n_q = n; h->reg.have_scan = true;
    h->hctx.n_q = (int32_t)n;
    // wave table capacity: every 64-point chunk plus a 50 % budget of extra waves for split chunks
    const int n_chunks = (int)((n + 63) / 64);
    constexpr int NW = kBlock / 64;
    // how finely to cut when the scan alone cannot fill the GPU (~2048 co-resident waves): 1, 2, 4 or 8
    int base_parts = 1;
    while (base_parts < 8 && n_chunks * base_parts * 2 <= 2048) base_parts *= 2;
    h->reg.base_parts = base_parts;
    int nblocks = (n_chunks * base_parts + n_chunks / 2 + NW - 1) / NW;
    nblocks = ((nblocks + kBlocksQuantum - 1) / kBlocksQuantum) * kBlocksQuantum;
    if (nblocks == 0) nblocks = kBlocksQuantum;
    const int table_cap = nblocks * NW;                   // wave-table entries: every chunk plus the budget for split chunks
    // more entries than one 8-wave workgroup per CU holds: 16-wave workgroups, one per CU (s2m_types.h, kBigWaves)
    const int wpb = (h->tune.big_blocks && n_chunks * base_parts > (kMaxBlocks / 2) * NW) ? kBigWaves : NW;
    // the grid stays co-resident - one workgroup per CU in either shape (the 8-wave shape of a single scan is built for 2 waves
    // per SIMD: 256 registers per lane, no scratch; the scan slots of a batch run the 128-register build, two per CU) - and waves
    // loop over the table
    nblocks = std::min((table_cap + wpb - 1) / wpb, (wpb == NW && h->batch.parent) ? kMaxBlocks : kMaxBlocks / 2);
    if (h->batch.parent && h->tune.batch_entries > 1) nblocks = std::max((nblocks + h->tune.batch_entries - 1) / h->tune.batch_entries, 1);   // a batch slot: several entries per wave
    h->hctx.wpb = wpb;
    h->hctx.nblocks = nblocks;
    h->hctx.table_cap = table_cap;
    h->ctx_dirty = true;
    if ((rc = ensure_rows(h, nblocks))) return rc;
    if (n == 0) return S2M_OK;

    const unsigned char* d_pts;
    if (on_device) d_pts = static_cast<const unsigned char*>(pts);
    else {
        if ((rc = stage_host_records(h, h->reg.raw_scan, pts, n * stride))) return rc;
        S2M_HIP(h, hipEventRecord(h->reg.ev_up, h->stream));   // waited for in scan_slot_finish: the caller's buffer is free when the call returns
        d_pts = h->reg.raw_scan.as<unsigned char>();
    }
    // locality order of the scan: log-polar Z-order bins (k_polar_count), no host round trip
    if ((rc = ensure(h, h->reg.qx, sizeof(float) * n))) return rc;
    if ((rc = ensure(h, h->reg.qy, sizeof(float) * n))) return rc;
    if ((rc = ensure(h, h->reg.qz, sizeof(float) * n))) return rc;
    if ((rc = ensure(h, h->reg.qperm, sizeof(int32_t) * n))) return rc;
    if ((rc = ensure(h, h->reg.npos, sizeof(int32_t) * 5 * n))) return rc;
    if ((rc = ensure(h, h->reg.plane_cache, sizeof(float4) * n))) return rc;
    if ((rc = ensure(h, h->reg.plane_alt, sizeof(float4) * n))) return rc;
    if ((rc = ensure(h, h->reg.npos_alt, sizeof(int32_t) * 5 * n))) return rc;
    if ((rc = ensure(h, h->reg.cert, sizeof(float4) * n))) return rc;           // cert and aux are reset by k_scatter_scan
    if ((rc = ensure(h, h->reg.aux, sizeof(int4) * n))) return rc;
    if ((rc = ensure(h, h->reg.front, sizeof(float4) * kNbrCap * n))) return rc;
    if ((rc = ensure(h, h->reg.q_cell_start, sizeof(int32_t) * kPolarCells))) return rc;
    if ((rc = ensure(h, h->reg.q_cell_of, sizeof(int32_t) * n))) return rc;
    if ((rc = ensure(h, h->reg.q_rank_of, sizeof(int32_t) * n))) return rc;
    const int npb = ((int)n + kPolarBlock - 1) / kPolarBlock;
    if ((rc = ensure(h, h->reg.q_block_hist, sizeof(int32_t) * (size_t)kPolarCells * (size_t)npb))) return rc;
    if ((rc = ensure(h, h->reg.chunk_parts, sizeof(int32_t) * (size_t)(n_chunks + 1)))) return rc;
    {   // density wishes: all zero between uses (k_chunk_table_density clears what it consumes)
        const void* before = h->reg.chunk_factor.p;
        if ((rc = ensure(h, h->reg.chunk_factor, sizeof(int32_t) * (size_t)(n_chunks + 1)))) return rc;
        if (h->reg.chunk_factor.p != before) S2M_HIP(h, hipMemsetAsync(h->reg.chunk_factor.p, 0, h->reg.chunk_factor.cap, h->stream));
    }
    if ((rc = ensure(h, h->reg.wave_table, sizeof(int2) * (size_t)table_cap))) return rc;
    if ((rc = ensure(h, h->reg.n_waves, 64))) return rc;

    ps->pts = d_pts; ps->stride = stride; ps->n = (int32_t)n; ps->n_chunks = n_chunks; ps->base_parts = base_parts;
    ps->capacity = table_cap; ps->npb = npb;
    ps->cell_of = h->reg.q_cell_of.as<int32_t>(); ps->rank_of = h->reg.q_rank_of.as<int32_t>(); ps->block_hist = h->reg.q_block_hist.as<int32_t>();
    ps->counts = h->reg.q_counts.as<int32_t>(); ps->cell_start = h->reg.q_cell_start.as<int32_t>();
    ps->qx = h->reg.qx.as<float>(); ps->qy = h->reg.qy.as<float>(); ps->qz = h->reg.qz.as<float>(); ps->qperm = h->reg.qperm.as<int32_t>();
    ps->cert = h->reg.cert.as<float4>(); ps->aux = h->reg.aux.as<int4>();
    ps->chunk_parts = h->reg.chunk_parts.as<int32_t>(); ps->wave_table = h->reg.wave_table.as<int2>(); ps->n_waves = h->reg.n_waves.as<int32_t>();
    ps->stamps = nullptr;                                 // (set_scan_impl: a single scan times its preparation)
    h->reg.prep_slot = *ps;

    h->hctx.qx = h->reg.qx.as<float>(); h->hctx.qy = h->reg.qy.as<float>(); h->hctx.qz = h->reg.qz.as<float>();
    h->hctx.qperm = h->reg.qperm.as<int32_t>();
    h->hctx.wave_table = h->reg.wave_table.as<int2>();
    h->hctx.n_waves = h->reg.n_waves.as<int32_t>();
    h->hctx.wave_table_rw = h->reg.wave_table.as<int2>();
    h->hctx.n_waves_rw = h->reg.n_waves.as<int32_t>();
    h->hctx.chunk_parts = h->reg.chunk_parts.as<int32_t>();
    h->hctx.chunk_factor = h->reg.chunk_factor.as<int32_t>();
    h->hctx.n_chunks = n_chunks;
    h->hctx.density_pending = 1;
    h->hctx.npos = h->reg.npos.as<int32_t>();
    h->hctx.cert = h->reg.cert.as<float4>();
    h->hctx.aux = h->reg.aux.as<int4>();
    h->hctx.front = h->reg.front.as<float4>();
    h->hctx.plane_cache = h->reg.plane_cache.as<float4>();
    h->hctx.plane_alt = h->reg.plane_alt.as<float4>();
    h->hctx.npos_alt = h->reg.npos_alt.as<int32_t>();
    h->ctx_dirty = true;
    return S2M_OK;
}

// the ordering kernels of `nslots` prepared slots (rows with n = 0 do nothing), on `stream`
// `single` (a scan of the handle's own, one slot): k_polar_count, k_polar_prefix, the scatter with the cell scan in it,
// k_chunk_parts - and no wave table: the scan's first optimisation asks for the density wishes chunk by chunk
// (k_wave_density_state) and k_chunk_table_density emits the table once; whatever else needs the extent-only table first
// builds it through ensure_wave_table.
void launch_scan_prep(hipStream_t stream, const PrepTable& t, int nslots, bool single = false)
{
    int npb = 0, nb = 0, ncb = 0;
    for (int k = 0; k < nslots; k++) {
        npb = std::max(npb, (int)t.s[k].npb);
        nb = std::max(nb, (t.s[k].n + 255) / 256);
        ncb = std::max(ncb, (t.s[k].n_chunks + 3) / 4);
    }
    if (npb == 0) return;
    hipLaunchKernelGGL(k_polar_count, dim3(npb, nslots), dim3(kPolarBlock), 0, stream, t);
    hipLaunchKernelGGL(k_polar_prefix, dim3(kPolarCells / 64, nslots), dim3(1024), 0, stream, t);
    if (single) {
        hipLaunchKernelGGL(k_scatter_scan_fold, dim3(npb, nslots), dim3(1024), 0, stream, t);
        hipLaunchKernelGGL(k_chunk_parts, dim3(ncb, nslots), dim3(256), 0, stream, t);
        return;
    }
    hipLaunchKernelGGL(k_polar_scan, dim3(1, nslots), dim3(1024), 0, stream, t);
    hipLaunchKernelGGL(k_scatter_scan, dim3(nb, nslots), dim3(256), 0, stream, t);
    hipLaunchKernelGGL(k_chunk_parts, dim3(ncb, nslots), dim3(256), 0, stream, t);
    hipLaunchKernelGGL(k_chunk_table, dim3(1, nslots), dim3(1024), 0, stream, t);
}

// the PrepSlot row of the resident scan, as far as k_chunk_table reads it
void table_slot_of(s2m_context* h, PrepSlot* ps)
{
    memset(ps, 0, sizeof(*ps));
    ps->n = (int32_t)h->reg.n_q; ps->n_chunks = h->hctx.n_chunks; ps->capacity = h->hctx.table_cap;
    ps->chunk_parts = h->reg.chunk_parts.as<int32_t>(); ps->wave_table = h->reg.wave_table.as<int2>(); ps->n_waves = h->reg.n_waves.as<int32_t>();
}

// The extent-only wave table of a single scan is built on demand: by whatever reads the table or its wave count before the
// scan's first optimisation has emitted the density-aware one (the observation and timing hooks, a handle with the density
// pass switched off).
void ensure_wave_table(s2m_context* h)
{
    if (!h->reg.table_stale) return;
    PrepTable t;
    table_slot_of(h, &t.s[0]);
    hipLaunchKernelGGL(k_chunk_table, dim3(1, 1), dim3(1024), 0, h->stream, t);
    h->reg.table_stale = false;
}

}  // namespace

int s2m::host::set_scan_impl(s2m_context* h, const void* pts, size_t n, size_t stride, bool on_device)
{
    S2M_HIP(h, hipSetDevice(h->device));
    PrepTable t;
    int rc = scan_slot_prepare(h, pts, n, stride, on_device, &t.s[0]);
    if (rc) return rc;
    if (n == 0) { h->reg.t_set_scan_ms = 0; h->reg.scan_timing_pending = false; h->reg.table_stale = false; return upload_ctx(h); }
    // the first and the last ordering kernel stamp the device's wall clock into the pinned block (s2m_last_timing): an event
    // record on either side is a packet of its own in the queue, 5.7 us of idle GPU each
    // (the last one is k_chunk_parts: PrepSlot::stamps)
    t.s[0].stamps = h->reg.h_stamps + kStampPrep0;
    const bool single = h->batch.parent == nullptr;       // the slots of a batch and of a stream of scans keep the six kernels
    launch_scan_prep(h->stream, t, 1, single);
    h->reg.table_stale = single;
    S2M_HIP(h, hipGetLastError());
    h->reg.scan_timing_pending = true;
    // (the DevCtx block goes to the device with the next launch that needs it: upload_ctx / push_state)
    // A host source (pageable or pinned) has been copied by the time this returns; the ordering kernels behind the copy
    // keep running.  A device-resident source is read asynchronously and must outlive the next synchronising call.
    if (!on_device) S2M_HIP(h, hipEventSynchronize(h->reg.ev_up));
    return S2M_OK;
}

namespace {

void fill_state(s2m_context* h, DevState* s, const float pose[6])
{
    memset(s, 0, sizeof(*s));
    memcpy(s->pose, pose, 24);
    memcpy(s->pose2[0], pose, 24);       // launch 0 runs with slot 0
    host_pose_to_transform(pose, s->T, s->sc);
    s->T_valid = 1;
    memcpy(s->matP, h->reg.persist_matP, sizeof(s->matP));
    s->isDegenerate = h->reg.persist_degenerate;
}

// `stamp` (pinned, may be null): where the kernel leaves the wall clock once the state is stored
int push_state(s2m_context* h, const float pose[6], unsigned long long* stamp = nullptr)
{
    DevState s;
    fill_state(h, &s, pose);
    ensure_wave_table(h);                                 // (k_set_state copies the wave count)
    if (h->ctx_dirty) {
        hipLaunchKernelGGL(k_set_ctx_state, dim3(1), dim3(64), 0, h->stream, h->reg.dctx.as<DevCtx>(), h->hctx, h->reg.state.as<DevState>(), s,
                           (const int32_t*)h->reg.n_waves.as<int32_t>(), stamp);
        h->ctx_dirty = false;
    } else
        hipLaunchKernelGGL(k_set_state, dim3(1), dim3(64), 0, h->stream, h->reg.state.as<DevState>(), s,
                           (const int32_t*)h->reg.n_waves.as<int32_t>(), stamp);
    S2M_HIP(h, hipGetLastError());
    return S2M_OK;
}

// The LM loop (:1304-1315) as a launch sequence.  One iteration L is either one launch of the fused kernel R(L), or -
// split - the certify kernel C(L) followed by the search kernel S(L) for the workgroups C put on its worklist (launch 0 of a
// scan, where nothing is certified yet: S alone, over every workgroup).  When the whole grid is co-resident iterations
// 1..n-2 are closed inside the prologue of the following R / C (solve_prev): every workgroup repeats the small solve, and
// a kernel boundary plus a one-workgroup kernel disappear from every iteration:
//   R0 F0 R1 R2' R3' ... R(n-1)' F(n-1)        (' = closes the iteration before it)
//   S0 F0 C1 S1 C2' S2 ... C(n-1)' S(n-1) F(n-1)
// The plain form  R0 F0 R1 F1 ...  remains for A/B measurements (S2M_NO_FUSE=1).
// Several scan slots (a batch) advance in lockstep: every launch has one grid row per slot.
constexpr int kFuseMaxBlocks = 512;
static_assert(sizeof(CtxTable) <= 4096 && sizeof(StateInitTable) <= 4096 && sizeof(PrepTable) <= 4096 && sizeof(SlotTable) <= 4096 &&
              sizeof(DensityStateArgs) <= 4096,
              "kernel arguments are limited to 4 KB");

// what one loop launches over: the scan slots (one for a single scan), the widest grid among them, their common workgroup shape
struct LoopShape {
    SlotTable tbl;
    int nslots = 1;
    int nblocks = 0;        // grid.x of the registration kernels: the largest DevCtx::nblocks among the slots
    int table_cap = 0;      // the largest wave-table capacity among the slots (grid of k_wave_density)
    int wpb = kBlock / 64;  // waves per workgroup (DevCtx::wpb, the same for every slot)
    bool batch = false;     // scan slots of a batch
    bool split = false;     // C + S per iteration instead of R
    bool late = false;      // the split iterations of this loop come late (few rows on the worklist): small search grid
    bool split_auto = false; // split if the loop's iterations are closed by k_finalize and the lean certify kernel applies
    bool wishes_done = false; // the density wishes of a pending re-split are in chunk_factor already (s2m_optimize_launch): the loop starts with k_chunk_table_density
    // a captured single-scan loop: the k_finalize that ends the range copies state + trace to `out` (the pinned mirror) and
    // stamps the wall clock at `stamp`; both null: the caller copies (plain launches, batches, diagnostics)
    DevState* out = nullptr;
    unsigned long long* stamp = nullptr;
};

LoopShape shape_of(s2m_context* h)
{
    LoopShape sh;
    memset(&sh.tbl, 0, sizeof(sh.tbl));
    sh.tbl.ctx[0] = h->reg.dctx.as<DevCtx>();
    sh.tbl.st[0] = h->reg.state.as<DevState>();
    sh.nslots = 1; sh.nblocks = h->hctx.nblocks; sh.table_cap = h->hctx.table_cap; sh.wpb = h->hctx.wpb;
    sh.batch = h->batch.parent != nullptr && !h->batch.slot_mode;
    sh.split = h->tune.split_mode == 1;
    return sh;
}

template <bool HOOK, int NW, int MINW, int MODE, int CNW>
inline void launch_k(hipStream_t s, const LoopShape& sh, int L, int flags, int grid_x = 0)
{
    hipLaunchKernelGGL((k_register<HOOK, NW, MINW, MODE, CNW>), dim3(grid_x > 0 ? std::min(grid_x, sh.nblocks) : sh.nblocks, sh.nslots), dim3(NW * 64), 0, s,
                       sh.tbl, L, flags);
}

// one fused launch R(L) in the workgroup shape of the scan (DevCtx::wpb); `hook`: the observation variant
inline void launch_fused(s2m_context* h, const LoopShape& sh, bool hook, int L, int solve_prev)
{
    constexpr int NW = kBlock / 64;
    const int fl = solve_prev ? kFlagSolvePrev : 0;
    if (sh.wpb == kBigWaves) {
        if (hook) launch_k<true, kBigWaves, 4, kFused, kBigWaves>(h->stream, sh, L, fl);
        else      launch_k<false, kBigWaves, 4, kFused, kBigWaves>(h->stream, sh, L, fl);
    } else if (sh.batch && h->tune.batch_minw == 4 && !hook) {
        launch_k<false, NW, 4, kFused, NW>(h->stream, sh, L, fl);          // two workgroups per CU (spills in the search path)
    } else {
        if (hook) launch_k<true, NW, 2, kFused, NW>(h->stream, sh, L, fl);
        else      launch_k<false, NW, 2, kFused, NW>(h->stream, sh, L, fl);
    }
}

// the search kernel S(L): over the worklist C(L) left, or (all) over every workgroup
// (small_grid: late in a loop the list is short - a few workgroups per slot walk it instead of one workgroup per row)
inline void launch_search(s2m_context* h, const LoopShape& sh, int L, bool all, bool small_grid = false)
{
    constexpr int NW = kBlock / 64;
    const bool close_after = small_grid && !all && h->tune.close_in_search;     // one workgroup per slot walks the list and closes the iteration
    const int fl = (all ? kFlagAll : 0) | (close_after ? kFlagCloseAfter : 0);
    const int gx = close_after ? 1 : ((small_grid && !all) ? h->tune.search_grid : 0);
    if (sh.wpb == kBigWaves) launch_k<false, NW, 2, kSearch, kBigWaves>(h->stream, sh, L, fl, gx);
    else if (sh.batch && h->tune.batch_minw == 4) launch_k<false, NW, 4, kSearch, NW>(h->stream, sh, L, fl, gx);
    else                     launch_k<false, NW, 2, kSearch, NW>(h->stream, sh, L, fl, gx);
}

inline void launch_certify(s2m_context* h, const LoopShape& sh, int L, int solve_prev, bool fused_loop)
{
    constexpr int NW = kBlock / 64;
    const int fl = solve_prev ? kFlagSolvePrev : 0;
    if (!fused_loop && sh.wpb == NW && h->tune.lean_certify)      // iterations closed by k_finalize: the 64-register kernel
        hipLaunchKernelGGL((k_certify_lean<NW, 1, kCertifyLeanWaves>), dim3(sh.nblocks, sh.nslots), dim3(NW * 64), 0, h->stream, sh.tbl, L);
    else if (sh.wpb == kBigWaves) launch_k<false, kBigWaves, kCertifyWavesBig, kCertify, kBigWaves>(h->stream, sh, L, fl);
    else                     launch_k<false, NW, kCertifyWaves, kCertify, NW>(h->stream, sh, L, fl);
}

// iteration L of the loop: R(L), or C(L) S(L)
inline void launch_iteration(s2m_context* h, const LoopShape& sh, int L, int solve_prev, bool fused_loop = true)
{
    if (!sh.split) { launch_fused(h, sh, false, L, solve_prev); return; }
    if (L == 0) { launch_search(h, sh, 0, true); return; }
    launch_certify(h, sh, L, solve_prev, fused_loop);
    launch_search(h, sh, L, false, sh.late);
}

// ends_range: the last launch of the range (it hands the record over, see LoopShape::out)
inline void launch_finalize(s2m_context* h, const LoopShape& sh, int L, int mode, bool ends_range = false)
{
    hipLaunchKernelGGL(k_finalize, dim3(1, sh.nslots), dim3(kFinThreads), 0, h->stream, sh.tbl, L, mode,
                       ends_range ? sh.out : (DevState*)nullptr, ends_range ? sh.stamp : (unsigned long long*)nullptr);
}

inline void launch_density(s2m_context* h, const LoopShape& sh)
{
    // re-split the wave table for the map density at the initial guess (the transform k_set_state just stored);
    // both kernels take everything from the DevCtx block, so the captured graph stays valid from scan to scan
    if (!sh.wishes_done) hipLaunchKernelGGL(k_wave_density, dim3((sh.table_cap + 3) / 4, sh.nslots), dim3(256), 0, h->stream, sh.tbl, h->tune.density_raw);
    hipLaunchKernelGGL(k_chunk_table_density, dim3(1, sh.nslots), dim3(1024), 0, h->stream, sh.tbl);
}

// Launches L0 .. L1-1 of the loop.  A range that starts after launch 0 begins like launch 1 does (transform rebuilt from the
// pose the k_finalize before it stored), and a range that ends before the last launch closes its last iteration with a
// k_finalize of its own: with early exit on, the loop is issued in two ranges and the second only if the first did not converge.
// `events`, if given, holds 2*n events recorded around every iteration's launches; with `coarse` only four pairs are recorded - around
// launch 0, launch 1, the run of back-to-back launches 2 .. n-2 (slots 4, 5) and launch n-1 (slots 6, 7) - so that the event
// packets do not break up the loop's back-to-back dispatch.
void enqueue_loop(s2m_context* h, const LoopShape& sh_in, hipEvent_t* events, bool coarse = false, int L0 = 0, int L1 = -1)
{
    const int n = h->prm.max_iter;
    if (L1 < 0) L1 = n;
    const bool fuse = h->tune.fuse_solve && sh_in.nblocks * sh_in.nslots <= h->tune.fuse_max_blocks;     // the whole grid co-resident (see above)
    LoopShape sh = sh_in;
    // S2M_SPLIT=2: from launch `split_from` on (the first launches search most points: there the certify kernel is only one
    // more launch in front of the search) the iterations of a loop closed by k_finalize run certify (lean) + search
    const bool split_late = sh.split_auto && !fuse && sh.wpb == kBlock / 64 && h->tune.lean_certify;   // (with early exit on these launches are the second range: issued only for scans that need them)
    if (h->tune.density_raw > 0 && L0 == 0) launch_density(h, sh);
    for (int L = L0; L < L1; L++) {
        const int slot = !coarse ? 2 * L : (L == 0 ? 0 : (L == 1 ? 2 : (L == n - 1 ? 6 : 4)));
        const bool open = events && (!coarse || L <= 2 || L == n - 1), close = events && (!coarse || L <= 1 || L >= n - 2);
        if (open) (void)hipEventRecord(events[slot], h->stream);
        sh.split = sh_in.split || (split_late && L >= h->tune.split_from);
        sh.late = !sh_in.split && sh.split;
        launch_iteration(h, sh, L, (fuse && L >= 2 && L != L0) ? 1 : 0, fuse);
        if (close) (void)hipEventRecord(events[slot + 1], h->stream);
        if ((!fuse || L == 0 || L == L1 - 1) && !(sh.late && h->tune.close_in_search)) launch_finalize(h, sh, L, 0, L == L1 - 1);   // (late split: the search launch closes)
    }
}

// part 0: the whole loop; 1: launches 0 .. seg-1; 2: launches seg .. max_iter-1
int get_graph(s2m_context* h, int nblocks, int part, hipGraphExec_t* out)
{
    // table_cap fixes both grids in the captured loop: k_register's (nblocks) and k_wave_density's
    LoopShape sh = shape_of(h);
    // Loop state + trace come back from inside the graph, into the pinned mirror (its address never changes).  The last launch
    // of a single scan's range is always a k_finalize (only the late split of a lockstep batch closes in the search kernel):
    // it writes the record there itself.  (A copy node as the graph's last: 4.4 us and a boundary; a copy issued behind the
    // graph starts ~10 us after the graph's last kernel.)  The first range - the whole loop, mostly - also stamps its end.
    sh.out = &h->reg.h_state[1];
    sh.stamp = part == 2 ? nullptr : h->reg.h_stamps + kStampLoop1;
    sh.wishes_done = h->batch.parent == nullptr;          // a single scan: k_wave_density_state ran as a plain launch in front of the graph
    const long long key = (((long long)h->hctx.table_cap * 4 + part) * 256 + (part ? h->tune.seg_iters : 0)) * 4 + (sh.split ? 1 : 0) + (sh.wpb == kBigWaves ? 2 : 0);
    auto it = h->reg.graphs.find(key);
    if (it != h->reg.graphs.end()) { *out = it->second; return S2M_OK; }
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    S2M_HIP(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    enqueue_loop(h, sh, nullptr, false, part == 2 ? h->tune.seg_iters : 0, part == 1 ? h->tune.seg_iters : -1);
    hipError_t e = hipStreamEndCapture(h->stream, &graph);
    if (e != hipSuccess || !graph) return fail(h, S2M_ERR_HIP, "hipStreamEndCapture", e);
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "hipGraphInstantiate", e);
    h->reg.graphs[key] = exec;
    *out = exec;
    return S2M_OK;
}

int launch_loop(s2m_context* h, int part = 0)
{
    const int nblocks = h->hctx.nblocks;
    // The first range is timed by device stamps: its start by the state upload before it (s2m_optimize_launch), its end by the
    // k_finalize that closes it.  The second range, issued only for a scan that did not converge in the first, keeps an event pair.
    if (h->tune.use_graph) {
        hipGraphExec_t exec = nullptr;
        int rc = get_graph(h, nblocks, part, &exec);
        if (rc == S2M_OK) {
            if (part == 2) S2M_HIP(h, hipEventRecord(h->reg.ev_a2, h->stream));
            S2M_HIP(h, hipGraphLaunch(exec, h->stream));
            if (part == 2) S2M_HIP(h, hipEventRecord(h->reg.ev_b2, h->stream));
            h->hctx.density_pending = 0;                  // cleared on the device by k_chunk_table_density: keep the host copy in step
            return S2M_OK;
        }
        h->tune.use_graph = false;       // capture unsupported here: fall back to plain launches
    }
    LoopShape sh = shape_of(h);
    sh.stamp = part == 2 ? nullptr : h->reg.h_stamps + kStampLoop1;
    sh.wishes_done = h->batch.parent == nullptr;
    if (part == 2) S2M_HIP(h, hipEventRecord(h->reg.ev_a2, h->stream));
    enqueue_loop(h, sh, nullptr, false, part == 2 ? h->tune.seg_iters : 0, part == 1 ? h->tune.seg_iters : -1);
    S2M_HIP(h, hipGetLastError());
    if (part == 2) S2M_HIP(h, hipEventRecord(h->reg.ev_b2, h->stream));
    S2M_HIP(h, hipMemcpyAsync(&h->reg.h_state[1], h->reg.state.p, sizeof(DevState) + sizeof(s2m_iter_trace) * h->prm.max_iter, hipMemcpyDeviceToHost, h->stream));
    h->hctx.density_pending = 0;
    return S2M_OK;
}

// the parameters the kernels read, into the host copy of the DevCtx block
void params_to_ctx(s2m_context* h, const s2m_params& prm)
{
    h->hctx.gate_f = nextafterf((float)prm.gate_sq, INFINITY);
    h->hctx.gate_r = nextafterf(sqrtf((float)prm.gate_sq), 0.0f);
    h->hctx.gate_sq = prm.gate_sq; h->hctx.plane_tol = prm.plane_tol; h->hctx.weight_scale = prm.weight_scale;
    h->hctx.weight_min = prm.weight_min; h->hctx.conv_deg = prm.conv_deg; h->hctx.conv_cm = prm.conv_cm;
    h->hctx.eig_thresh = prm.eig_thresh; h->hctx.min_corr = prm.min_corr; h->hctx.max_iter = prm.max_iter;
    h->hctx.early_exit = prm.early_exit;
    h->ctx_dirty = true;
}

// ---- ScanContext store ---------------------------------------------------------------------------
constexpr size_t kScDesc = (size_t)S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR;

// grow-with-copy (ensure() alone would drop the contents)
int sc_reserve(s2m_context* h, size_t want)
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

}  // namespace

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

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

const char* s2m_version(void) { return "liorf_amd s2m 0.1 (gfx950)"; }

int s2m_default_params(s2m_params* p)
{
    if (!p) return S2M_ERR_INVALID_ARG;
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(s2m_params);
    p->device_id = 0; p->stream = nullptr;
    p->k_neighbors = 5; p->gate_sq = 1.0; p->plane_tol = 0.2; p->weight_scale = 0.9; p->weight_min = 0.1;
    p->min_corr = 50; p->min_feats = 30; p->max_iter = 30; p->eig_thresh = 100.0f;
    p->conv_deg = 0.05; p->conv_cm = 0.05; p->z_tol = FLT_MAX; p->rot_tol = FLT_MAX;
    p->imu_type = 0; p->imu_rpy_weight = 0.01f; p->early_exit = 1;
    return S2M_OK;
}

int s2m_create(const s2m_params* p, s2m_handle* out)
{
    if (!out) return S2M_ERR_INVALID_ARG;
    *out = nullptr;
    s2m_params prm;
    if (p) {
        if (p->struct_size != sizeof(s2m_params)) return S2M_ERR_INVALID_ARG;
        prm = *p;
    } else s2m_default_params(&prm);
    if (prm.k_neighbors != 5 || prm.max_iter < 1 || prm.max_iter > kMaxIter || !(prm.gate_sq > 0.0)) return S2M_ERR_INVALID_ARG;

    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || prm.device_id < 0 || prm.device_id >= count)
        return S2M_ERR_NO_DEVICE;
    if (hipSetDevice(prm.device_id) != hipSuccess) return S2M_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, prm.device_id) != hipSuccess) return S2M_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return S2M_ERR_NO_DEVICE;   // kernels are built for gfx950 only

    s2m_context* h = new (std::nothrow) s2m_context();
    if (!h) return S2M_ERR_HIP;
    h->prm = prm; h->device = prm.device_id;
    if (const char* e = getenv("S2M_NO_GRAPH")) h->tune.use_graph = !(e[0] == '1');
    if (const char* e = getenv("S2M_NO_FUSE")) h->tune.fuse_solve = !(e[0] == '1');
    if (const char* e = getenv("S2M_DENSITY_RAW")) h->tune.density_raw = atoi(e);
    if (const char* e = getenv("S2M_BIG_BLOCKS")) h->tune.big_blocks = !(e[0] == '0');
    if (const char* e = getenv("S2M_SEGMENT")) h->tune.seg_iters = atoi(e);
    if (const char* e = getenv("S2M_SPLIT")) h->tune.split_mode = atoi(e);
    if (const char* e = getenv("S2M_LOCKSTEP")) h->tune.lockstep = !(e[0] == '0');
    if (const char* e = getenv("S2M_SPLIT_FROM")) h->tune.split_from = std::max(1, atoi(e));
    if (const char* e = getenv("S2M_SEARCH_GRID")) h->tune.search_grid = std::max(1, atoi(e));
    if (const char* e = getenv("S2M_CLOSE_IN_SEARCH")) h->tune.close_in_search = (e[0] == '1');
    if (const char* e = getenv("S2M_BATCH_MINW")) h->tune.batch_minw = atoi(e);
    if (const char* e = getenv("S2M_BATCH_ENTRIES")) h->tune.batch_entries = atoi(e);
    if (const char* e = getenv("S2M_LEAN")) h->tune.lean_certify = !(e[0] == '0');
    h->tune.fuse_max_blocks = kFuseMaxBlocks;
    if (const char* e = getenv("S2M_FUSE_MAX")) h->tune.fuse_max_blocks = atoi(e);

    auto bail = [&](int code) { s2m_destroy(h); return code; };
    if (prm.stream) { h->stream = static_cast<hipStream_t>(prm.stream); h->own_stream = false; }
    else {
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return bail(S2M_ERR_HIP);
        h->own_stream = true;
    }
    if (hipEventCreate(&h->reg.ev_a) != hipSuccess || hipEventCreate(&h->reg.ev_b) != hipSuccess ||
        hipEventCreate(&h->reg.ev_c) != hipSuccess || hipEventCreate(&h->reg.ev_d) != hipSuccess ||
        hipEventCreate(&h->reg.ev_a2) != hipSuccess || hipEventCreate(&h->reg.ev_b2) != hipSuccess ||
        hipEventCreateWithFlags(&h->reg.ev_up, hipEventDisableTiming) != hipSuccess) return bail(S2M_ERR_HIP);
    static_assert(sizeof(DevState) % 8 == 0, "the trace follows the state block");
    static_assert((sizeof(DevState) + sizeof(s2m_iter_trace) * kMaxIter) % 64 == 0, "a batch's state blocks (kid_states) all start on a 64-byte line");
    if (hipHostMalloc((void**)&h->reg.h_state, sizeof(DevState) * 2 + sizeof(s2m_iter_trace) * kMaxIter) != hipSuccess) return bail(S2M_ERR_HIP);
    h->reg.h_trace = reinterpret_cast<s2m_iter_trace*>(h->reg.h_state + 2);
    if (hipHostMalloc((void**)&h->reg.h_mm, 64) != hipSuccess) return bail(S2M_ERR_HIP);
    if (hipHostMalloc((void**)&h->reg.h_stamps, sizeof(unsigned long long) * kStampCount) != hipSuccess) return bail(S2M_ERR_HIP);
    memset(h->reg.h_stamps, 0, sizeof(unsigned long long) * kStampCount);
    {   // the constant-frequency counter behind wall_clock64(); a runtime that does not tell its rate leaves the timings at zero
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, prm.device_id) != hipSuccess || khz <= 0) { khz = 0; (void)hipGetLastError(); }
        h->reg.wall_clock_khz = khz;
    }
    if (hipHostMalloc((void**)&h->sc.h_stage, sizeof(double) * 1220) != hipSuccess) return bail(S2M_ERR_HIP);
    if (ensure(h, h->reg.state, sizeof(DevState) + sizeof(s2m_iter_trace) * kMaxIter) ||      // loop state, then the trace
        ensure(h, h->reg.dctx, sizeof(DevCtx)) || ensure(h, h->reg.mm, 64 + sizeof(uint32_t) * 8 * 1024) ||
        ensure(h, h->sc.bins, sizeof(uint32_t) * 1200) || ensure(h, h->sc.out, sizeof(double) * 1220) ||
        ensure(h, h->reg.q_counts, sizeof(int32_t) * kPolarCells))
        return bail(S2M_ERR_HIP);
    if (hipMemsetAsync(h->reg.q_counts.p, 0, sizeof(int32_t) * kPolarCells, h->stream) != hipSuccess) return bail(S2M_ERR_HIP);

    if (!(h->voxel.ws = vox_create())) return bail(S2M_ERR_HIP);
    if (!(h->loop.icp = icp_create())) return bail(S2M_ERR_HIP);

    memset(&h->hctx, 0, sizeof(h->hctx));
    h->hctx.nblocks = kBlocksQuantum;
    h->hctx.wpb = kBlock / 64;
    if (ensure_rows(h, kBlocksQuantum)) return bail(S2M_ERR_HIP);
    h->hctx.state = h->reg.state.as<DevState>();
    h->hctx.trace = reinterpret_cast<s2m_iter_trace*>(h->reg.state.as<DevState>() + 1);
    params_to_ctx(h, prm);
    if (const char* e = getenv("S2M_ABLATE")) h->hctx.ablate = atoi(e);
    h->hctx.tune[0] = 0; h->hctx.tune[1] = 0; h->hctx.tune[2] = 0; h->hctx.tune[3] = 2;      // tune[0..2] are spare: no kernel reads them
    if (const char* e = getenv("S2M_TUNE")) { (void)sscanf(e, "%d,%d,%d,%d", &h->hctx.tune[0], &h->hctx.tune[1], &h->hctx.tune[2], &h->hctx.tune[3]); h->tune.tune_env = true; }
    h->ctx_dirty = true;
    if (upload_ctx(h) != S2M_OK) return bail(S2M_ERR_HIP);
    *out = h;
    return S2M_OK;
}

int s2m_destroy(s2m_handle h)
{
    if (!h) return S2M_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    loop_drop_pending(h, true);                                                         // (a launched loop closure uses the loop buffers)
    pg_drop_pending(h, true);                                                           // (a launched optimise uses the pose graph's)
    for (hipStream_t st : h->batch.branch_streams) (void)hipStreamSynchronize(st);      // (slot work in flight uses the slots' buffers)
    if (h->gmap.copy_stream) (void)hipStreamSynchronize(h->gmap.copy_stream);
    for (s2m_context* k : h->batch.kids) (void)s2m_destroy(k);
    h->batch.kids.clear();
    if (h->batch.state_borrowed) { h->reg.state.forget(); h->reg.h_state = nullptr; }    // (the parent's blocks)
    for (auto& kv : h->batch.graphs) (void)hipGraphExecDestroy(kv.second);
    for (auto& kv : h->reg.graphs) (void)hipGraphExecDestroy(kv.second);
    for (const std::vector<hipEvent_t>* evs : { &h->batch.branch_events, &h->batch.prep_events, &h->reg.iter_events })
        for (hipEvent_t e : *evs) (void)hipEventDestroy(e);
    for (hipEvent_t e : { h->batch.ev_fork, h->batch.ev_prep, h->gmap.ev_xf[0], h->gmap.ev_xf[1], h->gmap.ev_cp[0], h->gmap.ev_cp[1],
                          h->reg.ev_a, h->reg.ev_b, h->reg.ev_a2, h->reg.ev_b2, h->reg.ev_c, h->reg.ev_d, h->reg.ev_up })
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t st : h->batch.branch_streams) (void)hipStreamDestroy(st);
    if (h->gmap.copy_stream) (void)hipStreamDestroy(h->gmap.copy_stream);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    vox_destroy(h->voxel.ws);
    icp_destroy(h->loop.icp);
    for (void* p : { (void*)h->batch.h_kid_states, (void*)h->reg.h_state, (void*)h->reg.h_mm, (void*)h->reg.h_stamps, (void*)h->sc.h_stage, (void*)h->proj.h_count,
                     (void*)h->pg.h_sc })
        if (p) (void)hipHostFree(p);
    delete h;                                              // every DevBuf and the key-frame arena go with their owners
    return S2M_OK;
}

const char* s2m_last_error(s2m_handle h) { return h ? h->err.c_str() : "null handle"; }

int s2m_get_params(s2m_handle h, s2m_params* out)
{
    if (!h || !out) return S2M_ERR_INVALID_ARG;
    *out = h->prm;
    return S2M_OK;
}

int s2m_set_params(s2m_handle h, const s2m_params* p)
{
    if (!h || !p) return S2M_ERR_INVALID_ARG;
    if (p->struct_size != sizeof(s2m_params)) return fail(h, S2M_ERR_INVALID_ARG, "s2m_params.struct_size does not match this library");
    if (p->device_id != h->prm.device_id || p->stream != h->prm.stream || p->k_neighbors != h->prm.k_neighbors ||
        p->gate_sq != h->prm.gate_sq)
        return fail(h, S2M_ERR_INVALID_ARG, "device_id, stream, k_neighbors and gate_sq are fixed at s2m_create (the search grid is built for the gate)");
    if (p->max_iter < 1 || p->max_iter > kMaxIter) return fail(h, S2M_ERR_INVALID_ARG, "max_iter out of range");
    if (h->reg.opt_pending) return fail(h, S2M_ERR_INVALID_ARG, "an optimize launch is pending: collect it first");
    if (p->max_iter != h->prm.max_iter) {               // the captured loops hold max_iter launches
        S2M_HIP(h, hipSetDevice(h->device));
        S2M_HIP(h, hipStreamSynchronize(h->stream));
        for (auto& kv : h->reg.graphs) (void)hipGraphExecDestroy(kv.second);
        h->reg.graphs.clear();
        for (auto& kv : h->batch.graphs) (void)hipGraphExecDestroy(kv.second);     // (every branch of a batch graph is such a loop)
        h->batch.graphs.clear();
    }
    h->prm = *p;
    params_to_ctx(h, h->prm);                           // uploaded by the next call that launches anything
    return S2M_OK;
}

int s2m_set_map(s2m_handle h, const void* pts, size_t n, size_t stride_bytes)
{ return set_map_impl(h, pts, n, stride_bytes, false); }
int s2m_set_map_device(s2m_handle h, const void* d_pts, size_t n, size_t stride_bytes)
{ return set_map_impl(h, d_pts, n, stride_bytes, true); }
int s2m_set_scan(s2m_handle h, const void* pts, size_t n, size_t stride_bytes)
{ return set_scan_impl(h, pts, n, stride_bytes, false); }
int s2m_set_scan_device(s2m_handle h, const void* d_pts, size_t n, size_t stride_bytes)
{ return set_scan_impl(h, d_pts, n, stride_bytes, true); }

int s2m_optimize_launch(s2m_handle h, const float pose[6])
{
    if (!h || !pose) return S2M_ERR_INVALID_ARG;
    if (!h->reg.have_scan) return fail(h, S2M_ERR_NO_SCAN, "s2m_set_scan has not been called");
    S2M_HIP(h, hipSetDevice(h->device));
    memcpy(h->reg.pending_pose_in, pose, 24);
    h->reg.opt_pending = true;
    h->reg.pending_skipped = 0;
    if (h->reg.n_m == 0) { h->reg.pending_skipped = 1; return S2M_OK; }                    // :1297
    if ((int)h->reg.n_q <= h->prm.min_feats) { h->reg.pending_skipped = 2; return S2M_OK; } // :1300
    int rc;
    if (!h->batch.parent && h->hctx.density_pending && h->tune.density_raw > 0) {
        // the first optimisation of a single scan: the density wishes, the DevCtx block and the loop state in one plain launch
        // (k_wave_density_state needs no wave table; the graph behind it starts with k_chunk_table_density)
        DensityStateArgs a;
        a.c = h->hctx;
        fill_state(h, &a.v, pose);
        a.cdst = h->reg.dctx.as<DevCtx>(); a.sdst = h->reg.state.as<DevState>();
        a.stamp = h->reg.h_stamps + kStampLoop0;
        a.raw_limit = h->tune.density_raw;
        hipLaunchKernelGGL(k_wave_density_state, dim3((h->hctx.n_chunks + 3) / 4 + 1), dim3(256), 0, h->stream, a);       // (+ 1: the workgroup that stores the blocks)
        S2M_HIP(h, hipGetLastError());
        h->ctx_dirty = false;
        h->reg.table_stale = false;                       // k_chunk_table_density emits the table
    } else if ((rc = push_state(h, pose, h->reg.h_stamps + kStampLoop0))) return rc;      // (with the DevCtx block when that changed)
    h->reg.seg_pending = h->prm.early_exit && h->tune.seg_iters > 1 && h->tune.seg_iters < h->prm.max_iter;
    if ((rc = launch_loop(h, h->reg.seg_pending ? 1 : 0))) return rc;        // (state + trace come back with it)
    return S2M_OK;
}

int s2m_optimize_collect(s2m_handle h, float pose[6], const s2m_imu_init* imu, s2m_result* out)
{
    if (!h || !pose) return S2M_ERR_INVALID_ARG;
    if (!h->reg.opt_pending) return fail(h, S2M_ERR_INVALID_ARG, "no optimize launch pending");
    h->reg.opt_pending = false;
    s2m_result r;
    memset(&r, 0, sizeof(r));
    r.skipped = h->reg.pending_skipped;
    h->reg.last_trace_n = 0;
    float t[6];
    memcpy(t, h->reg.pending_pose_in, 24);
    if (!r.skipped) {
        S2M_HIP(h, hipSetDevice(h->device));
        S2M_HIP(h, hipStreamSynchronize(h->stream));
        if (h->batch.parent && !h->batch.slot_mode) h->reg.t_optimize_ms = h->batch.parent->reg.t_optimize_ms;      // a slot of a batch: the batch was timed as a whole
        else h->reg.t_optimize_ms = stamps_ms(h, kStampLoop0, kStampLoop1);
        if (h->reg.seg_pending && !h->reg.h_state[1].done) {
            // the first range did not converge: the rest of the loop
            int rc2 = launch_loop(h, 2);
            if (rc2) return rc2;
            S2M_HIP(h, hipStreamSynchronize(h->stream));
            float t2 = 0.0f;
            S2M_HIP(h, hipEventElapsedTime(&t2, h->reg.ev_a2, h->reg.ev_b2));
            h->reg.t_optimize_ms += t2;
        }
        h->reg.seg_pending = false;
        const DevState& s = h->reg.h_state[1];
        memcpy(t, s.pose, 24);
        r.iters_run = s.iters_run; r.converged = s.converged; r.is_degenerate = s.isDegenerate;
        r.n_sel_last = s.n_sel_last;
        h->reg.persist_degenerate = s.isDegenerate;
        memcpy(h->reg.persist_matP, s.matP, sizeof(s.matP));
        // trace: executed iterations; a loop that stalled at iteration k (fewer than min_corr correspondences,
        // pose unchanged, :1178-1180) repeats that no-op record for the iterations the reference would still run
        int n_exec = s.iters_run, stall_at = -1;
        for (int i = 0; i < n_exec && i < kMaxIter; i++) {
            if (stall_at >= 0) { h->reg.last_trace[i] = h->reg.last_trace[stall_at]; continue; }
            h->reg.last_trace[i] = h->reg.h_trace[i];
            if (s.stalled && !h->reg.h_trace[i].stepped) stall_at = i;
        }
        h->reg.last_trace_n = n_exec < kMaxIter ? n_exec : kMaxIter;
        host_transform_update(h->prm, imu, t, r.affine);                           // :1317
    } else {
        host_pose_to_transform(t, r.affine, nullptr);
        r.is_degenerate = h->reg.persist_degenerate;
    }
    memcpy(r.pose, t, 24);
    memcpy(pose, t, 24);
    if (out) *out = r;
    return S2M_OK;
}

int s2m_optimize_resident(s2m_handle h, float pose[6], const s2m_imu_init* imu, s2m_result* out)
{
    int rc = s2m_optimize_launch(h, pose);
    if (rc) return rc;
    return s2m_optimize_collect(h, pose, imu, out);
}

int s2m_optimize(s2m_handle h, const void* scan, size_t n, size_t stride_bytes, float pose[6],
                 const s2m_imu_init* imu, s2m_result* out)
{
    int rc = s2m_set_scan(h, scan, n, stride_bytes);
    if (rc) return rc;
    return s2m_optimize_resident(h, pose, imu, out);
}

// ---- a batch of scans against one resident map -------------------------------------------------------
namespace {

// field by field (the struct has padding): everything a slot has to take over from its parent
bool same_params_but_stream(const s2m_params& a, const s2m_params& b)
{
    return a.struct_size == b.struct_size && a.device_id == b.device_id && a.k_neighbors == b.k_neighbors && a.gate_sq == b.gate_sq &&
           a.plane_tol == b.plane_tol && a.weight_scale == b.weight_scale && a.weight_min == b.weight_min && a.min_corr == b.min_corr &&
           a.min_feats == b.min_feats && a.max_iter == b.max_iter && a.eig_thresh == b.eig_thresh && a.conv_deg == b.conv_deg &&
           a.conv_cm == b.conv_cm && a.z_tol == b.z_tol && a.rot_tol == b.rot_tol && a.imu_type == b.imu_type &&
           a.imu_rpy_weight == b.imu_rpy_weight && a.early_exit == b.early_exit;
}

// child b borrows the parent's map index (no copy) and its per-scan certificates are void when the index changed
int adopt_map(s2m_context* h, s2m_context* k)
{
    if (k->batch.adopted_epoch == h->batch.map_epoch) return S2M_OK;
    k->reg.n_m = h->reg.n_m;
    k->hctx.n_m = h->hctx.n_m;
    k->hctx.g = h->hctx.g;
    k->hctx.map_sorted = h->hctx.map_sorted;
    k->hctx.cell_start = h->hctx.cell_start;
    k->ctx_dirty = true;
    k->batch.adopted_epoch = h->batch.map_epoch;
    if (k->reg.have_scan && k->reg.n_q > 0 && k->reg.cert.p) {
        S2M_HIP(k, hipMemsetAsync(k->reg.cert.p, 0, sizeof(float4) * k->reg.n_q, k->stream));
        S2M_HIP(k, hipMemsetAsync(k->reg.aux.p, 0, sizeof(int4) * k->reg.n_q, k->stream));
    }
    return S2M_OK;
}

int ensure_kids(s2m_context* h, int n)
{
    while ((int)h->batch.kids.size() < n) {
        s2m_params p = h->prm;
        p.stream = h->stream;                              // everything outside the captured graph is ordered on the parent's stream
        s2m_context* k = nullptr;
        const int rc = s2m_create(&p, &k);
        if (rc) return fail(h, rc, "batch: could not create a scan slot");
        k->batch.parent = h;
        k->hctx.ablate = h->hctx.ablate;
        memcpy(k->hctx.tune, h->hctx.tune, sizeof(h->hctx.tune));
        {   // the slot's loop state and trace live in the parent's block
            constexpr size_t kStride = sizeof(DevState) + sizeof(s2m_iter_trace) * kMaxIter;
            if (!h->batch.kid_states.p) {
                if (ensure(h, h->batch.kid_states, kStride * kMaxSlots) != S2M_OK ||
                    hipHostMalloc((void**)&h->batch.h_kid_states, sizeof(DevState) + kStride * kMaxSlots) != hipSuccess) {
                    (void)s2m_destroy(k);
                    return fail(h, S2M_ERR_HIP, "batch: state block allocation failed");
                }
            }
            const size_t slot = h->batch.kids.size();
            (void)k->reg.state.reset();                        // from here on an alias: forgotten, not freed, in s2m_destroy
            (void)hipHostFree(k->reg.h_state);
            k->reg.state.p = h->batch.kid_states.as<unsigned char>() + kStride * slot; k->reg.state.cap = kStride;
            k->reg.h_state = reinterpret_cast<DevState*>(h->batch.h_kid_states + kStride * slot);      // [1] = the download area of this slot
            k->reg.h_trace = reinterpret_cast<s2m_iter_trace*>(k->reg.h_state + 2);
            k->batch.state_borrowed = true;
            k->hctx.state = k->reg.state.as<DevState>();
            k->hctx.trace = reinterpret_cast<s2m_iter_trace*>(k->reg.state.as<DevState>() + 1);
            k->ctx_dirty = true;
        }
        h->batch.kids.push_back(k);
        hipStream_t st = nullptr;
        hipEvent_t ev = nullptr, ev2 = nullptr;
        // The streams of neighbouring slots get different priorities.  HIP deals a process's streams of one priority onto a small
        // pool of hardware queues in creation order (GPU_MAX_HW_QUEUES, default 4), and two streams that land on one queue run
        // strictly one after the other: with other streams alive in the process (a ROS node has them) the two slots of a stream
        // of scans could end up sharing a queue and lose the overlap of one's preparation with the other's loop.  Streams of
        // different priority never share a hardware queue, whatever else the process has created.
        int prio_least = 0, prio_greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
        const int prio = (h->batch.kids.size() & 1) ? prio_greatest : prio_least;
        if (hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio) != hipSuccess || hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&ev2, hipEventDisableTiming) != hipSuccess)
            return fail(h, S2M_ERR_HIP, "batch: stream / event creation failed");
        h->batch.branch_streams.push_back(st);
        h->batch.branch_events.push_back(ev);
        h->batch.prep_events.push_back(ev2);
        h->batch.prep_pending.push_back(0);
    }
    if (!h->batch.ev_fork && hipEventCreateWithFlags(&h->batch.ev_fork, hipEventDisableTiming) != hipSuccess) return fail(h, S2M_ERR_HIP, "batch: event creation failed");
    if (!h->batch.ev_prep && hipEventCreateWithFlags(&h->batch.ev_prep, hipEventDisableTiming) != hipSuccess) return fail(h, S2M_ERR_HIP, "batch: event creation failed");
    return S2M_OK;
}

// One graph for the whole batch.  Lockstep (default): the slots' loops advance together, every launch of the loop has one
// grid row per slot (slots of different workgroup shape form groups, one loop per group on a branch of its own).  Otherwise
// (S2M_LOCKSTEP=0, A/B measurements): a fork, one branch per scan with that scan's loop, a join.
// part 0: the whole loop; 1: launches 0 .. seg-1; 2: launches seg .. max_iter-1 (as get_graph)
int get_batch_graph(s2m_context* h, const std::vector<int>& live, int part, hipGraphExec_t* out)
{
    std::vector<int> key;
    key.push_back(part); key.push_back(part ? h->tune.seg_iters : 0);
    for (int b : live) { key.push_back(b); key.push_back(h->batch.kids[(size_t)b]->hctx.table_cap); key.push_back(h->batch.kids[(size_t)b]->hctx.wpb); }
    auto it = h->batch.graphs.find(key);
    if (it != h->batch.graphs.end()) { *out = it->second; return S2M_OK; }
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    // the loops to run: (shape, stream to run it on)
    std::vector<LoopShape> loops;
    if (h->tune.lockstep) {
        for (int wpb : { kBlock / 64, kBigWaves }) {
            LoopShape sh;
            memset(&sh.tbl, 0, sizeof(sh.tbl));
            sh.nslots = 0; sh.wpb = wpb; sh.batch = true;
            for (int b : live) {
                s2m_context* k = h->batch.kids[(size_t)b];
                if (k->hctx.wpb != wpb) continue;
                sh.tbl.ctx[sh.nslots] = k->reg.dctx.as<DevCtx>();
                sh.tbl.st[sh.nslots] = k->reg.state.as<DevState>();
                sh.nslots++;
                sh.nblocks = std::max(sh.nblocks, k->hctx.nblocks);
                sh.table_cap = std::max(sh.table_cap, k->hctx.table_cap);
            }
            sh.split = h->tune.split_mode == 1;         // (default: decided in enqueue_loop - split where the loop is not fused)
            sh.split_auto = h->tune.split_mode == 2 || h->tune.split_mode < 0;   // (default: certify (lean) + search from launch split_from on, where k_finalize closes the iterations)
            if (sh.nslots) loops.push_back(sh);
        }
    } else
        for (int b : live) loops.push_back(shape_of(h->batch.kids[(size_t)b]));
    S2M_HIP(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    bool ok = hipEventRecord(h->batch.ev_fork, h->stream) == hipSuccess;
    hipStream_t keep = h->stream;
    for (size_t j = 0; j < loops.size(); j++) {
        hipStream_t br = h->batch.branch_streams[j];
        ok = ok && hipStreamWaitEvent(br, h->batch.ev_fork, 0) == hipSuccess;
        h->stream = br;                                       // (enqueue_loop launches on the handle's stream; settings are the parent's)
        enqueue_loop(h, loops[j], nullptr, false, part == 2 ? h->tune.seg_iters : 0, part == 1 ? h->tune.seg_iters : -1);
        h->stream = keep;
        ok = ok && hipEventRecord(h->batch.branch_events[j], br) == hipSuccess;
        ok = ok && hipStreamWaitEvent(h->stream, h->batch.branch_events[j], 0) == hipSuccess;
    }
    hipError_t e = hipStreamEndCapture(h->stream, &graph);
    if (!ok || e != hipSuccess || !graph) return fail(h, S2M_ERR_HIP, "batch: stream capture failed", e);
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return fail(h, S2M_ERR_HIP, "batch: hipGraphInstantiate", e);
    h->batch.graphs[key] = exec;
    *out = exec;
    return S2M_OK;
}

}  // namespace

int s2m_batch_set_scan(s2m_handle h, int slot, const void* pts, size_t n, size_t stride_bytes, int on_device)
{
    if (!h || slot < 0 || slot >= 64) return S2M_ERR_INVALID_ARG;
    S2M_HIP(h, hipSetDevice(h->device));
    int rc = ensure_kids(h, slot + 1);
    if (rc) return rc;
    s2m_context* k = h->batch.kids[(size_t)slot];
    if ((rc = adopt_map(h, k))) return fail(h, rc, k->err.c_str());
    // The ordering of one slot's scan does not depend on the others': it runs on the slot's own stream, behind everything
    // issued on the handle's stream so far (the previous batch read the slot's buffers), and the batch launch waits for it.
    hipStream_t br = h->batch.branch_streams[(size_t)slot];
    S2M_HIP(h, hipEventRecord(h->batch.ev_prep, h->stream));
    S2M_HIP(h, hipStreamWaitEvent(br, h->batch.ev_prep, 0));
    k->stream = br;
    rc = set_scan_impl(k, pts, n, stride_bytes, on_device != 0);
    k->stream = h->stream;
    if (rc) { (void)hipStreamSynchronize(br); return fail(h, rc, k->err.c_str()); }
    S2M_HIP(h, hipEventRecord(h->batch.prep_events[(size_t)slot], br));
    h->batch.prep_pending[(size_t)slot] = 1;
    return S2M_OK;
}

int s2m_batch_set_scans(s2m_handle h, int n_scans, const void* const* scans, const size_t* sizes, size_t stride_bytes, int on_device)
{
    if (!h || n_scans < 1 || n_scans > kMaxSlots || !scans || !sizes) return S2M_ERR_INVALID_ARG;
    S2M_HIP(h, hipSetDevice(h->device));
    int rc = ensure_kids(h, n_scans);
    if (rc) return rc;
    // Work still queued on a slot's own stream (a preparation from s2m_batch_set_scan, a loop from s2m_slot_optimize_launch)
    // uses the buffers this call rewrites: the handle's stream waits for it first.
    for (int b = 0; b < n_scans; b++) {
        S2M_HIP(h, hipEventRecord(h->batch.prep_events[(size_t)b], h->batch.branch_streams[(size_t)b]));
        S2M_HIP(h, hipStreamWaitEvent(h->stream, h->batch.prep_events[(size_t)b], 0));
        h->batch.prep_pending[(size_t)b] = 0;
    }
    for (int b0 = 0; b0 < n_scans; b0 += kPrepSlots) {
        PrepTable t;
        const int nb = std::min(kPrepSlots, n_scans - b0);
        for (int j = 0; j < nb; j++) {
            s2m_context* k = h->batch.kids[(size_t)(b0 + j)];
            if ((rc = adopt_map(h, k)) == S2M_OK) rc = scan_slot_prepare(k, scans[b0 + j], sizes[b0 + j], stride_bytes, on_device != 0, &t.s[j]);
            if (rc) {
                // no slot of this call holds a scan after a failure: the groups before this one were ordered, but a batch
                // of which some scans are missing is of no use to the caller
                for (int q = 0; q <= b0 + j; q++) h->batch.kids[(size_t)q]->reg.have_scan = false;
                (void)hipStreamSynchronize(h->stream);
                return fail(h, rc, k->err.c_str());
            }
            k->reg.t_set_scan_ms = 0; k->reg.scan_timing_pending = false;
        }
        launch_scan_prep(h->stream, t, nb);
        S2M_HIP(h, hipGetLastError());
    }
    if (!on_device) S2M_HIP(h, hipStreamSynchronize(h->stream));       // the callers' buffers are free again
    return S2M_OK;
}

// ---- a stream of scans: slot k's preparation and loop run on slot k's own stream, so that the ordering of scan i+1 (slot B)
// overlaps the LM loop of scan i (slot A) - the reference does the two strictly one after the other (:257-265) ----------
int s2m_slot_set_scan(s2m_handle h, int slot, const void* pts, size_t n, size_t stride_bytes, int on_device)
{ return s2m_batch_set_scan(h, slot, pts, n, stride_bytes, on_device); }

int s2m_slot_optimize_launch(s2m_handle h, int slot, const float pose[6])
{
    if (!h || slot < 0 || slot >= (int)h->batch.kids.size() || !pose) return S2M_ERR_INVALID_ARG;
    s2m_context* k = h->batch.kids[(size_t)slot];
    if (!k->reg.have_scan) return fail(h, S2M_ERR_NO_SCAN, "s2m_slot_set_scan has not been called for this slot");
    S2M_HIP(h, hipSetDevice(h->device));
    int rc;
    if (!same_params_but_stream(k->prm, h->prm)) {
        s2m_params p = h->prm;
        p.stream = k->prm.stream;
        if ((rc = s2m_set_params(k, &p))) return fail(h, rc, k->err.c_str());
    }
    h->batch.prep_pending[(size_t)slot] = 0;                       // (the preparation is ahead of the loop on the same stream)
    k->stream = h->batch.branch_streams[(size_t)slot];
    k->batch.slot_mode = true;
    rc = adopt_map(h, k);
    if (!rc) rc = s2m_optimize_launch(k, pose);
    k->stream = h->stream;
    return rc ? fail(h, rc, k->err.c_str()) : S2M_OK;
}

int s2m_slot_optimize_collect(s2m_handle h, int slot, float pose[6], const s2m_imu_init* imu, s2m_result* out)
{
    if (!h || slot < 0 || slot >= (int)h->batch.kids.size() || !pose) return S2M_ERR_INVALID_ARG;
    s2m_context* k = h->batch.kids[(size_t)slot];
    k->stream = h->batch.branch_streams[(size_t)slot];
    const int rc = s2m_optimize_collect(k, pose, imu, out);
    k->stream = h->stream;
    k->batch.slot_mode = false;
    return rc ? fail(h, rc, k->err.c_str()) : S2M_OK;
}

int s2m_optimize_batch_launch(s2m_handle h, int n_scans, const float* poses)
{
    if (!h || n_scans < 1 || n_scans > 64 || !poses) return S2M_ERR_INVALID_ARG;
    if ((int)h->batch.kids.size() < n_scans) return fail(h, S2M_ERR_NO_SCAN, "s2m_batch_set_scan has not been called for every slot");
    S2M_HIP(h, hipSetDevice(h->device));
    std::vector<int> live;
    int rc;
    for (size_t b = 0; b < h->batch.prep_pending.size(); b++)
        if (h->batch.prep_pending[b]) { S2M_HIP(h, hipStreamWaitEvent(h->stream, h->batch.prep_events[b], 0)); h->batch.prep_pending[b] = 0; }
    for (int b = 0; b < n_scans; b++) {
        s2m_context* k = h->batch.kids[(size_t)b];
        if (!k->reg.have_scan) return fail(h, S2M_ERR_NO_SCAN, "s2m_batch_set_scan has not been called for every slot");
        if (!same_params_but_stream(k->prm, h->prm)) {     // any parameter changed on the parent since the slot was made
            s2m_params p = h->prm;
            p.stream = k->prm.stream;
            if ((rc = s2m_set_params(k, &p))) return fail(h, rc, k->err.c_str());
        }
        if ((rc = adopt_map(h, k))) return fail(h, rc, k->err.c_str());
        memcpy(k->reg.pending_pose_in, poses + 6 * (size_t)b, 24);
        k->reg.opt_pending = true;
        k->reg.pending_skipped = 0;
        if (k->reg.n_m == 0) { k->reg.pending_skipped = 1; continue; }                            // :1297
        if ((int)k->reg.n_q <= k->prm.min_feats) { k->reg.pending_skipped = 2; continue; }         // :1300
        live.push_back(b);
    }
    {   // DevCtx blocks that changed and the loop state every live slot starts from: one launch per kCtxSlots / kInitSlots slots
        CtxTable ct; int nc = 0;
        auto flush_ctx = [&]() { if (nc) { for (int j = nc; j < kCtxSlots; j++) ct.dst[j] = nullptr; hipLaunchKernelGGL(k_set_ctxs, dim3(nc), dim3(64), 0, h->stream, ct); nc = 0; } };
        for (int b = 0; b < n_scans; b++) {
            s2m_context* k = h->batch.kids[(size_t)b];
            if (!k->ctx_dirty) continue;
            ct.dst[nc] = k->reg.dctx.as<DevCtx>(); ct.v[nc] = k->hctx; nc++;
            k->ctx_dirty = false;
            if (nc == kCtxSlots) flush_ctx();
        }
        flush_ctx();
        StateInitTable it; int ni = 0;
        auto flush_init = [&]() { if (ni) { for (int j = ni; j < kInitSlots; j++) it.s[j].dst = nullptr; hipLaunchKernelGGL(k_init_states, dim3(ni), dim3(256), 0, h->stream, it); ni = 0; } };
        for (int b : live) {
            s2m_context* k = h->batch.kids[(size_t)b];
            DevState s0;
            fill_state(k, &s0, poses + 6 * (size_t)b);
            StateInit& si = it.s[ni++];
            si.dst = k->reg.state.as<DevState>(); si.n_waves = k->reg.n_waves.as<int32_t>();
            memcpy(si.pose, s0.pose, sizeof(si.pose)); memcpy(si.T, s0.T, sizeof(si.T)); memcpy(si.sc, s0.sc, sizeof(si.sc));
            memcpy(si.matP, s0.matP, sizeof(si.matP)); si.isDegenerate = s0.isDegenerate;
            if (ni == kInitSlots) flush_init();
        }
        flush_init();
        S2M_HIP(h, hipGetLastError());
    }
    // With early exit on the loops are issued as launches 0 .. seg-1 and, only if some slot has not converged by then, the rest
    // (s2m_optimize_batch_collect looks at the slots' `done` flags, which come back with the states anyway): the launches behind
    // the convergence of every slot - idle, but a kernel boundary and a k_finalize each - were a fifth of an early-exit batch.
    h->batch.seg_pending = h->prm.early_exit && h->tune.seg_iters > 1 && h->tune.seg_iters < h->prm.max_iter;
    h->batch.live = live;
    S2M_HIP(h, hipEventRecord(h->reg.ev_a, h->stream));
    if (!live.empty()) {
        hipGraphExec_t exec = nullptr;
        if ((rc = get_batch_graph(h, live, h->batch.seg_pending ? 1 : 0, &exec))) return rc;
        S2M_HIP(h, hipGraphLaunch(exec, h->stream));
    }
    S2M_HIP(h, hipEventRecord(h->reg.ev_b, h->stream));
    for (int b : live) h->batch.kids[(size_t)b]->hctx.density_pending = 0;
    if (!live.empty()) {
        // state + trace of every slot up to the last live one, in one copy (the slots' blocks are contiguous)
        constexpr size_t kStride = sizeof(DevState) + sizeof(s2m_iter_trace) * kMaxIter;
        const size_t upto = (size_t)live.back() + 1;
        S2M_HIP(h, hipMemcpyAsync(h->batch.h_kid_states + sizeof(DevState), h->batch.kid_states.p, kStride * upto, hipMemcpyDeviceToHost, h->stream));
    }
    return S2M_OK;
}

int s2m_optimize_batch_collect(s2m_handle h, int n_scans, float* poses, const s2m_imu_init* imu, s2m_result* out)
{
    if (!h || n_scans < 1 || (int)h->batch.kids.size() < n_scans || !poses) return S2M_ERR_INVALID_ARG;
    S2M_HIP(h, hipSetDevice(h->device));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    S2M_HIP(h, hipEventElapsedTime(&h->reg.t_optimize_ms, h->reg.ev_a, h->reg.ev_b));
    if (h->batch.seg_pending && !h->batch.live.empty()) {
        h->batch.seg_pending = false;
        bool all_done = true;
        for (int b : h->batch.live) all_done = all_done && h->batch.kids[(size_t)b]->reg.h_state[1].done != 0;
        if (!all_done) {
            // some slot needs more than the first range: the rest of the loop for all of them (a converged slot's launches return at once)
            hipGraphExec_t exec = nullptr;
            int rc2 = get_batch_graph(h, h->batch.live, 2, &exec);
            if (rc2) return rc2;
            S2M_HIP(h, hipEventRecord(h->reg.ev_a2, h->stream));
            S2M_HIP(h, hipGraphLaunch(exec, h->stream));
            S2M_HIP(h, hipEventRecord(h->reg.ev_b2, h->stream));
            constexpr size_t kStride = sizeof(DevState) + sizeof(s2m_iter_trace) * kMaxIter;
            const size_t upto = (size_t)h->batch.live.back() + 1;
            S2M_HIP(h, hipMemcpyAsync(h->batch.h_kid_states + sizeof(DevState), h->batch.kid_states.p, kStride * upto, hipMemcpyDeviceToHost, h->stream));
            S2M_HIP(h, hipStreamSynchronize(h->stream));
            float t2 = 0.0f;
            S2M_HIP(h, hipEventElapsedTime(&t2, h->reg.ev_a2, h->reg.ev_b2));
            h->reg.t_optimize_ms += t2;
        }
    }
    for (int b = 0; b < n_scans; b++) {
        s2m_context* k = h->batch.kids[(size_t)b];
        const int rc = s2m_optimize_collect(k, poses + 6 * (size_t)b, imu ? imu + b : nullptr, out ? out + b : nullptr);
        if (rc) return fail(h, rc, k->err.c_str());
    }
    return S2M_OK;
}

int s2m_optimize_batch(s2m_handle h, int n_scans, const void* const* scans, const size_t* sizes, size_t stride_bytes,
                       float* poses, const s2m_imu_init* imu, s2m_result* out)
{
    if (!h || n_scans < 1 || n_scans > 64 || !scans || !sizes || !poses) return S2M_ERR_INVALID_ARG;
    int rc = s2m_batch_set_scans(h, n_scans, scans, sizes, stride_bytes, 0);
    if (rc) return rc;
    rc = s2m_optimize_batch_launch(h, n_scans, poses);
    if (rc) return rc;
    return s2m_optimize_batch_collect(h, n_scans, poses, imu, out);
}

int s2m_batch_get_trace(s2m_handle h, int slot, s2m_iter_trace* out, int cap)
{
    if (!h || slot < 0 || slot >= (int)h->batch.kids.size()) return S2M_ERR_INVALID_ARG;
    return s2m_get_trace(h->batch.kids[(size_t)slot], out, cap);
}

int s2m_get_trace(s2m_handle h, s2m_iter_trace* out, int cap)
{
    if (!h || (!out && cap > 0)) return S2M_ERR_INVALID_ARG;
    int n = h->reg.last_trace_n < cap ? h->reg.last_trace_n : cap;
    for (int i = 0; i < n; i++) out[i] = h->reg.last_trace[i];
    return n;
}

int s2m_surf_optimization(s2m_handle h, const float pose[6], int32_t* idx5, float* d2_5, uint8_t* flag, float* coeff4)
{
    if (!h || !pose) return S2M_ERR_INVALID_ARG;
    if (!h->reg.have_scan) return fail(h, S2M_ERR_NO_SCAN, "s2m_set_scan has not been called");
    S2M_HIP(h, hipSetDevice(h->device));
    const size_t n = h->reg.n_q;
    if (n == 0) return S2M_OK;
    if (h->reg.n_m == 0) {          // no map: nothing is ever gated
        if (idx5) for (size_t i = 0; i < 5 * n; i++) idx5[i] = -1;
        if (d2_5) for (size_t i = 0; i < 5 * n; i++) d2_5[i] = INFINITY;
        if (flag) memset(flag, 0, n);
        if (coeff4) memset(coeff4, 0, sizeof(float) * 4 * n);
        return S2M_OK;
    }
    int rc;
    if ((rc = ensure(h, h->reg.dbg_idx5, sizeof(int32_t) * 5 * n))) return rc;
    if ((rc = ensure(h, h->reg.dbg_d2, sizeof(float) * 5 * n))) return rc;
    if ((rc = ensure(h, h->reg.dbg_flag, n))) return rc;
    if ((rc = ensure(h, h->reg.dbg_coeff, sizeof(float) * 4 * n))) return rc;
    h->hctx.dbg_idx5 = h->reg.dbg_idx5.as<int32_t>(); h->hctx.dbg_d2 = h->reg.dbg_d2.as<float>();
    h->hctx.dbg_flag = h->reg.dbg_flag.as<uint8_t>(); h->hctx.dbg_coeff = h->reg.dbg_coeff.as<float>();
    h->ctx_dirty = true;
    if ((rc = upload_ctx(h))) return rc;
    if ((rc = push_state(h, pose))) return rc;
    launch_fused(h, shape_of(h), true, 0, 0);
    S2M_HIP(h, hipGetLastError());
    if (idx5) S2M_HIP(h, hipMemcpyAsync(idx5, h->reg.dbg_idx5.p, sizeof(int32_t) * 5 * n, hipMemcpyDeviceToHost, h->stream));
    if (d2_5) S2M_HIP(h, hipMemcpyAsync(d2_5, h->reg.dbg_d2.p, sizeof(float) * 5 * n, hipMemcpyDeviceToHost, h->stream));
    if (flag) S2M_HIP(h, hipMemcpyAsync(flag, h->reg.dbg_flag.p, n, hipMemcpyDeviceToHost, h->stream));
    if (coeff4) S2M_HIP(h, hipMemcpyAsync(coeff4, h->reg.dbg_coeff.p, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    h->hctx.dbg_idx5 = nullptr; h->hctx.dbg_d2 = nullptr; h->hctx.dbg_flag = nullptr; h->hctx.dbg_coeff = nullptr;
    h->ctx_dirty = true;
    return upload_ctx(h);
}

int s2m_debug_wave_profile(s2m_handle h, const float pose[6], int launches, uint64_t* out, size_t cap_waves)
{
    if (!h || !pose || !out || launches == 0) return S2M_ERR_INVALID_ARG;
    if (!h->reg.have_scan || h->reg.n_m == 0 || h->reg.n_q == 0) return fail(h, S2M_ERR_NO_SCAN, "needs a resident scan and map");
    S2M_HIP(h, hipSetDevice(h->device));
    const size_t nwaves = (size_t)h->hctx.nblocks * (size_t)h->hctx.wpb;   // one record per wave of the grid
    int rc;
    if ((rc = ensure(h, h->reg.dbg_clk, sizeof(uint64_t) * kProfWords * nwaves))) return rc;
    S2M_HIP(h, hipMemsetAsync(h->reg.dbg_clk.p, 0, sizeof(uint64_t) * kProfWords * nwaves, h->stream));
    h->hctx.dbg_clk = h->reg.dbg_clk.as<unsigned long long>();
    h->ctx_dirty = true;
    if ((rc = upload_ctx(h))) return rc;
    if ((rc = push_state(h, pose))) return rc;
    if (launches < 0) {
        // a real loop as enqueue_loop issues it (density re-split, R0 F0 R1 R2' ...); the recorded launch is number
        // N = -launches - 1 (N = 0: the first launch of a scan), closing the iteration before it when the loop is fused
        const LoopShape sh = shape_of(h);
        const int nblocks = h->hctx.nblocks, N = -launches - 1;
        const bool fuse = h->tune.fuse_solve && nblocks <= h->tune.fuse_max_blocks;
        if (h->tune.density_raw > 0) launch_density(h, sh);
        h->hctx.density_pending = 0;                      // cleared on the device by the kernel: keep the host copy in step
        for (int L = 0; L < N; L++) {
            launch_iteration(h, sh, L, (fuse && L >= 2) ? 1 : 0);
            if (!fuse || L == 0) launch_finalize(h, sh, L, 0);
        }
        launch_fused(h, sh, true, N, (fuse && N >= 2) ? 1 : 0);
    }
    for (int rep = 0; rep < launches; rep++)
        launch_fused(h, shape_of(h), true, 0, 0);
    S2M_HIP(h, hipGetLastError());
    const size_t n = nwaves < cap_waves ? nwaves : cap_waves;
    S2M_HIP(h, hipMemcpyAsync(out, h->reg.dbg_clk.p, sizeof(uint64_t) * kProfWords * n, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    h->hctx.dbg_clk = nullptr;
    h->ctx_dirty = true;
    if ((rc = upload_ctx(h))) return rc;
    return (int)n;
}

int s2m_debug_device_trig(s2m_handle h, const float* x, size_t n, float* s, float* c, float* a)
{
    if (!h || (n > 0 && (!x || !s || !c)) || n > (size_t)0x3fffffff) return S2M_ERR_INVALID_ARG;
    if (n == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    int rc = ensure(h, h->voxel.in, sizeof(float) * 4 * n);
    if (rc) return rc;
    float* d = h->voxel.in.as<float>();
    S2M_HIP(h, hipMemcpyAsync(d, x, sizeof(float) * n, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_debug_sincos, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const float*)d, (int)n, d + n, d + 2 * n,
                       a ? d + 3 * n : (float*)nullptr);
    S2M_HIP(h, hipGetLastError());
    S2M_HIP(h, hipMemcpyAsync(s, d + n, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipMemcpyAsync(c, d + 2 * n, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    if (a) S2M_HIP(h, hipMemcpyAsync(a, d + 3 * n, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    return S2M_OK;
}

int s2m_debug_device_hypot(s2m_handle h, const float* x, const float* y, size_t n, float* r)
{
    if (!h || (n > 0 && (!x || !y || !r)) || n > (size_t)0x3fffffff) return S2M_ERR_INVALID_ARG;
    if (n == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    int rc = ensure(h, h->voxel.in, sizeof(float) * 3 * n);
    if (rc) return rc;
    float* d = h->voxel.in.as<float>();
    S2M_HIP(h, hipMemcpyAsync(d, x, sizeof(float) * n, hipMemcpyHostToDevice, h->stream));
    S2M_HIP(h, hipMemcpyAsync(d + n, y, sizeof(float) * n, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_debug_hypot, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const float*)d, (const float*)(d + n), (int)n, d + 2 * n);
    S2M_HIP(h, hipGetLastError());
    S2M_HIP(h, hipMemcpyAsync(r, d + 2 * n, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    return S2M_OK;
}

int s2m_debug_lm_close_check_args(int form, int iter, int max_iter, const double* rows, int n_rows, const float pose0[6],
                                  const float matP_in[36], const s2m_debug_lm_close_out* out)
{
    if (n_rows < 0 || (n_rows > 0 && !rows) || !pose0 || !matP_in || !out) return S2M_ERR_INVALID_ARG;
    if (form != 0 && form != 1) return S2M_ERR_INVALID_ARG;
    if (iter < 0 || iter >= max_iter) return S2M_ERR_INVALID_ARG;
    if (form == 1 && iter == 0) return S2M_ERR_INVALID_ARG;     // launch 1 never closes: iteration 0 needs the degeneracy analysis
    return S2M_OK;
}

int s2m_debug_lm_close(s2m_handle h, int form, int iter, const double* rows, int n_rows, const float pose0[6],
                       int degen_in, const float matP_in[36], s2m_debug_lm_close_out* out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (s2m_debug_lm_close_check_args(form, iter, h->prm.max_iter, rows, n_rows, pose0, matP_in, out))
        return fail(h, S2M_ERR_INVALID_ARG, "null argument, form outside {0, 1}, iter outside 0 .. max_iter-1, or form 1 at iter 0");
    if (h->reg.opt_pending) return fail(h, S2M_ERR_INVALID_ARG, "an optimize launch is pending: collect it first");
    if (!h->reg.have_scan || h->reg.n_m == 0 || h->reg.n_q == 0) return fail(h, S2M_ERR_NO_SCAN, "needs a resident scan and map");
    S2M_HIP(h, hipSetDevice(h->device));
    int rc;
    if ((rc = upload_ctx(h))) return rc;                   // (the parameters of the last s2m_set_params with it)
    // the rows a close reads: one per workgroup the wave table of the resident scan needs (k_finalize, k_register)
    ensure_wave_table(h);
    int32_t n_waves = 0;
    S2M_HIP(h, hipMemcpyAsync(&n_waves, h->reg.n_waves.p, sizeof(n_waves), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    const int nblocks = h->hctx.nblocks, wpb = h->hctx.wpb;
    const int nb_act = std::min((n_waves + wpb - 1) / wpb, nblocks);
    if (n_rows > nb_act) return fail(h, S2M_ERR_INVALID_ARG, "more rows than the resident scan has active workgroups");
    std::vector<double> part((size_t)2 * (size_t)nblocks * kAcc, std::numeric_limits<double>::quiet_NaN());
    double* slot = part.data() + (size_t)(iter & 1) * (size_t)nblocks * kAcc;
    for (size_t k = 0; k < (size_t)nb_act * kAcc; k++) slot[k] = k < (size_t)n_rows * kAcc ? rows[k] : 0.0;
    S2M_HIP(h, hipMemcpyAsync(h->reg.partials.p, part.data(), sizeof(double) * part.size(), hipMemcpyHostToDevice, h->stream));
    DevState s;
    fill_state(h, &s, pose0);
    for (int k = 0; k < 6; k++) { s.pose2[iter & 1][k] = pose0[k]; s.pose2[(iter + 1) & 1][k] = NAN; }
    s.T_valid = 0;
    s.isDegenerate = degen_in;
    memcpy(s.matP, matP_in, sizeof(s.matP));
    hipLaunchKernelGGL(k_set_state, dim3(1), dim3(64), 0, h->stream, h->reg.state.as<DevState>(), s, (const int32_t*)h->reg.n_waves.as<int32_t>(),
                       (unsigned long long*)nullptr);
    S2M_HIP(h, hipMemsetAsync(h->hctx.trace + iter, 0xff, sizeof(s2m_iter_trace), h->stream));
    const LoopShape sh = shape_of(h);
    if (form == 0) launch_finalize(h, sh, iter, 0);
    else           launch_fused(h, sh, false, iter + 1, 1);
    S2M_HIP(h, hipGetLastError());
    S2M_HIP(h, hipMemcpyAsync(&h->reg.h_state[1], h->reg.state.p, sizeof(DevState), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipMemcpyAsync(&h->reg.h_trace[iter], h->hctx.trace + iter, sizeof(s2m_iter_trace), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    const DevState& r = h->reg.h_state[1];
    memcpy(out->AtA, r.AtA, sizeof(out->AtA));
    memcpy(out->AtB, r.AtB, sizeof(out->AtB));
    out->n_sel_last = r.n_sel_last;
    out->trace = h->reg.h_trace[iter];
    memcpy(out->pose, r.pose, 24);
    memcpy(out->pose_next, r.pose2[(iter + 1) & 1], 24);
    out->iters_run = r.iters_run; out->converged = r.converged; out->done = r.done; out->stalled = r.stalled;
    out->is_degenerate = r.isDegenerate;
    out->n_rows_active = nb_act;
    memcpy(out->matP, r.matP, sizeof(out->matP));
    return S2M_OK;
}

int s2m_normal_eq(s2m_handle h, const float pose[6], float AtA[36], float AtB[6], int32_t* n_sel)
{
    if (!h || !pose) return S2M_ERR_INVALID_ARG;
    if (!h->reg.have_scan) return fail(h, S2M_ERR_NO_SCAN, "s2m_set_scan has not been called");
    S2M_HIP(h, hipSetDevice(h->device));
    if (h->reg.n_m == 0 || h->reg.n_q == 0) {
        if (AtA) memset(AtA, 0, sizeof(float) * 36);
        if (AtB) memset(AtB, 0, sizeof(float) * 6);
        if (n_sel) *n_sel = 0;
        return S2M_OK;
    }
    int rc;
    if ((rc = upload_ctx(h))) return rc;
    if ((rc = push_state(h, pose))) return rc;
    {
        const LoopShape sh = shape_of(h);
        launch_fused(h, sh, false, 0, 0);
        launch_finalize(h, sh, 0, 1);
    }
    S2M_HIP(h, hipGetLastError());
    S2M_HIP(h, hipMemcpyAsync(&h->reg.h_state[1], h->reg.state.p, sizeof(DevState), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    if (AtA) memcpy(AtA, h->reg.h_state[1].AtA, sizeof(float) * 36);
    if (AtB) memcpy(AtB, h->reg.h_state[1].AtB, sizeof(float) * 6);
    if (n_sel) *n_sel = h->reg.h_state[1].n_sel_last;
    return S2M_OK;
}

int s2m_debug_scan_prep(s2m_handle h, int32_t chain, const float pose[6], int32_t* qperm, float* qxyz, int32_t* chunk_parts,
                        int32_t* chunk_factor, int32_t* wave_table, int32_t* n_waves)
{
    if (!h || chain < S2M_DEBUG_PREP_READ || chain > S2M_DEBUG_PREP_LEGACY) return S2M_ERR_INVALID_ARG;
    if (h->batch.parent) return fail(h, S2M_ERR_INVALID_ARG, "a scan slot of a batch keeps the six-kernel chain");
    if (h->reg.opt_pending) return fail(h, S2M_ERR_INVALID_ARG, "an optimize launch is pending: collect it first");
    if (!h->reg.have_scan) return fail(h, S2M_ERR_NO_SCAN, "s2m_set_scan has not been called");
    const size_t n = h->reg.n_q;
    if (n == 0) { if (n_waves) *n_waves = 0; return S2M_OK; }
    if (pose && chain != S2M_DEBUG_PREP_READ && h->reg.n_m == 0) return fail(h, S2M_ERR_NO_SCAN, "the density pass needs a map");
    S2M_HIP(h, hipSetDevice(h->device));
    const int n_chunks = h->hctx.n_chunks;
    if (chain != S2M_DEBUG_PREP_READ) {
        const bool legacy = chain == S2M_DEBUG_PREP_LEGACY;
        PrepTable t;
        t.s[0] = h->reg.prep_slot;
        S2M_HIP(h, hipMemsetAsync(h->reg.chunk_factor.p, 0, sizeof(int32_t) * (size_t)(n_chunks + 1), h->stream));
        launch_scan_prep(h->stream, t, 1, !legacy);
        S2M_HIP(h, hipGetLastError());
        h->reg.table_stale = !legacy;
        h->hctx.density_pending = 1;
        h->ctx_dirty = true;
        if (pose) {
            const LoopShape sh = shape_of(h);
            if (legacy) {
                int rc = push_state(h, pose);
                if (rc) return rc;
                hipLaunchKernelGGL(k_wave_density, dim3((sh.table_cap + 3) / 4, 1), dim3(256), 0, h->stream, sh.tbl, h->tune.density_raw);
            } else {
                DensityStateArgs a;
                a.c = h->hctx;
                fill_state(h, &a.v, pose);
                a.cdst = h->reg.dctx.as<DevCtx>(); a.sdst = h->reg.state.as<DevState>();
                a.stamp = nullptr;
                a.raw_limit = h->tune.density_raw;
                hipLaunchKernelGGL(k_wave_density_state, dim3((n_chunks + 3) / 4 + 1), dim3(256), 0, h->stream, a);
                h->ctx_dirty = false;
                h->reg.table_stale = false;
            }
            S2M_HIP(h, hipGetLastError());
            // the wishes before k_chunk_table_density consumes them
            if (chunk_factor) S2M_HIP(h, hipMemcpyAsync(chunk_factor, h->reg.chunk_factor.p, sizeof(int32_t) * (size_t)n_chunks, hipMemcpyDeviceToHost, h->stream));
            hipLaunchKernelGGL(k_chunk_table_density, dim3(1, 1), dim3(1024), 0, h->stream, sh.tbl);
            S2M_HIP(h, hipGetLastError());
            h->hctx.density_pending = 0;                  // cleared on the device by the kernel: keep the host copy in step
        } else if (wave_table || n_waves)
            ensure_wave_table(h);
    }
    if ((!pose || chain == S2M_DEBUG_PREP_READ) && chunk_factor)
        S2M_HIP(h, hipMemcpyAsync(chunk_factor, h->reg.chunk_factor.p, sizeof(int32_t) * (size_t)n_chunks, hipMemcpyDeviceToHost, h->stream));
    if (qperm) S2M_HIP(h, hipMemcpyAsync(qperm, h->reg.qperm.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    if (qxyz) {
        S2M_HIP(h, hipMemcpyAsync(qxyz, h->reg.qx.p, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
        S2M_HIP(h, hipMemcpyAsync(qxyz + n, h->reg.qy.p, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
        S2M_HIP(h, hipMemcpyAsync(qxyz + 2 * n, h->reg.qz.p, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    }
    if (chunk_parts) S2M_HIP(h, hipMemcpyAsync(chunk_parts, h->reg.chunk_parts.p, sizeof(int32_t) * (size_t)n_chunks, hipMemcpyDeviceToHost, h->stream));
    int32_t nw = 0;
    const bool have_table = !h->reg.table_stale;
    if (have_table) S2M_HIP(h, hipMemcpyAsync(&nw, h->reg.n_waves.p, sizeof(nw), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    if (nw < 0 || nw > h->hctx.table_cap) return fail(h, S2M_ERR_HIP, "wave count outside the table");
    if (wave_table && nw > 0) {
        S2M_HIP(h, hipMemcpyAsync(wave_table, h->reg.wave_table.p, sizeof(int2) * (size_t)nw, hipMemcpyDeviceToHost, h->stream));
        S2M_HIP(h, hipStreamSynchronize(h->stream));
    }
    if (n_waves) *n_waves = have_table ? nw : -1;
    return S2M_OK;
}

// Diagnostics: workgroups the certify kernels of the last collected loop handed to the search kernel (0 for a fused loop;
// slot >= 0: that scan slot of the last batch).
int s2m_debug_deferred(s2m_handle h, int slot)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (slot >= 0) { if (slot >= (int)h->batch.kids.size()) return S2M_ERR_INVALID_ARG; h = h->batch.kids[(size_t)slot]; }
    return h->reg.h_state ? h->reg.h_state[1].deferred_total : 0;
}

// set_scan_ms: from the start of the first ordering kernel to the end of the last.  optimize_ms: from the end of the state upload
// of s2m_optimize_launch to the end of the k_finalize that closes the loop (with early exit on: its first range; the second
// range, where one was needed, is added from an event pair of its own).  Both intervals of a single scan are read from
// wall_clock64() stamps the bracketing kernels store in pinned memory - event records around them cost GPU time in every step -
// so optimize_ms no longer includes the idle time between an event's packet and the first kernel behind it.  A batch is still
// timed by an event pair around its graph; set_map_ms by events.  Synchronises if a scan preparation is still to be timed.
int s2m_last_timing(s2m_handle h, float* optimize_ms, float* set_map_ms, float* set_scan_ms)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (h->reg.scan_timing_pending) {
        S2M_HIP(h, hipSetDevice(h->device));
        S2M_HIP(h, hipStreamSynchronize(h->stream));
        h->reg.t_set_scan_ms = stamps_ms(h, kStampPrep0, kStampPrep1);
        h->reg.scan_timing_pending = false;
    }
    if (optimize_ms) *optimize_ms = h->reg.t_optimize_ms;
    if (set_map_ms) *set_map_ms = h->reg.t_set_map_ms;
    if (set_scan_ms) *set_scan_ms = h->reg.t_set_scan_ms;
    return S2M_OK;
}

static int time_iterations_impl(s2m_handle h, const float pose[6], int reps, float* ms_mean, float* ms_per_iter)
{
    if (!h || !pose || reps < 1) return S2M_ERR_INVALID_ARG;
    if (!h->reg.have_scan || h->reg.n_m == 0 || h->reg.n_q == 0) return fail(h, S2M_ERR_NO_SCAN, "needs a resident scan and map");
    S2M_HIP(h, hipSetDevice(h->device));
    int rc;
    if ((rc = upload_ctx(h))) return rc;
    const int nit = h->prm.max_iter;
    if (h->reg.iter_events.size() < (size_t)(2 * nit)) {
        const size_t old = h->reg.iter_events.size();
        h->reg.iter_events.resize(2 * nit);
        for (size_t k = old; k < h->reg.iter_events.size(); k++) S2M_HIP(h, hipEventCreate(&h->reg.iter_events[k]));
    }
    std::vector<double> per_iter((size_t)nit, 0.0);
    for (int rep = 0; rep < reps; rep++) {
        // a new scan starts without a prior or cached planes (what s2m_set_scan leaves behind)
        S2M_HIP(h, hipMemsetAsync(h->reg.cert.p, 0, sizeof(float4) * h->reg.n_q, h->stream));
        S2M_HIP(h, hipMemsetAsync(h->reg.aux.p, 0, sizeof(int4) * h->reg.n_q, h->stream));
        if ((rc = push_state(h, pose))) return rc;
        enqueue_loop(h, shape_of(h), h->reg.iter_events.data());     // the real loop, launched one by one between event pairs
        h->hctx.density_pending = 0;
        S2M_HIP(h, hipGetLastError());
        S2M_HIP(h, hipStreamSynchronize(h->stream));
        for (int it = 0; it < nit; it++) {
            float ms = 0;
            S2M_HIP(h, hipEventElapsedTime(&ms, h->reg.iter_events[2 * it], h->reg.iter_events[2 * it + 1]));
            per_iter[(size_t)it] += ms;
        }
    }
    double total = 0.0;
    for (int it = 0; it < nit; it++) {
        total += per_iter[(size_t)it];
        if (ms_per_iter) ms_per_iter[it] = (float)(per_iter[(size_t)it] / reps);
    }
    if (ms_mean) *ms_mean = (float)(total / ((double)reps * nit));
    return S2M_OK;
}

// Diagnostics: one full loop from `pose` (max_iter iterations, so early_exit should be off), then `reps` back-to-back
// replays of the loop's last registration launch in the state the loop ended in (nearly every point certified):
// solve_prev = 1 closes the iteration before it in its prologue each time (the steady launch of the fused loop),
// 0 rebuilds the transform only.  Returns the mean time per replayed launch, gaps included.
int s2m_debug_time_steady(s2m_handle h, const float pose[6], int reps, int solve_prev, float* us_per_launch)
{
    if (!h || !pose || reps < 1 || !us_per_launch) return S2M_ERR_INVALID_ARG;
    if (!h->reg.have_scan || h->reg.n_m == 0 || h->reg.n_q == 0) return fail(h, S2M_ERR_NO_SCAN, "needs a resident scan and map");
    float p[6];
    memcpy(p, pose, 24);
    s2m_result r;
    int rc = s2m_optimize_resident(h, p, nullptr, &r);
    if (rc) return rc;
    if (r.skipped || r.iters_run != h->prm.max_iter) return fail(h, S2M_ERR_INVALID_ARG, "the loop ended early: switch early_exit off");
    const LoopShape sh = shape_of(h);
    const int L = h->prm.max_iter;
    S2M_HIP(h, hipEventRecord(h->reg.ev_c, h->stream));
    for (int k = 0; k < reps; k++)
        launch_iteration(h, sh, sh.split ? L + (k & 1) : L, solve_prev ? 1 : 0);   // (split: the worklist slots alternate with the launch parity)
    S2M_HIP(h, hipGetLastError());
    S2M_HIP(h, hipEventRecord(h->reg.ev_d, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    float ms = 0;
    S2M_HIP(h, hipEventElapsedTime(&ms, h->reg.ev_c, h->reg.ev_d));
    *us_per_launch = ms * 1e3f / (float)reps;
    return S2M_OK;
}

// Mean duration of a k_register launch over `reps` whole LM loops (max_iter >= 5, fused loop), gaps between the back-to-back
// launches included: HIP events on the handle's stream around launch 0, launch 1, the run of launches 2 .. n-2 and launch n-1.
int s2m_time_loop_launches(s2m_handle h, const float pose[6], int reps, float* us_per_launch)
{
    if (!h || !pose || reps < 1 || !us_per_launch) return S2M_ERR_INVALID_ARG;
    if (!h->reg.have_scan || h->reg.n_m == 0 || h->reg.n_q == 0) return fail(h, S2M_ERR_NO_SCAN, "needs a resident scan and map");
    const int nit = h->prm.max_iter;
    if (nit < 5) return fail(h, S2M_ERR_INVALID_ARG, "needs max_iter >= 5");
    S2M_HIP(h, hipSetDevice(h->device));
    int rc;
    if ((rc = upload_ctx(h))) return rc;
    while (h->reg.iter_events.size() < 8) { hipEvent_t e; S2M_HIP(h, hipEventCreate(&e)); h->reg.iter_events.push_back(e); }
    double total_ms = 0.0;
    for (int rep = 0; rep < reps; rep++) {
        S2M_HIP(h, hipMemsetAsync(h->reg.cert.p, 0, sizeof(float4) * h->reg.n_q, h->stream));      // a new scan: no certificates, no neighbourhoods
        S2M_HIP(h, hipMemsetAsync(h->reg.aux.p, 0, sizeof(int4) * h->reg.n_q, h->stream));
        if ((rc = push_state(h, pose))) return rc;
        enqueue_loop(h, shape_of(h), h->reg.iter_events.data(), true);
        h->hctx.density_pending = 0;
        S2M_HIP(h, hipGetLastError());
        S2M_HIP(h, hipStreamSynchronize(h->stream));
        for (int k = 0; k < 4; k++) {
            float ms = 0;
            S2M_HIP(h, hipEventElapsedTime(&ms, h->reg.iter_events[2 * k], h->reg.iter_events[2 * k + 1]));
            total_ms += ms;
        }
    }
    *us_per_launch = (float)(total_ms * 1e3 / ((double)reps * nit));
    return S2M_OK;
}

int s2m_time_iteration_kernel(s2m_handle h, const float pose[6], int reps, float* ms_per_launch)
{
    if (!ms_per_launch) return S2M_ERR_INVALID_ARG;
    return time_iterations_impl(h, pose, reps, ms_per_launch, nullptr);
}

int s2m_time_iterations(s2m_handle h, const float pose[6], int reps, float* ms_per_iter, int cap)
{
    if (!h || !ms_per_iter || cap < h->prm.max_iter) return S2M_ERR_INVALID_ARG;
    return time_iterations_impl(h, pose, reps, nullptr, ms_per_iter);
}

int s2m_make_scancontext(s2m_handle h, const void* pts, size_t n, size_t stride_bytes,
                         double desc[S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR], double ringkey[S2M_SC_NUM_RING])
{
    int rc = check_records(h, pts, n, stride_bytes);
    if (rc) return rc;
    if (!desc || !ringkey) return S2M_ERR_INVALID_ARG;
    S2M_HIP(h, hipSetDevice(h->device));
    if ((rc = sc_build_descriptor(h, pts, n, stride_bytes))) return rc;
    S2M_HIP(h, hipMemcpyAsync(h->sc.h_stage, h->sc.out.p, sizeof(double) * 1220, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    memcpy(desc, h->sc.h_stage, sizeof(double) * 1200);
    memcpy(ringkey, h->sc.h_stage + 1200, sizeof(double) * 20);
    return S2M_OK;
}

// ---- section 8(f) row F3: the SCManager loop detector ---------------------------------------------

int s2m_sc_reset(s2m_handle h)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    h->sc.n = 0; h->sc.n_search = 0; h->sc.counter = 0;
    return S2M_OK;
}

int s2m_sc_size(s2m_handle h) { return h ? (int)h->sc.n : S2M_ERR_INVALID_ARG; }

int s2m_sc_add_scan(s2m_handle h, const void* pts, size_t n, size_t stride_bytes)
{
    int rc = check_records(h, pts, n, stride_bytes);
    if (rc) return rc;
    S2M_HIP(h, hipSetDevice(h->device));
    if ((rc = sc_build_descriptor(h, pts, n, stride_bytes))) return rc;
    if ((rc = sc_append_from_out(h))) return rc;
    S2M_HIP(h, hipStreamSynchronize(h->stream));          // the caller's cloud is free again
    return S2M_OK;
}

int s2m_sc_add_descriptor(s2m_handle h, const double desc[S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR])
{
    if (!h || !desc) return S2M_ERR_INVALID_ARG;
    S2M_HIP(h, hipSetDevice(h->device));
    // ring key = row means, as makeRingkeyFromScancontext (:198-211) / k_sc_finish compute them
    memcpy(h->sc.h_stage, desc, sizeof(double) * kScDesc);
    for (int r = 0; r < S2M_SC_NUM_RING; r++) {
        double a = 0.0;
        for (int k = 0; k < S2M_SC_NUM_SECTOR; k++) a += desc[r * S2M_SC_NUM_SECTOR + k];
        h->sc.h_stage[kScDesc + r] = a / 60.0;
    }
    S2M_HIP(h, hipMemcpyAsync(h->sc.out.p, h->sc.h_stage, sizeof(double) * 1220, hipMemcpyHostToDevice, h->stream));
    int rc = sc_append_from_out(h);
    if (rc) return rc;
    S2M_HIP(h, hipStreamSynchronize(h->stream));          // h_sc is reused by the next call
    return S2M_OK;
}

int s2m_sc_detect_loop(s2m_handle h, int32_t* loop_id, float* yaw_diff_rad, s2m_sc_match* detail)
{
    if (!h || !loop_id || !yaw_diff_rad) return S2M_ERR_INVALID_ARG;
    *loop_id = -1; *yaw_diff_rad = 0.0f;
    if (detail) { memset(detail, 0, sizeof(*detail)); detail->min_dist = 10000000; }
    constexpr int NUM_EXCLUDE_RECENT = 30, TREE_MAKING_PERIOD = 10;       // Scancontext.h:89, :99
    if ((int)h->sc.n < NUM_EXCLUDE_RECENT + 1) return S2M_OK;              // :263-267
    // the reference rebuilds its kd-tree every TREE_MAKING_PERIOD_ calls; between rebuilds the search sees the older set
    if (h->sc.counter % TREE_MAKING_PERIOD == 0) h->sc.n_search = h->sc.n - NUM_EXCLUDE_RECENT;
    h->sc.counter = h->sc.counter + 1;
    S2M_HIP(h, hipSetDevice(h->device));
    // the kernel writes its 48-byte result straight into the pinned staging block (host-coherent memory the device can address):
    // a copy behind the kernel would be a second trip through the queue, and one to pageable memory ~50 us more
    static_assert(sizeof(ScDetectOut) <= sizeof(double) * 1220, "the result fits the pinned ScanContext staging block");
    hipLaunchKernelGGL(k_sc_detect, dim3(1), dim3(kScThreads), 0, h->stream, (const double*)h->sc.store_desc.as<double>(),
                       (const float*)h->sc.store_ring.as<float>(), (const double*)h->sc.store_sector.as<double>(),
                       (int)h->sc.n, (int)h->sc.n_search, reinterpret_cast<ScDetectOut*>(h->sc.h_stage));
    S2M_HIP(h, hipGetLastError());
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    ScDetectOut o;
    memcpy(&o, h->sc.h_stage, sizeof(o));
    *loop_id = o.loop_id; *yaw_diff_rad = o.yaw_diff_rad;
    if (detail) {
        detail->min_dist = o.min_dist; detail->nn_idx = o.nn_idx; detail->nn_align = o.nn_align;
        for (int k = 0; k < 3; k++) { detail->cand_idx[k] = o.cand_idx[k]; detail->cand_d2[k] = o.cand_d2[k]; }
    }
    return S2M_OK;
}

int s2m_sc_distance(s2m_handle h, int32_t query_idx, const int32_t* cand_idx, int32_t m, double* dist, int32_t* shift)
{
    if (!h || m < 0 || (m > 0 && (!cand_idx || !dist || !shift))) return S2M_ERR_INVALID_ARG;
    if (query_idx < 0 || (size_t)query_idx >= h->sc.n) return fail(h, S2M_ERR_INVALID_ARG, "query index outside the descriptor store");
    for (int32_t k = 0; k < m; k++)
        if (cand_idx[k] < 0 || (size_t)cand_idx[k] >= h->sc.n) return fail(h, S2M_ERR_INVALID_ARG, "candidate index outside the descriptor store");
    if (m == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    const size_t off_d = ((sizeof(int32_t) * (size_t)m + 15) & ~(size_t)15), off_s = off_d + sizeof(double) * (size_t)m;
    int rc = ensure(h, h->sc.cand, off_s + sizeof(int32_t) * (size_t)m);
    if (rc) return rc;
    unsigned char* base = h->sc.cand.as<unsigned char>();
    S2M_HIP(h, hipMemcpyAsync(base, cand_idx, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_sc_distance_batch, dim3((unsigned)m), dim3(kScThreads), 0, h->stream, (const double*)h->sc.store_desc.as<double>(),
                       (const double*)h->sc.store_sector.as<double>(), (int)query_idx, (const int32_t*)base,
                       (double*)(base + off_d), (int32_t*)(base + off_s));
    S2M_HIP(h, hipGetLastError());
    S2M_HIP(h, hipMemcpyAsync(dist, base + off_d, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipMemcpyAsync(shift, base + off_s, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    return S2M_OK;
}

}  // extern "C"
