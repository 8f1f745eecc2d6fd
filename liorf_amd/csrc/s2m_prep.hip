// s2m_prep.hip — what stands in front of the LM loop: the map's uniform-grid index (s2m_set_map) and the scan's locality order
// with its wave table (s2m_set_scan, the scan slots of a batch), built on the device by s2m_prep.hpp's kernels; memory is
// grow-only, sized by the actual point counts.  The C entry points are s2m_abi.hip's; the loop's units reach the scan
// preparation through scan_slot_prepare, launch_scan_prep and ensure_wave_table (s2m_context.hpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <algorithm>
#include <string>

#include "s2m_context.hpp"
#include "s2m_prep.hpp"

using namespace s2m;
using namespace s2m::host;

namespace {

inline uint32_t host_f2ord(float f) { uint32_t u; memcpy(&u, &f, 4); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
inline float host_ord2f(uint32_t o) { uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o; float f; memcpy(&f, &u, 4); return f; }

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

}  // namespace

// s2m_set_scan in three steps, so that the scan slots of a batch share the launches of the middle one:
//   scan_slot_prepare   host side: sizes, buffers, the upload of a host source, the DevCtx fields - and the slot's row of the table
//   launch_scan_prep    the ordering kernels, one grid row per slot (blockIdx.y): six for the slots of a batch, four for a single
//                       scan (the cell scan inside the scatter; the wave table left to the scan's first optimisation)
//   scan_slot_finish    bookkeeping
int s2m::host::scan_slot_prepare(s2m_context* h, const void* pts, size_t n, size_t stride, bool on_device, PrepSlot* ps)
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
void s2m::host::launch_scan_prep(hipStream_t stream, const PrepTable& t, int nslots, bool single, int* issued)
{
    int npb = 0, nb = 0, ncb = 0;
    for (int k = 0; k < nslots; k++) {
        npb = std::max(npb, (int)t.s[k].npb);
        nb = std::max(nb, (t.s[k].n + 255) / 256);
        ncb = std::max(ncb, (t.s[k].n_chunks + 3) / 4);
    }
    if (npb == 0) return;
    if (issued) ++*issued;                                // (a table of empty rows only is not launched, and not counted)
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
    launch_chunk_table(stream, t, nslots);
}

namespace {

// the PrepSlot row of the resident scan, as far as k_chunk_table reads it
void table_slot_of(s2m_context* h, PrepSlot* ps)
{
    memset(ps, 0, sizeof(*ps));
    ps->n = (int32_t)h->reg.n_q; ps->n_chunks = h->hctx.n_chunks; ps->capacity = h->hctx.table_cap;
    ps->chunk_parts = h->reg.chunk_parts.as<int32_t>(); ps->wave_table = h->reg.wave_table.as<int2>(); ps->n_waves = h->reg.n_waves.as<int32_t>();
}

}  // namespace

// The extent-only wave table of a single scan is built on demand: by whatever reads the table or its wave count before the
// scan's first optimisation has emitted the density-aware one (the observation and timing hooks, a handle with the density
// pass switched off).
void s2m::host::ensure_wave_table(s2m_context* h)
{
    if (!h->reg.table_stale) return;
    PrepTable t;
    table_slot_of(h, &t.s[0]);
    launch_chunk_table(h->stream, t, 1);
    h->reg.table_stale = false;
}

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
