// s2m_icp.hpp — ICP loop-closure alignment on the device:
// pcl::IterativeClosestPoint<PointXYZI, PointXYZI> as the reference configures it at
// src/mapOptmization.cpp:571-586 and :663-678.  Implemented in s2m_icp.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstddef>
#include <cstdint>

#include "s2m_icp_close.hpp"
#include "s2m_icp_layout.hpp"    // kIcpMaxSlots, kIcpMaxPairs

namespace s2m {

struct IcpWorkspace;
IcpWorkspace* icp_create();
void          icp_destroy(IcpWorkspace* w);

struct IcpParams { double max_corr_dist; int max_iter; double trans_eps; double fit_eps; };
struct IcpResult { float T[16]; int converged; int iterations; double fitness; };
// no alignment took place (an empty cloud): the identity, not converged, no fitness
inline IcpResult icp_result_none()
{
    IcpResult r{};
    r.T[0] = r.T[5] = r.T[10] = r.T[15] = 1.0f;
    r.fitness = DBL_MAX;
    return r;
}

// src / tgt: device records (x, y, z at byte 0/4/8). Synchronises `stream` once per iteration (the
// close of an iteration, icp_close_step, runs on the host between iterations). Not beside a device loop in flight.
// guess: align(output, guess) - a row-major 4x4 (host) that final_transformation_ starts from, the source moved by it (fp32,
// m0*x + m1*y + m2*z + m3 left to right, k_icp_transform's arithmetic) before the first search; res->T includes it. Null or
// equal to the identity: no guess, the alignment from the identity with the source as it is.
hipError_t icp_align(IcpWorkspace* w, hipStream_t stream, const unsigned char* d_src, size_t n_src,
                     const unsigned char* d_tgt, size_t n_tgt, size_t stride, const IcpParams& prm, IcpResult* res,
                     const float* guess = nullptr);

// ---- the device loop: the same alignment queued on a stream and left alone ------------------------------------------------
// Every iteration is closed on the device (k_icp_close runs icp_close_step, the host loop's own source: s2m_icp_close.hpp), so
// nothing waits between iterations. Iterations are queued in ranges of kIcpRange; a range ends with a copy of the state blocks
// to the host and an event. Once an alignment has ended the remaining launches of its range return at entry.
// icp_align launches the loop's own load, reset, sums and fold kernels on the one-slot layout; only its search (k_icp_nn) and its
// transform (k_icp_transform, the step by value from the host) are kernels of its own.
constexpr int kIcpRange = 8;            // iterations queued at a time
constexpr bool kIcpUseGrid = true;      // the device loop's search: the uniform grid with its brute-force fallback, or brute force only
constexpr float kIcpCellLeaves = 2.0f;  // grid cell edge in units of icp_leaf
constexpr int kIcpShellCap = 3;         // largest Chebyshev radius (cells) searched before a point goes to the brute force
struct IcpTuning { float cell; int shell_cap; int use_grid; };

// What to align: n independent alignments advanced by the same launches through the same kernels, in the form the caller names.
// kSlots: one source (d_src[0], n_src[0]) against n <= kIcpMaxSlots targets, the single alignment its n = 1 case; the slots go to
// every kernel by value and a slot is a grid dimension. kTable: n <= kIcpMaxPairs pairs, pair k with a source of its own
// (d_src[k], n_src[k]); the pairs' descriptions go to the device once, as a table, and a kernel finds its pair by blockIdx.z.
// The two forms launch different instantiations of the kernels, so the form is never chosen from the sizes.
// d_src, d_tgt: device records (x, y, z at byte 0/4/8, `stride` bytes apart). guess: null, or n pointers, each null or a
// row-major 4x4 (host, read before the call that takes the set returns): alignment k's guess as icp_align takes one - every
// alignment owns its moving copy of its source, so they may start at different places.
enum class IcpForm { kSlots, kTable };
struct IcpSet {
    IcpForm                     form;
    int                         n;
    const unsigned char* const* d_src;
    const size_t*               n_src;
    const unsigned char* const* d_tgt;
    const size_t*               n_tgt;
    const float* const*         guess;
    size_t                      stride;
};

void icp_dev_cancel(IcpWorkspace* w);                                    // forget the alignment in flight (the caller has drained the stream)
// Loads the clouds of the set (every size > 0), builds a grid over every target, queues the first range. Does not wait.
// Alignment k gives the bits icp_align gives for its source, its target and its guess alone.
hipError_t icp_dev_begin(IcpWorkspace* w, hipStream_t stream, const IcpSet& set, const IcpParams& prm, const IcpTuning& tune);
// wait == false: tests the event (hipEventQuery) and, where the queued work has ended, queues what follows (the next range, or
// the fitness pass) without waiting for it; wait == true: the same with hipEventSynchronize until the result is there. Ranges are
// queued until every alignment has ended - one that has ended idles meanwhile - then one fitness pass runs for all.
// res: room for res_cap results; a flight of more alignments than that is refused.
// *done: `res` holds the set's n results, res[k] bit for bit what alignment k alone gives, and nothing is in flight any more.
// The sources must stay as they were until then (the fitness pass reloads them).
hipError_t icp_dev_advance(IcpWorkspace* w, hipStream_t stream, bool wait, bool* done, IcpResult* res, int res_cap);
// one nearest-neighbour search of src against tgt, synchronously: mode 0 the host loop's search (k_icp_nn: nn_tiles over every
// source), mode 1 the device loop's search (the grid with its fallback, or with tune.use_grid off k_icp_nn_list over every
// source). keys: host, n_src entries of (fp32 d2 bits << 32 | target index), ~0 = no match. reps > 0: the search `reps`
// times between events (us_search per search; us_build: the grid's construction).
hipError_t icp_dev_nearest(IcpWorkspace* w, hipStream_t stream, const unsigned char* d_src, size_t n_src, const unsigned char* d_tgt,
                           size_t n_tgt, size_t stride, int mode, const IcpTuning& tune, unsigned long long* keys, int* n_fallback,
                           int reps, float* us_build, float* us_search);

// the grids of the device loop over n_slots <= kIcpMaxSlots targets, synchronously: the layout, the target load and the
// preparation of icp_dev_begin (k_icp_begin, box, shape, counts, scan, scatter - built whatever tune.use_grid says), no source and
// no search. info[k]: the slot's IcpGrid as the device holds it (without a grid the targets are not counted: n_fin is 1 where
// one is finite). Each of cell_start / cell_end / order may be null, and so may each of their entries: cell_start[k] and
// cell_end[k] take the n[0] * n[1] * n[2] cell starts and ends of slot k (room for kIcpGridMaxCells), order[k] the original
// index of each of the n_fin entries of the slot's sorted targets (room for n_tgt[k]); nothing is written for a slot without a grid.
constexpr int kIcpGridMaxCells = 1 << 18;
struct IcpGridInfo { float lo[3]; float cell, inv; int n[3]; int n_fin; int usable; };
hipError_t icp_dev_grid(IcpWorkspace* w, hipStream_t stream, const unsigned char* const* d_tgt, const size_t* n_tgt, int n_slots, size_t stride,
                        const IcpTuning& tune, IcpGridInfo* info, int* const* cell_start, int* const* cell_end, int* const* order);

// the close of one iteration on the device, synchronously: n <= kIcpMaxPairs blocks of the table form take sums[17 k ..] and
// the state in[k], k_icp_close runs once over all of them (the loop's own launch), out[k] is the state it left. A state that
// comes in done comes back as it was.
hipError_t icp_dev_close(IcpWorkspace* w, hipStream_t stream, int n, const double* sums, const IcpLoopState* in, const IcpParams& prm,
                         IcpLoopState* out);
// the sums of iteration 0 of a set, synchronously: icp_dev_begin up to and including the preparation, then one search,
// k_icp_sums_dev and k_icp_fold_dev as the first range queues them - no close, no transform. sums: n x 17 folded sums; n_rows[k]:
// the partial rows of alignment k; parts, keys: null, or per alignment null or room for 17 * 256 partial sums (n_rows[k] rows are
// written) and for the n_src keys of the search.
hipError_t icp_dev_sums(IcpWorkspace* w, hipStream_t stream, const IcpSet& set, double max_corr_dist, const IcpTuning& tune, double* sums,
                        int* n_rows, double* const* parts, unsigned long long* const* keys);

}  // namespace s2m
