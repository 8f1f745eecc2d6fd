// s2m_icp.hpp — ICP loop-closure alignment on the device:
// pcl::IterativeClosestPoint<PointXYZI, PointXYZI> as the reference configures it at
// src/mapOptmization.cpp:571-586 and :663-678.  Implemented in s2m_icp.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace s2m {

struct IcpWorkspace;
IcpWorkspace* icp_create();
void          icp_destroy(IcpWorkspace* w);

struct IcpParams { double max_corr_dist; int max_iter; double trans_eps; double fit_eps; };
struct IcpResult { float T[16]; int converged; int iterations; double fitness; };

// src / tgt: device records (x, y, z at byte 0/4/8). Synchronises `stream` once per iteration (the
// close of an iteration, icp_close_step, runs on the host between iterations).
hipError_t icp_align(IcpWorkspace* w, hipStream_t stream, const unsigned char* d_src, size_t n_src,
                     const unsigned char* d_tgt, size_t n_tgt, size_t stride, const IcpParams& prm, IcpResult* res);

// ---- the device loop: the same alignment queued on a stream and left alone ------------------------------------------------
// Every iteration is closed on the device (k_icp_close runs icp_close_step, the host loop's own source: s2m_icp_close.hpp), so
// nothing waits between iterations. Iterations are queued in ranges of kIcpRange; a range ends with a copy of the state block
// to the host and an event. Once the alignment has ended the remaining launches of its range return at entry.
constexpr int kIcpRange = 8;            // iterations queued at a time
constexpr bool kIcpUseGrid = true;      // the device loop's search: the uniform grid with its brute-force fallback, or brute force only
constexpr float kIcpCellLeaves = 2.0f;  // grid cell edge in units of icp_leaf
constexpr int kIcpShellCap = 3;         // largest Chebyshev radius (cells) searched before a point goes to the brute force

struct IcpTuning { float cell; int shell_cap; int use_grid; };

void icp_dev_cancel(IcpWorkspace* w);                                    // forget the alignment in flight (the caller has drained the stream)
// loads both clouds, builds the grid over the target, queues the first range. n_src, n_tgt > 0. Does not wait.
hipError_t icp_dev_begin(IcpWorkspace* w, hipStream_t stream, const unsigned char* d_src, size_t n_src, const unsigned char* d_tgt,
                         size_t n_tgt, size_t stride, const IcpParams& prm, const IcpTuning& tune);
// wait == false: tests the event (hipEventQuery) and, where the queued work has ended, queues what follows (the next range, or
// the fitness pass) without waiting for it; wait == true: the same with hipEventSynchronize until the result is there.
// *done: `res` holds the result and nothing is in flight any more. d_src must stay as it was until then (the fitness pass reloads it).
hipError_t icp_dev_advance(IcpWorkspace* w, hipStream_t stream, bool wait, bool* done, IcpResult* res);
// The same for one source against n_slots <= kIcpMaxSlots targets: n_slots independent alignments advance through the same
// launches (the slot is a grid dimension of every kernel of the loop; icp_dev_begin is the one-slot case). Ranges are queued
// until every slot has ended - a slot that has ended idles meanwhile - then one fitness pass runs for all. res: n_slots results,
// res[k] bit for bit what icp_dev_begin / icp_dev_advance give for d_tgt[k] alone. n_tgt[k] > 0.
constexpr int kIcpMaxSlots = 8;
hipError_t icp_dev_begin_many(IcpWorkspace* w, hipStream_t stream, const unsigned char* d_src, size_t n_src, const unsigned char* const* d_tgt,
                              const size_t* n_tgt, int n_slots, size_t stride, const IcpParams& prm, const IcpTuning& tune);
hipError_t icp_dev_advance_many(IcpWorkspace* w, hipStream_t stream, bool wait, bool* done, IcpResult* res);
// one nearest-neighbour search of src against tgt, synchronously: mode 0 k_icp_nn, mode 1 the device loop's search (the grid with its
// fallback, or with tune.use_grid off k_icp_nn_list over every source). keys: host,
// n_src entries of (fp32 d2 bits << 32 | target index), ~0 = no match. reps > 0: the search `reps` times between events
// (us_search per search; us_build: the grid's construction).
hipError_t icp_dev_nearest(IcpWorkspace* w, hipStream_t stream, const unsigned char* d_src, size_t n_src, const unsigned char* d_tgt,
                           size_t n_tgt, size_t stride, int mode, const IcpTuning& tune, unsigned long long* keys, int* n_fallback,
                           int reps, float* us_build, float* us_search);

}  // namespace s2m
