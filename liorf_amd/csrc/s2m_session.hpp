// s2m_session.hpp — the device side of saving and loading a session (s2m_session.hip): the bulk sections of the blob (the key
// frames' records, the ScanContext descriptors) move between their places on the device and a staging chunk, 16 bytes per lane,
// and the same pass reduces the section's checksum; the keys of loaded descriptors are rebuilt in one launch.  The C ABI on
// top is s2m_abi_session.hip's; DESIGN.md section 19 has the format.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace s2m {

// A section is a run of 32-byte units ("records": a key frame's point, or a quarter of a descriptor row pair - 9600 bytes are
// 300 units) that lie in n_seg segments: segment k holds units [off[k], off[k+1]) of the section at ptr[k]. Empty segments are
// allowed. A workgroup moves kSessTile consecutive units of the chunk it is launched over.
constexpr int kSessUnit = 32;
constexpr int kSessTile = 512;
constexpr int kSessThreads = 256;

// The checksum over a section's 32-bit words w[0..m): s1 = sum w[i], s2 = sum (i + 1) w[i], both mod 2^64. Associative: every
// workgroup leaves the sums of its tile with i counted from the section's start, and the section's checksum is their plain sum.
struct SessSum { unsigned long long s1, s2; };

// The placement of an appended session. A rigid move {R row-major, t} in fp64, passed by value:
// A o X is R' = A_R R, t' = A_R t + A_t, every entry ((a0 b0 + a1 b1) + a2 b2), the translation that sum plus A_t.
struct SessMove { double a[12]; };
// What k_session_place reads and leaves for `count` keys, each array behind the one before, every offset a multiple of 16:
struct SessPlaced {
    size_t count;
    // in:  the stored-pose states (12 fp64 a key) | the estimates (12 fp64) | int32 has-an-estimate
    size_t in_state() const { return 0; }
    size_t in_est() const { return 96 * count; }
    size_t in_has() const { return 192 * count; }
    size_t in_bytes() const { return 196 * count; }
    // out: the composed estimates (fp64 bits) | position records (float4) | cached transforms (12 floats) | float poses (6) |
    //      int32: some result was not finite
    size_t out_est() const { return 0; }
    size_t out_pos() const { return 96 * count; }
    size_t out_T() const { return 112 * count; }
    size_t out_pose() const { return 160 * count; }
    size_t out_bad() const { return (184 * count + 15) & ~(size_t)15; }
    size_t out_bytes() const { return out_bad() + 16; }
};

namespace host __attribute__((visibility("hidden"))) {

inline size_t session_tiles(uint64_t units) { return (size_t)((units + kSessTile - 1) / kSessTile); }

// k_session_gather: units [r0, r1) of the section, r0 < r1, into stage (device, (r1 - r0) * 32 bytes); partial[0 .. tiles) gets
// the tiles' sums. k_session_scatter: the inverse, from stage to the segments.
void session_launch_gather(hipStream_t stream, const unsigned char* const* seg_ptr, const uint64_t* seg_off, int n_seg, uint64_t r0, uint64_t r1,
                           unsigned char* stage, SessSum* partial);
void session_launch_scatter(hipStream_t stream, unsigned char* const* seg_ptr, const uint64_t* seg_off, int n_seg, uint64_t r0, uint64_t r1,
                            const unsigned char* stage, SessSum* partial);
// k_sc_keys_batch: fp32 ring keys and fp64 sector keys of descriptors first .. first+n-1 of the store, one workgroup each
void session_launch_sc_keys(hipStream_t stream, const double* store_desc, float* store_ring, double* store_sector, int first, int n);
// k_session_place: keys 0 .. count-1 of an appended session moved by A (one lane per key). in: count stored-pose states | count
// estimates | count int32 "has an estimate"; out: see SessPlaced. Nothing of the store is touched.
void session_launch_place(hipStream_t stream, const SessMove& A, const unsigned char* in, int count, unsigned char* out);

}  // namespace host
}  // namespace s2m
