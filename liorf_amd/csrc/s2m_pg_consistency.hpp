// s2m_pg_consistency.hpp — the mutually consistent loops among many candidates (s2m_pg_consistent_loops): the integer chain
// length of the estimates, the all-pairs consistency matrix as bit rows, degrees and ranks, the matrix in rank order, a greedy
// growth from every start and the pick of the largest set.  Implemented in s2m_pg_consistency.hip (own translation unit); the
// host part is s2m_abi_pg_consistency.hip; semantics in include/liorf_s2m.h, design in DESIGN.md section 24.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "../../include/liorf_s2m.h"

namespace s2m {

constexpr int kPgcTile = 64;                                   // candidates of a tile: one word of a row, one lane each
constexpr int kPgcMaxWords = S2M_PG_CONSISTENCY_MAX / 64;      // words of a row: lane w of k_pgc_grow holds word w
constexpr int kPgcScanKeys = 1024;                             // keys of one block of the chain-length scan
static_assert(kPgcMaxWords == 64 && S2M_PG_CONSISTENCY_MAX % 64 == 0, "a row of the matrix is at most one word per lane of a wave");

// A candidate as the device holds it: its two keys and Z = (R row-major, t).
struct PgcCand {
    int32_t from, to;
    double  Z[12];
};

struct PgcOut {                                                // k_pgc_pick's record, behind selected[] and degree[] in one block
    int32_t n_candidates, n_selected, start, reserved;
    int64_t n_consistent_pairs;
};
static_assert(sizeof(PgcOut) == sizeof(s2m_pg_consistency_result), "the record is the ABI's");

inline size_t pgc_words(int m) { return (size_t)((m + 63) / 64); }
inline size_t pgc_scan_blocks(int n) { return (size_t)((n + kPgcScanKeys - 1) / kPgcScanKeys); }
// the block of one download: selected (m bytes, padded to 8) | degree (m int32, padded to 8) | PgcOut
inline size_t pgc_deg_off(int m) { return ((size_t)m + 7) & ~(size_t)7; }
inline size_t pgc_rec_off(int m) { return pgc_deg_off(m) + ((sizeof(int32_t) * (size_t)m + 7) & ~(size_t)7); }
inline size_t pgc_out_bytes(int m) { return pgc_rec_off(m) + sizeof(PgcOut); }

struct PgcArgs {
    const double*  X;              // the estimates: [n] x 12
    int            n;              // variables, > 0
    long long*     s;              // [n] chain length, micrometres
    long long*     blk;            // [pgc_scan_blocks(n)]
    const PgcCand* cand;           // [m]
    int            m;              // 1 .. S2M_PG_CONSISTENCY_MAX
    double         tol_m, tol_chord, rate_m, rate_chord;
    unsigned long long* mat;       // [m][pgc_words(m)] in the caller's order
    unsigned long long* mat_rank;  // the same in rank order
    int32_t*       rank;           // [m] rank of candidate p | [m] order: the candidate at rank r | [m] size of the set grown from rank r
    unsigned char* out;            // pgc_out_bytes(m)
};

// Enqueues the kernels of one call on `stream`.
hipError_t pgc_launch(hipStream_t stream, const PgcArgs& a);

}  // namespace s2m
