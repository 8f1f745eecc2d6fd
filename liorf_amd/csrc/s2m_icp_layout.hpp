// s2m_icp_layout.hpp — the host-only arithmetic of an ICP alignment set: the shape constants its kernels share with it, the target
// slices of the brute-force search, the partial rows of the sums, and where each alignment's stretch of every buffer starts.
// Plain C++ with no HIP in it, so that a stand-alone program can walk the layout under a sanitizer; included by s2m_icp.hpp.
#pragma once
#include <algorithm>
#include <cstddef>

namespace s2m {

constexpr int kIcpMaxSlots = 8;          // alignments of one shared source, the kernels' arguments by value
constexpr int kIcpMaxPairs = 64;         // alignments of the pair table
constexpr int kNnThreads = 256;
constexpr int kNnTile = 1024;            // target points per LDS tile
constexpr int kSumBlocks = 256;          // most k_icp_sums_dev workgroups: rows of the partial-sum buffer
constexpr size_t kIcpMaxPoints = 0x3fffffff;

// the brute force's grid for n_src sources against n_tgt targets (both > 0): source blocks, target slices, targets per slice
inline void nn_shape(int n_src, int n_tgt, int* sb_out, int* slices_out, int* slice_len_out)
{
    const int sb = (n_src + kNnThreads - 1) / kNnThreads;
    int slices = (1024 + sb - 1) / sb;                                   // ~1000 workgroups in flight
    slices = std::max(1, std::min(slices, (n_tgt + kNnTile - 1) / kNnTile));
    const int slice_len = (((n_tgt + slices - 1) / slices) + kNnTile - 1) / kNnTile * kNnTile;
    *sb_out = sb; *slices_out = (n_tgt + slice_len - 1) / slice_len; *slice_len_out = slice_len;
}

// the partial rows of the sums over n_src sources: a workgroup of 256 per row, at most kSumBlocks
inline int icp_rows(int n_src) { return std::min((n_src + 255) / 256, kSumBlocks); }

// Alignment k of a set: its sizes, its rows and slices - those of the single alignment of its sizes - and where its stretch of
// each buffer starts, in elements: cur, best and list by sources, tgt and gsorted by targets, part by rows (17 doubles a row).
// The blocks and the three cell arrays are laid out by k itself.
struct IcpLayoutItem {
    size_t src_off, tgt_off, row_off;
    int    n_src, n_tgt, rows, slices, slice_len;
};
struct IcpLayout {
    int           n;
    IcpLayoutItem at[kIcpMaxPairs];
    size_t        tot_src, tot_tgt, tot_rows;                            // what the buffers are ensured for
    int           n_src_max, n_tgt_max, rows_max, slices_max;            // what the launches are sized by
};

// The layout of n alignments: every stretch starts where the one before ends. shared: the slot form, n <= kIcpMaxSlots alignments
// of one source of n_src[0] points, each with a moving copy of its own - the table form with every n_src[k] equal; its bound is on
// the source and on the sum of the targets. Otherwise the table form, n <= kIcpMaxPairs with a bound on every size and on both
// sums. An alignment with an empty cloud (the grid hook has no source) has one slice of no length. false: out of bounds.
inline bool icp_layout(int n, bool shared, const size_t* n_src, const size_t* n_tgt, IcpLayout* out)
{
    if (n < 1 || n > (shared ? kIcpMaxSlots : kIcpMaxPairs)) return false;
    IcpLayout L{};
    L.n = n;
    L.slices_max = 1;
    for (int k = 0; k < n; k++) {
        const size_t ns = n_src[shared ? 0 : k], nt = n_tgt[k];
        if (ns > kIcpMaxPoints || nt > kIcpMaxPoints) return false;      // (a target beyond it: so is the sum, the slots' bound)
        IcpLayoutItem& a = L.at[k];
        a.src_off = L.tot_src; a.tgt_off = L.tot_tgt; a.row_off = L.tot_rows;
        a.n_src = (int)ns; a.n_tgt = (int)nt;
        a.rows = icp_rows(a.n_src);
        a.slices = 1;
        int sb = 0;
        if (ns && nt) nn_shape(a.n_src, a.n_tgt, &sb, &a.slices, &a.slice_len);
        L.tot_src += ns; L.tot_tgt += nt; L.tot_rows += (size_t)a.rows;
        if (L.tot_tgt > kIcpMaxPoints || (!shared && L.tot_src > kIcpMaxPoints)) return false;
        L.n_src_max = std::max(L.n_src_max, a.n_src); L.n_tgt_max = std::max(L.n_tgt_max, a.n_tgt);
        L.rows_max = std::max(L.rows_max, a.rows); L.slices_max = std::max(L.slices_max, a.slices);
    }
    *out = L;
    return true;
}

}  // namespace s2m
