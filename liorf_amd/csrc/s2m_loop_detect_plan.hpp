// s2m_loop_detect_plan.hpp — the host-only half of the loop detection by position for many keys: the shape constants of its
// kernels, the argument table of s2m_loop_detect_keys and the plan of its passes.  Plain C++ with no HIP in it, so that a
// stand-alone program can walk the table under a sanitizer; included by s2m_loop_detect.hpp.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "../../include/liorf_s2m.h"

namespace s2m {

constexpr int kLdTile = 128;           // T: stored (position, time) items a workgroup holds in LDS (3 KB)
constexpr int kLdBlock = 64;           // B: queries a workgroup walks past its tiles, one per lane of its one wave
constexpr int kLdMaxSplits = 64;       // store splits (gridDim.y): one partial list per (query, split)
constexpr int kLdTargetGroups = 1024;  // workgroups the grid aims at (4 per CU): few queries take more splits
constexpr size_t kLdScratchMax = (size_t)64 << 20;   // keys and times, lists and rows of one pass: the place queries' bound

// the list a lane keeps holds top_k rounded up to 1, 2, 4 or 8 words
inline int ld_list_words(int top_k) { return top_k <= 1 ? 1 : top_k <= 2 ? 2 : top_k <= 4 ? 4 : 8; }
static_assert(S2M_LOOP_MAX_CANDIDATES <= 8, "a lane's list holds up to 8 words");

inline int ld_tiles(int64_t n_range) { return (int)((n_range + kLdTile - 1) / kLdTile); }
// splits for `queries` queries of one grid against n_range keys: enough to reach kLdTargetGroups workgroups, at most a tile each
inline int ld_splits(int64_t n_range, size_t queries)
{
    const size_t blocks = (queries + kLdBlock - 1) / kLdBlock;
    size_t s = blocks ? (kLdTargetGroups + blocks - 1) / blocks : 1;
    const size_t cap = (size_t)(ld_tiles(n_range) < kLdMaxSplits ? ld_tiles(n_range) : kLdMaxSplits);
    if (s > cap) s = cap;
    return s < 1 ? 1 : (int)s;
}

// bytes of one pass per query, by buffer
inline size_t ld_in_bytes(bool has_time) { return sizeof(int32_t) + (has_time ? sizeof(double) : 0); }                        // key | time_cur
inline size_t ld_part_bytes(int splits, int top_k) { return sizeof(unsigned long long) * (size_t)splits * (size_t)ld_list_words(top_k); }
inline size_t ld_out_bytes(int top_k) { return (sizeof(int32_t) + sizeof(float)) * (size_t)top_k + sizeof(int32_t); }         // key_pre | d2 | n_cand

// historyKeyframeSearchRadius and historyKeyframeSearchTimeDiff as every loop call takes them (s2m_loop_params, s2m_loop_detect_params)
inline bool loop_radius_time_ok(float search_radius, float time_diff_s)
{
    return search_radius > 0.0f && std::isfinite(search_radius) && std::isfinite(time_diff_s);
}

inline s2m_loop_detect_params ld_defaults()
{
    return s2m_loop_detect_params{ 10.0f, 30.0f, 0, -1, 0, 0, 0, 0, 1, 0 };   // include/utility.h:245-246; the whole store, no window, top_k 1
}

// the argument table from the store's size alone.  An empty store holds no key to be outside of: its queries are not looked at
// and every row is empty.
inline bool ld_args_ok(int64_t n, const int32_t* keys, int64_t m, const s2m_loop_detect_params& p)
{
    if (n < 0 || m < 0) return false;
    if (!loop_radius_time_ok(p.search_radius, p.time_diff_s)) return false;
    if (p.top_k < 1 || p.top_k > S2M_LOOP_MAX_CANDIDATES || p.reserved != 0) return false;
    if (p.first < 0 || p.count < -1 || p.first > n) return false;
    if (p.count >= 0 && (int64_t)p.first + p.count > n) return false;
    if (m > 0 && !keys) return false;
    if (n > 0)
        for (int64_t i = 0; i < m; i++)
            if (keys[i] < 0 || (int64_t)keys[i] >= n) return false;
    return true;
}

// The passes of a checked call of m > 0 queries against the range [first, end), first < end: queries per pass, the store splits of
// every pass and the device bytes of a pass per query.  pass_hook: s2m_debug_loop_detect_pass (0: none); split_hook:
// s2m_debug_loop_detect_splits (0: none, else at most this many splits).  A function of the arguments alone.
struct LdPlan {
    int32_t first, end;
    int     splits;
    size_t  pass, per_q;
};
inline LdPlan ld_plan(int64_t n, int64_t m, bool has_time, const s2m_loop_detect_params& p, int pass_hook, int split_hook = 0)
{
    LdPlan pl{};
    pl.first = p.first;
    pl.end = (int32_t)(p.count < 0 ? n : (int64_t)p.first + p.count);
    size_t pass = (size_t)(m > 0 ? m : 1);
    if (pass_hook > 0 && (size_t)pass_hook < pass) pass = (size_t)pass_hook;
    pl.splits = ld_splits((int64_t)pl.end - pl.first, pass);
    if (split_hook > 0 && split_hook < pl.splits) pl.splits = split_hook;
    pl.per_q = ld_in_bytes(has_time) + ld_part_bytes(pl.splits, p.top_k) + ld_out_bytes(p.top_k);
    const size_t fit = (kLdScratchMax - 64) / pl.per_q;   // (64: the times of a pass start on an 8-byte boundary, the rows on a 16-byte one)
    pl.pass = pass < fit ? pass : fit;                    // (per_q <= 4 KB + 112: thousands of queries fit)
    return pl;
}

}  // namespace s2m
