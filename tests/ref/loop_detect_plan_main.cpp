// loop_detect_plan_main.cpp — liorf_amd/csrc/s2m_loop_detect_plan.hpp (the argument table and the pass plan of
// s2m_loop_detect_keys: plain host code) built by the host compiler with -fsanitize=address,undefined and walked stand-alone:
// every verdict of a small table, and over a sweep of store sizes, query counts, top_k and pass hooks the plan's invariants -
// at least one query per pass, splits within their bounds, a pass within the scratch bound.  Prints "ok <plans>"; any miss
// prints the case and exits 1.
#include <climits>
#include <cmath>
#include <cstdio>
#include <vector>

#include "s2m_loop_detect_plan.hpp"

using namespace s2m;

static int fails = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); fails++; } } while (0)

int main()
{
    const s2m_loop_detect_params d = ld_defaults();
    EXPECT(d.search_radius == 10.0f && d.time_diff_s == 30.0f && d.first == 0 && d.count == -1 && d.top_k == 1 && d.reserved == 0, "defaults");
    // the argument table: keys at the edges of the store, every field out of range in turn
    const int32_t N = 50;
    std::vector<int32_t> keys{ 0, N - 1, 3, 3 };
    EXPECT(ld_args_ok(N, keys.data(), (int64_t)keys.size(), d), "defaults");
    EXPECT(ld_args_ok(N, nullptr, 0, d) && !ld_args_ok(N, nullptr, 1, d) && !ld_args_ok(N, keys.data(), -1, d), "m and null keys");
    EXPECT(!ld_args_ok(-1, nullptr, 0, d), "n < 0");
    keys[1] = N;
    EXPECT(!ld_args_ok(N, keys.data(), 4, d) && ld_args_ok(N, keys.data(), 1, d), "key N is looked at only within m");
    keys[1] = -1;
    EXPECT(!ld_args_ok(N, keys.data(), 4, d) && ld_args_ok(0, keys.data(), 4, d), "key -1; an empty store looks at no key");
    keys[1] = 1;
    for (int k = -1; k <= S2M_LOOP_MAX_CANDIDATES + 1; k++) {
        s2m_loop_detect_params p = d; p.top_k = k;
        EXPECT(ld_args_ok(N, keys.data(), 4, p) == (k >= 1 && k <= S2M_LOOP_MAX_CANDIDATES), "top_k %d", k);
    }
    struct Range { int32_t first, count; bool ok; };
    for (const Range& r : { Range{ 0, -1, true }, { -1, -1, false }, { N, -1, true }, { N + 1, -1, false }, { 0, -2, false }, { 10, N - 10, true },
                            { 10, N - 9, false }, { 10, INT32_MAX, false }, { INT32_MAX, INT32_MAX, false }, { 5, 0, true } }) {
        s2m_loop_detect_params p = d; p.first = r.first; p.count = r.count;
        EXPECT(ld_args_ok(N, keys.data(), 4, p) == r.ok, "range %d %d", r.first, r.count);
    }
    for (float r : { 0.0f, -1.0f, INFINITY, NAN }) { s2m_loop_detect_params p = d; p.search_radius = r; EXPECT(!ld_args_ok(N, keys.data(), 4, p), "radius %g", r); }
    for (float w : { INFINITY, -INFINITY, NAN }) { s2m_loop_detect_params p = d; p.time_diff_s = w; EXPECT(!ld_args_ok(N, keys.data(), 4, p), "time_diff %g", w); }
    { s2m_loop_detect_params p = d; p.reserved = 1; EXPECT(!ld_args_ok(N, keys.data(), 4, p), "reserved"); }
    { s2m_loop_detect_params p = d; p.exclude_lo = INT32_MIN; p.exclude_hi = INT32_MAX; p.rel_lo = INT32_MIN; p.rel_hi = INT32_MAX;
      EXPECT(ld_args_ok(N, keys.data(), 4, p), "windows of any kind"); }
    // the plan
    long plans = 0;
    for (int64_t n : { (int64_t)1, (int64_t)kLdTile - 1, (int64_t)kLdTile, (int64_t)kLdTile + 1, (int64_t)50000, (int64_t)INT32_MAX })
        for (int64_t m : { (int64_t)1, (int64_t)kLdBlock - 1, (int64_t)kLdBlock, (int64_t)kLdBlock + 1, (int64_t)50000, (int64_t)INT32_MAX })
            for (int k = 1; k <= S2M_LOOP_MAX_CANDIDATES; k++)
                for (int has_time = 0; has_time < 2; has_time++)
                    for (int hook : { 0, 1, 5, kLdBlock + 1, INT_MAX }) {
                        s2m_loop_detect_params p = d; p.top_k = k;
                        const LdPlan pl = ld_plan(n, m, has_time != 0, p, hook);
                        const LdPlan again = ld_plan(n, m, has_time != 0, p, hook);
                        EXPECT(pl.first == 0 && pl.end == n, "range of %lld", (long long)n);
                        EXPECT(pl.pass >= 1 && (int64_t)pl.pass <= m && (hook == 0 || pl.pass <= (size_t)hook), "pass %zu of m %lld hook %d", pl.pass, (long long)m, hook);
                        EXPECT(pl.splits >= 1 && pl.splits <= kLdMaxSplits && pl.splits <= ld_tiles(n), "splits %d of n %lld", pl.splits, (long long)n);
                        EXPECT(pl.per_q == ld_in_bytes(has_time != 0) + ld_part_bytes(pl.splits, k) + ld_out_bytes(k), "per_q");
                        EXPECT(pl.per_q * pl.pass + 64 <= kLdScratchMax, "scratch %zu", pl.per_q * pl.pass);
                        EXPECT(pl.pass == again.pass && pl.splits == again.splits, "the plan depends on the arguments alone");
                        const LdPlan one = ld_plan(n, m, has_time != 0, p, hook, 1), wide = ld_plan(n, m, has_time != 0, p, hook, INT_MAX);
                        EXPECT(one.splits == 1 && one.pass >= pl.pass && wide.splits == pl.splits && wide.pass == pl.pass, "the split hook only lowers the splits");
                        plans++;
                    }
    if (fails) return 1;
    std::printf("ok %ld\n", plans);
    return 0;
}
