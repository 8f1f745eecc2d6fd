// icp_layout_main.cpp — liorf_amd/csrc/s2m_icp_layout.hpp (where each alignment of an ICP alignment set lies in the workspace's
// buffers, with its rows and slices: plain host code) built by the host compiler with -fsanitize=address,undefined and walked
// stand-alone at the sizes where it can go wrong: every buffer's stretches in order, back to back and ending at the total the
// workspace ensures, the shared form equal to the table form of equal sources, rows and slices within their bounds, the maxima,
// each form's size bound.  Prints "ok <cases>"; any miss prints the case and exits 1.
#include <cstdio>
#include <vector>

#include "s2m_icp_layout.hpp"

using namespace s2m;

static int fails = 0, cases = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); fails++; } } while (0)

// every property of one accepted layout; shared: the sources are n_src[0]
static void check(int n, bool shared, const std::vector<size_t>& n_src, const std::vector<size_t>& n_tgt, const char* what)
{
    IcpLayout L;
    cases++;
    if (!icp_layout(n, shared, n_src.data(), n_tgt.data(), &L)) { EXPECT(false, "%s refused: n %d shared %d", what, n, (int)shared); return; }
    EXPECT(L.n == n, "%s", what);
    size_t so = 0, to = 0, ro = 0;
    int ms = 0, mt = 0, mr = 0, ml = 1;
    for (int k = 0; k < n; k++) {
        const IcpLayoutItem& a = L.at[k];
        const size_t ns = n_src[shared ? 0 : k], nt = n_tgt[k];
        EXPECT((size_t)a.n_src == ns && (size_t)a.n_tgt == nt, "%s: sizes of %d", what, k);
        // in order, disjoint and back to back: a stretch starts where the one before ends
        EXPECT(a.src_off == so && a.tgt_off == to && a.row_off == ro, "%s: alignment %d starts at %zu %zu %zu, not %zu %zu %zu", what, k,
               a.src_off, a.tgt_off, a.row_off, so, to, ro);
        EXPECT(a.rows == (int)((ns + 255) / 256 < (size_t)kSumBlocks ? (ns + 255) / 256 : (size_t)kSumBlocks), "%s: rows %d of %zu sources", what, a.rows, ns);
        EXPECT(a.rows <= kSumBlocks && (a.rows >= 1 || ns == 0), "%s: rows %d", what, a.rows);
        EXPECT(a.slices >= 1, "%s: slices %d", what, a.slices);
        if (ns && nt) {
            EXPECT(a.slice_len > 0 && a.slice_len % kNnTile == 0, "%s: slice_len %d", what, a.slice_len);
            EXPECT((size_t)a.slices * (size_t)a.slice_len >= nt, "%s: %d slices of %d for %zu targets", what, a.slices, a.slice_len, nt);
            EXPECT((size_t)(a.slices - 1) * (size_t)a.slice_len < nt, "%s: the last of %d slices of %d is empty (%zu targets)", what, a.slices, a.slice_len, nt);
        }
        so += ns; to += nt; ro += (size_t)a.rows;
        ms = a.n_src > ms ? a.n_src : ms; mt = a.n_tgt > mt ? a.n_tgt : mt; mr = a.rows > mr ? a.rows : mr; ml = a.slices > ml ? a.slices : ml;
    }
    EXPECT(L.tot_src == so && L.tot_tgt == to && L.tot_rows == ro, "%s: totals %zu %zu %zu, not %zu %zu %zu", what, L.tot_src, L.tot_tgt, L.tot_rows, so, to, ro);
    EXPECT(L.n_src_max == ms && L.n_tgt_max == mt && L.rows_max == mr && L.slices_max == ml, "%s: maxima %d %d %d %d, not %d %d %d %d", what,
           L.n_src_max, L.n_tgt_max, L.rows_max, L.slices_max, ms, mt, mr, ml);
    if (shared && n_src[0] > 0) {                           // the slot form is the table form with every n_src[k] equal
        IcpLayout T;
        const std::vector<size_t> every((size_t)n, n_src[0]);
        if (!icp_layout(n, false, every.data(), n_tgt.data(), &T)) {        // (only the table bounds the sum of the sources)
            EXPECT((size_t)n * n_src[0] > kIcpMaxPoints, "%s: the table form of the same sizes refused", what);
            return;
        }
        bool same = T.n == L.n && T.tot_src == L.tot_src && T.tot_tgt == L.tot_tgt && T.tot_rows == L.tot_rows && T.n_src_max == L.n_src_max &&
                    T.n_tgt_max == L.n_tgt_max && T.rows_max == L.rows_max && T.slices_max == L.slices_max;
        for (int k = 0; k < n; k++) {
            const IcpLayoutItem &a = L.at[k], &b = T.at[k];
            same = same && a.src_off == b.src_off && a.tgt_off == b.tgt_off && a.row_off == b.row_off && a.n_src == b.n_src && a.n_tgt == b.n_tgt &&
                   a.rows == b.rows && a.slices == b.slices && a.slice_len == b.slice_len;
        }
        EXPECT(same, "%s: shared and table differ", what);
    }
}

int main()
{
    const size_t big_src = 256 * (size_t)kSumBlocks + 1, many_tiles = 37 * (size_t)kNnTile + 5;
    const std::vector<size_t> srcs{ 1, 255, 256, 257, big_src };
    const std::vector<size_t> tgts{ 1, (size_t)kNnTile - 1, (size_t)kNnTile, (size_t)kNnTile + 1, many_tiles };
    // every source size against every target size, alone, in 8 slots and in a table of 64
    for (size_t ns : srcs)
        for (size_t nt : tgts) {
            check(1, true, { ns }, { nt }, "one slot");
            check(1, false, { ns }, { nt }, "one pair");
            check(kIcpMaxSlots, true, { ns }, std::vector<size_t>(kIcpMaxSlots, nt), "8 slots");
            check(kIcpMaxPairs, false, std::vector<size_t>(kIcpMaxPairs, ns), std::vector<size_t>(kIcpMaxPairs, nt), "64 pairs");
        }
    // no source (the grid hook): the shared form only, nothing by sources or rows
    for (size_t nt : tgts) { check(1, true, { 0 }, { nt }, "no source"); check(kIcpMaxSlots, true, { 0 }, std::vector<size_t>(kIcpMaxSlots, nt), "no source, 8"); }
    // mixed sizes: the slots' targets, and a table whose sources and targets run through every size out of step
    check(5, true, { 257 }, tgts, "mixed slots");
    std::vector<size_t> ms, mt;
    for (int k = 0; k < kIcpMaxPairs; k++) { ms.push_back(srcs[(size_t)k % srcs.size()]); mt.push_back(tgts[(size_t)(k / 3) % tgts.size()]); }
    check(kIcpMaxPairs, false, ms, mt, "mixed table");
    check(7, false, ms, mt, "mixed table of 7");
    // the number of alignments
    IcpLayout L;
    const std::vector<size_t> ones(kIcpMaxPairs + 1, 1);
    EXPECT(!icp_layout(0, true, ones.data(), ones.data(), &L) && !icp_layout(0, false, ones.data(), ones.data(), &L), "n = 0");
    EXPECT(icp_layout(kIcpMaxSlots, true, ones.data(), ones.data(), &L) && !icp_layout(kIcpMaxSlots + 1, true, ones.data(), ones.data(), &L), "slots");
    EXPECT(icp_layout(kIcpMaxPairs, false, ones.data(), ones.data(), &L) && !icp_layout(kIcpMaxPairs + 1, false, ones.data(), ones.data(), &L), "pairs");
    // each form's bounds, accepted at 0x3fffffff and refused one above. The slots: the source and the sum of the targets
    const size_t top = 0x3fffffff;
    EXPECT(kIcpMaxPoints == top, "the bound");
    check(1, true, { top }, { 1 }, "slots: source at the bound");
    check(kIcpMaxSlots, true, { top }, std::vector<size_t>(kIcpMaxSlots, 1), "8 slots: source at the bound");
    check(2, true, { 1 }, { top - 1, 1 }, "slots: targets sum to the bound");
    size_t one = 1, over = top + 1, two[2] = { top, 1 };
    EXPECT(!icp_layout(1, true, &over, &one, &L), "slots: source over");
    EXPECT(!icp_layout(1, true, &one, &over, &L) && !icp_layout(2, true, &one, two, &L), "slots: targets over");
    // the table: every size, and both sums
    check(1, false, { top }, { top }, "table: both at the bound");
    check(2, false, { top - 1, 1 }, { 1, top - 1 }, "table: sums at the bound");
    size_t a2[2] = { 1, 1 };
    EXPECT(!icp_layout(1, false, &over, &one, &L) && !icp_layout(1, false, &one, &over, &L), "table: a size over");
    EXPECT(!icp_layout(2, false, two, a2, &L) && !icp_layout(2, false, a2, two, &L), "table: a sum over");
    if (fails) return 1;
    std::printf("ok %d\n", cases);
    return 0;
}
