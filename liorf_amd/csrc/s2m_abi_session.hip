// s2m_abi_session.hip — C ABI of saving and loading a session: the blob's format (restated independently
// in tests/ref/session_ref.py), its checks on the host, and the two streams - device -> pinned chunk -> callback and back -
// around s2m_session.hip's kernels.  The small sections (keys, loop pairs, factors, variables) are built and read here; the
// bulk (records, descriptors) is moved and summed by the device and only handed through.  Behind them the append of a saved
// session to a handle that holds one, its placement by a rigid anchor and the anchor from pose pairs.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "s2m_context.hpp"
#include "s2m_session.hpp"

using namespace s2m;
using namespace s2m::host;

namespace {

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the blob is little-endian and is written from memory as it lies");
static_assert(kPgPrior == S2M_PG_PRIOR && kPgBetween == S2M_PG_BETWEEN && kPgGps == S2M_PG_GPS, "a stored factor's type is the ABI's kind");

constexpr unsigned char kMagic[8] = { 'S', '2', 'M', 'S', 'E', 'S', 'S', 0 };
constexpr size_t kHeaderBytes = 112, kFooterBytes = 112;
enum { kSecKeys, kSecCloud, kSecDesc, kSecLoops, kSecFactors, kSecVars, kSecCount };
constexpr size_t kKeyBytes = 40;                            // 6 x f32 pose, f64 time, i32 point count, u32 zero
constexpr size_t kDescBytes = sizeof(double) * S2M_SC_NUM_RING * S2M_SC_NUM_SECTOR;
constexpr size_t kPairBytes = 8;                            // i32 key_cur, i32 key_pre
constexpr size_t kFactorBytes = 168;                        // i32 type, i, j, rows; f64 R[9], t[3], sw[6], k
constexpr size_t kVarBytes = 96, kInitBytes = 4;            // 12 x f64 per variable, then u32 has_init per variable
constexpr int64_t kMaxCount = (int64_t)1 << 24;             // keys, descriptors, variables (as the stores)
constexpr int64_t kMaxKeyPoints = 0x3fffffff;               // check_records' bound on one cloud
constexpr size_t kChunkDefault = (size_t)16 << 20, kChunkMin = 1024;
static_assert(kDescBytes % kSessUnit == 0, "a descriptor is a whole number of units");

struct Sum { uint64_t s1 = 0, s2 = 0; };
bool operator==(const Sum& a, const Sum& b) { return a.s1 == b.s1 && a.s2 == b.s2; }

// adds words [first, first + bytes / 4) of a section, which lie at p
void sum_words(Sum& s, const void* p, size_t bytes, uint64_t first)
{
    const unsigned char* q = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < bytes / 4; i++) {
        uint32_t w;
        memcpy(&w, q + 4 * i, 4);
        s.s1 += w;
        s.s2 += (first + i + 1) * (uint64_t)w;
    }
}

template <typename T> void put(unsigned char* at, T v) { memcpy(at, &v, sizeof(T)); }
template <typename T> T get(const unsigned char* at) { T v; memcpy(&v, at, sizeof(T)); return v; }

struct Header {
    int32_t n_keys = 0, n_desc = 0, n_search = 0, counter = 0, n_pairs = 0, n_vars = 0, n_factors = 0;
    uint64_t n_points = 0, sec[kSecCount] = { 0 }, total = 0;
};

void sizes_from_counts(Header& hd)
{
    hd.sec[kSecKeys] = kKeyBytes * (uint64_t)hd.n_keys;
    hd.sec[kSecCloud] = kDsStride * hd.n_points;
    hd.sec[kSecDesc] = kDescBytes * (uint64_t)hd.n_desc;
    hd.sec[kSecLoops] = kPairBytes * (uint64_t)hd.n_pairs;
    hd.sec[kSecFactors] = kFactorBytes * (uint64_t)hd.n_factors;
    hd.sec[kSecVars] = (kVarBytes + kInitBytes) * (uint64_t)hd.n_vars;
    hd.total = kHeaderBytes + kFooterBytes;
    for (uint64_t b : hd.sec) hd.total += b;
}

void encode_header(const Header& hd, unsigned char out[kHeaderBytes])
{
    memset(out, 0, kHeaderBytes);
    memcpy(out, kMagic, 8);
    put<uint32_t>(out + 8, S2M_SESSION_VERSION);
    put<uint32_t>(out + 12, (uint32_t)kHeaderBytes);
    const int32_t counts[7] = { hd.n_keys, hd.n_desc, hd.n_search, hd.counter, hd.n_pairs, hd.n_vars, hd.n_factors };
    for (int k = 0; k < 7; k++) put<int32_t>(out + 16 + 4 * k, counts[k]);
    put<uint64_t>(out + 48, hd.n_points);
    for (int k = 0; k < kSecCount; k++) put<uint64_t>(out + 56 + 8 * k, hd.sec[k]);
    put<uint64_t>(out + 104, hd.total);
}

// magic, version and header size: what every other field's meaning rests on
int decode_header(const unsigned char in[kHeaderBytes], Header& hd)
{
    if (memcmp(in, kMagic, 8) != 0 || get<uint32_t>(in + 8) != S2M_SESSION_VERSION || get<uint32_t>(in + 12) != kHeaderBytes) return S2M_ERR_FORMAT;
    int32_t* counts[7] = { &hd.n_keys, &hd.n_desc, &hd.n_search, &hd.counter, &hd.n_pairs, &hd.n_vars, &hd.n_factors };
    for (int k = 0; k < 7; k++) *counts[k] = get<int32_t>(in + 16 + 4 * k);
    hd.n_points = get<uint64_t>(in + 48);
    for (int k = 0; k < kSecCount; k++) hd.sec[k] = get<uint64_t>(in + 56 + 8 * k);
    hd.total = get<uint64_t>(in + 104);
    return S2M_OK;
}

// the counts' ranges, and the section sizes and total that follow from them
int check_counts(const Header& hd)
{
    if (hd.n_keys < 0 || hd.n_keys > kMaxCount || hd.n_desc < 0 || hd.n_desc > kMaxCount || hd.n_vars < 0 || hd.n_vars >= kMaxCount ||
        hd.n_pairs < 0 || hd.n_pairs > hd.n_keys || hd.n_factors < 0 || hd.counter < 0 || hd.n_search < 0 || hd.n_search > hd.n_desc ||
        hd.n_points > (uint64_t)hd.n_keys * (uint64_t)kMaxKeyPoints) return S2M_ERR_FORMAT;
    Header want = hd;
    sizes_from_counts(want);
    for (int k = 0; k < kSecCount; k++) if (want.sec[k] != hd.sec[k]) return S2M_ERR_FORMAT;
    return want.total == hd.total ? S2M_OK : S2M_ERR_FORMAT;
}

void encode_footer(const Sum sums[kSecCount], const unsigned char header[kHeaderBytes], unsigned char out[kFooterBytes])
{
    for (int k = 0; k < kSecCount; k++) { put<uint64_t>(out + 16 * k, sums[k].s1); put<uint64_t>(out + 16 * k + 8, sums[k].s2); }
    Sum hs;                                                 // header, then the footer's section sums, as one run of words
    sum_words(hs, header, kHeaderBytes, 0);
    sum_words(hs, out, 16 * kSecCount, kHeaderBytes / 4);
    put<uint64_t>(out + 16 * kSecCount, hs.s1);
    put<uint64_t>(out + 16 * kSecCount + 8, hs.s2);
}

int check_footer(const unsigned char header[kHeaderBytes], const unsigned char footer[kFooterBytes])
{
    Sum hs;
    sum_words(hs, header, kHeaderBytes, 0);
    sum_words(hs, footer, 16 * kSecCount, kHeaderBytes / 4);
    return hs.s1 == get<uint64_t>(footer + 16 * kSecCount) && hs.s2 == get<uint64_t>(footer + 16 * kSecCount + 8) ? S2M_OK : S2M_ERR_CHECKSUM;
}

Sum footer_sum(const unsigned char footer[kFooterBytes], int k) { return Sum{ get<uint64_t>(footer + 16 * k), get<uint64_t>(footer + 16 * k + 8) }; }

// ---- the content checks, shared by s2m_session_check and s2m_session_load -----------------------------------

int check_keys(const unsigned char* p, const Header& hd)
{
    uint64_t total = 0;
    for (int32_t k = 0; k < hd.n_keys; k++, p += kKeyBytes) {
        for (int a = 0; a < 6; a++) if (!std::isfinite(get<float>(p + 4 * a))) return S2M_ERR_FORMAT;
        if (!std::isfinite(get<double>(p + 24))) return S2M_ERR_FORMAT;
        const int32_t n = get<int32_t>(p + 32);
        if (n < 0 || n > kMaxKeyPoints || get<uint32_t>(p + 36) != 0) return S2M_ERR_FORMAT;
        total += (uint64_t)n;
    }
    return total == hd.n_points ? S2M_OK : S2M_ERR_FORMAT;
}

int check_pairs(const unsigned char* p, const Header& hd)
{
    int64_t last = -1;
    for (int32_t k = 0; k < hd.n_pairs; k++, p += kPairBytes) {
        const int32_t cur = get<int32_t>(p), pre = get<int32_t>(p + 4);
        if (cur <= last || cur >= hd.n_keys || pre < 0 || pre >= hd.n_keys) return S2M_ERR_FORMAT;
        last = cur;
    }
    return S2M_OK;
}

// Field by field, never a copy of the struct: the file survives a change of PgFactor.
void encode_factor(const PgFactor& f, unsigned char* p)
{
    put<int32_t>(p, f.type); put<int32_t>(p + 4, f.i); put<int32_t>(p + 8, f.j); put<int32_t>(p + 12, f.rows);
    for (int a = 0; a < 9; a++) put<double>(p + 16 + 8 * a, f.R[a]);
    for (int a = 0; a < 3; a++) put<double>(p + 88 + 8 * a, f.t[a]);
    for (int a = 0; a < 6; a++) put<double>(p + 112 + 8 * a, f.sw[a]);
    put<double>(p + 160, f.k);
}

PgFactor decode_factor(const unsigned char* p)
{
    PgFactor f{};
    f.type = get<int32_t>(p); f.i = get<int32_t>(p + 4); f.j = get<int32_t>(p + 8); f.rows = get<int32_t>(p + 12);
    for (int a = 0; a < 9; a++) f.R[a] = get<double>(p + 16 + 8 * a);
    for (int a = 0; a < 3; a++) f.t[a] = get<double>(p + 88 + 8 * a);
    for (int a = 0; a < 6; a++) f.sw[a] = get<double>(p + 112 + 8 * a);
    f.k = get<double>(p + 160);
    return f;
}

// The factors and the variables. A factor is put to s2m_pg_check_args as the add call that made it was: its kind, its keys
// against a graph that holds n_vars variables (so the largest key allowed is n_vars - 1), the measurement's translation and
// the row sums of its rotation as the six values (finite exactly when every entry is), the variances 1 / sw^2, and k.
int check_graph(const unsigned char* pf, const unsigned char* pv, const Header& hd)
{
    const size_t n = (size_t)hd.n_vars;
    const unsigned char* init = pv + kVarBytes * n;
    for (size_t k = 0; k < n; k++) {
        if (get<uint32_t>(init + 4 * k) > 1) return S2M_ERR_FORMAT;
        for (int a = 0; a < 12; a++) if (!std::isfinite(get<double>(pv + kVarBytes * k + 8 * a))) return S2M_ERR_FORMAT;
    }
    // the variables the add calls can have made, in this factor order: a key is new only as the next variable, and
    // s2m_pg_set_initial may have made any run of variables with a value in between
    size_t made = 0;
    auto touch = [&](int32_t key) {
        while (made < (size_t)key && made < n && get<uint32_t>(init + 4 * made)) made++;
        if ((size_t)key > made) return false;
        if ((size_t)key == made) made++;
        return true;
    };
    for (int32_t x = 0; x < hd.n_factors; x++) {
        const PgFactor f = decode_factor(pf + kFactorBytes * (size_t)x);
        if (f.type < kPgPrior || f.type > kPgGps || f.rows != (f.type == kPgGps ? 3 : 6) || (f.type != kPgBetween && f.j != -1)) return S2M_ERR_FORMAT;
        float values[6];
        double var[6];
        for (int a = 0; a < 3; a++) {
            values[a] = (float)f.t[a];
            values[3 + a] = (float)((f.R[3 * a] + f.R[3 * a + 1]) + f.R[3 * a + 2]);
            if (!std::isfinite(values[3 + a])) return S2M_ERR_FORMAT;          // (a GPS factor's last three values are not read there)
        }
        for (int a = 0; a < 6; a++) {
            var[a] = (1.0 / f.sw[a]) * (1.0 / f.sw[a]);
            if (a >= f.rows && f.sw[a] != 0.0) return S2M_ERR_FORMAT;
        }
        if (s2m_pg_check_args(f.type, hd.n_vars - 1, f.i, f.j, values, var, f.k) != S2M_OK) return S2M_ERR_FORMAT;
        const int32_t other = f.type == kPgBetween ? f.j : f.i;
        if (!touch(std::min(f.i, other)) || !touch(std::max(f.i, other))) return S2M_ERR_FORMAT;
    }
    while (made < n && get<uint32_t>(init + 4 * made)) made++;
    return made == n ? S2M_OK : S2M_ERR_FORMAT;
}

// ---- what a handle would write -------------------------------------------------------------------------------

Header header_of(const s2m_context* h)
{
    Header hd;
    hd.n_keys = (int32_t)h->kf.time.size();
    hd.n_desc = (int32_t)h->sc.n; hd.n_search = (int32_t)h->sc.n_search; hd.counter = h->sc.counter;
    hd.n_pairs = (int32_t)h->loop.index.size();
    hd.n_vars = (int32_t)h->pg.has_init.size(); hd.n_factors = (int32_t)h->pg.factors.size();
    for (const KfFrame& f : h->kf.frame) hd.n_points += (uint64_t)f.n;
    sizes_from_counts(hd);
    return hd;
}

void info_from(const Header& hd, s2m_session_info* out)
{
    if (!out) return;
    *out = s2m_session_info{ S2M_SESSION_VERSION, hd.n_keys, hd.n_desc, hd.n_pairs, hd.n_vars, hd.n_factors, hd.n_points, hd.total };
}

int session_busy(s2m_context* h)
{
    if (h->loop.pending != s2m_context::LoopClosure::kNone || h->pg.pending)
        return fail(h, S2M_ERR_BUSY, "a launched loop closure or pose-graph optimise is pending: collect it before the session is saved or loaded");
    return S2M_OK;
}

// ---- the two streams around the kernels ----------------------------------------------------------------------

struct Section {                                            // a bulk section as the kernels see it
    std::vector<unsigned char*> ptr;
    std::vector<uint64_t> off{ 0 };
    void push(const unsigned char* p, uint64_t units) { ptr.push_back(const_cast<unsigned char*>(p)); off.push_back(off.back() + units); }
    uint64_t units() const { return off.back(); }
};

struct Pipe {                                               // one section's trip through the staging chunks
    s2m_context* h;
    uint64_t total, chunk;                                  // units, units per chunk
    size_t n_chunks;
    unsigned char* const* d_ptr;
    const uint64_t* d_off;
    int n_seg;
    uint64_t r0(size_t c) const { return chunk * c; }
    uint64_t r1(size_t c) const { return std::min(total, chunk * (c + 1)); }
    size_t bytes(size_t c) const { return (size_t)(r1(c) - r0(c)) * kSessUnit; }
    SessSum* partial(size_t c) const { return h->sess.partial.as<SessSum>() + c * session_tiles(chunk); }
};

void drain(s2m_context* h)
{
    if (h->gmap.copy_stream) (void)hipStreamSynchronize(h->gmap.copy_stream);
    (void)hipStreamSynchronize(h->stream);
}

// table, partials, staging on the device and the pinned chunks for a section
int pipe_open(s2m_context* h, const Section& s, Pipe& p)
{
    const size_t chunk_bytes = h->sess.chunk_bytes ? h->sess.chunk_bytes : kChunkDefault;
    p.h = h; p.total = s.units(); p.chunk = chunk_bytes / kSessUnit;
    p.n_chunks = (size_t)((p.total + p.chunk - 1) / p.chunk);
    p.n_seg = (int)s.ptr.size();
    const size_t ptr_bytes = (sizeof(void*) * s.ptr.size() + 15) & ~(size_t)15;
    int rc;
    if ((rc = ensure(h, h->sess.tab, ptr_bytes + sizeof(uint64_t) * s.off.size())) ||
        (rc = ensure(h, h->sess.partial, sizeof(SessSum) * p.n_chunks * session_tiles(p.chunk)))) return rc;
    const size_t need = (size_t)std::min<uint64_t>(p.total, p.chunk) * kSessUnit;
    for (int k = 0; k < 2 && k < (int)p.n_chunks; k++)
        if ((rc = ensure(h, h->gmap.stage[k], need))) return rc;
    if (h->sess.h_chunk_cap < need) {
        for (unsigned char*& c : h->sess.h_chunk) { if (c) (void)hipHostFree(c); c = nullptr; }
        h->sess.h_chunk_cap = 0;
        for (unsigned char*& c : h->sess.h_chunk) S2M_HIP(h, hipHostMalloc((void**)&c, need));
        h->sess.h_chunk_cap = need;
    }
    if ((rc = copy_pipeline(h))) return rc;
    unsigned char* tab = h->sess.tab.as<unsigned char>();
    S2M_HIP(h, hipMemcpyAsync(tab, s.ptr.data(), sizeof(void*) * s.ptr.size(), hipMemcpyHostToDevice, h->stream));
    S2M_HIP(h, hipMemcpyAsync(tab + ptr_bytes, s.off.data(), sizeof(uint64_t) * s.off.size(), hipMemcpyHostToDevice, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));           // (the section's host table is read by the copies until here)
    p.d_ptr = reinterpret_cast<unsigned char* const*>(tab);
    p.d_off = reinterpret_cast<const uint64_t*>(tab + ptr_bytes);
    return S2M_OK;
}

// the section's checksum: the plain sum of every tile's partial, once the stream has drained
int pipe_sum(const Pipe& p, Sum* out)
{
    s2m_context* h = p.h;
    const size_t last = p.n_chunks - 1;                     // every chunk but the last is full
    const size_t tiles = last * session_tiles(p.chunk) + session_tiles(p.r1(last) - p.r0(last));
    std::vector<SessSum> part(tiles);
    S2M_HIP(h, hipMemcpyAsync(part.data(), h->sess.partial.p, sizeof(SessSum) * tiles, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    for (const SessSum& s : part) { out->s1 += s.s1; out->s2 += s.s2; }
    return S2M_OK;
}

// device -> pinned -> write(): chunk c+1 is gathered and copied while write() has chunk c
template <typename Write> int stream_out(s2m_context* h, const Section& s, Sum* sum, Write write)
{
    if (s.units() == 0) return S2M_OK;
    Pipe p;
    int rc = pipe_open(h, s, p);
    if (rc) return rc;
    auto& g = h->gmap;
    auto issue = [&](size_t c) -> int {
        const int b = (int)(c & 1);
        if (c >= 2) S2M_HIP(h, hipStreamWaitEvent(h->stream, g.ev_cp[b], 0));          // chunk c-2's copy has left the buffer
        session_launch_gather(h->stream, p.d_ptr, p.d_off, p.n_seg, p.r0(c), p.r1(c), g.stage[b].as<unsigned char>(), p.partial(c));
        S2M_HIP(h, hipGetLastError());
        S2M_HIP(h, hipEventRecord(g.ev_xf[b], h->stream));
        S2M_HIP(h, hipStreamWaitEvent(g.copy_stream, g.ev_xf[b], 0));
        S2M_HIP(h, hipMemcpyAsync(h->sess.h_chunk[b], g.stage[b].p, p.bytes(c), hipMemcpyDeviceToHost, g.copy_stream));
        S2M_HIP(h, hipEventRecord(g.ev_cp[b], g.copy_stream));
        return S2M_OK;
    };
    rc = issue(0);
    for (size_t c = 0; c < p.n_chunks && rc == S2M_OK; c++) {
        if (c + 1 < p.n_chunks && (rc = issue(c + 1))) break;
        const hipError_t e = hipEventSynchronize(g.ev_cp[c & 1]);
        if (e != hipSuccess) { rc = fail(h, S2M_ERR_HIP, "session: chunk copy", e); break; }
        rc = write(h->sess.h_chunk[c & 1], p.bytes(c));
    }
    if (rc) { drain(h); return rc; }
    return pipe_sum(p, sum);
}

// read() -> pinned -> device: read() fills chunk c+1 while chunk c is copied up and scattered
template <typename Read> int stream_in(s2m_context* h, const Section& s, Sum* sum, Read read)
{
    if (s.units() == 0) return S2M_OK;
    Pipe p;
    int rc = pipe_open(h, s, p);
    if (rc) return rc;
    auto& g = h->gmap;
    auto step = [&](size_t c) -> int {
        const int b = (int)(c & 1);
        if (c >= 2) S2M_HIP(h, hipEventSynchronize(g.ev_cp[b]));                       // chunk c-2's upload has left the pinned chunk
        const int r = read(h->sess.h_chunk[b], p.bytes(c));
        if (r) return r;
        if (c >= 2) S2M_HIP(h, hipStreamWaitEvent(g.copy_stream, g.ev_xf[b], 0));      // chunk c-2's scatter has left the buffer
        S2M_HIP(h, hipMemcpyAsync(g.stage[b].p, h->sess.h_chunk[b], p.bytes(c), hipMemcpyHostToDevice, g.copy_stream));
        S2M_HIP(h, hipEventRecord(g.ev_cp[b], g.copy_stream));
        S2M_HIP(h, hipStreamWaitEvent(h->stream, g.ev_cp[b], 0));
        session_launch_scatter(h->stream, p.d_ptr, p.d_off, p.n_seg, p.r0(c), p.r1(c), g.stage[b].as<unsigned char>(), p.partial(c));
        S2M_HIP(h, hipGetLastError());
        S2M_HIP(h, hipEventRecord(g.ev_xf[b], h->stream));
        return S2M_OK;
    };
    for (size_t c = 0; c < p.n_chunks && rc == S2M_OK; c++) rc = step(c);
    if (rc) { drain(h); return rc; }
    return pipe_sum(p, sum);
}

// the records of keys first .. of the store
Section cloud_section(const s2m_context* h, size_t first = 0)
{
    Section s;
    for (size_t k = first; k < h->kf.frame.size(); k++) s.push(h->kf.frame[k].src, (uint64_t)h->kf.frame[k].n);
    return s;
}

// descriptors first .. first+n-1 of the store
Section desc_section(const s2m_context* h, size_t n, size_t first = 0)
{
    Section s;
    s.push(h->sc.store_desc.as<unsigned char>() + kDescBytes * first, (uint64_t)n * (kDescBytes / kSessUnit));
    return s;
}

int save_impl(s2m_context* h, s2m_session_write_fn w, void* user)
{
    int rc;
    if ((rc = session_busy(h))) return rc;
    S2M_HIP(h, hipSetDevice(h->device));
    if ((rc = pg_host_current(h))) return rc;              // the estimates a save writes are the newest, as s2m_pg_get_poses reads them
    const Header hd = header_of(h);
    auto write = [&](const void* p, size_t bytes) -> int {
        if (bytes == 0) return S2M_OK;
        return w(user, p, bytes) == 0 ? S2M_OK : fail(h, S2M_ERR_IO, "session save: the write callback failed");
    };
    Sum sums[kSecCount];
    auto host_section = [&](int k, const std::vector<unsigned char>& b) -> int {
        sum_words(sums[k], b.data(), b.size(), 0);
        return write(b.data(), b.size());
    };
    unsigned char header[kHeaderBytes], footer[kFooterBytes];
    encode_header(hd, header);
    if ((rc = write(header, kHeaderBytes))) return rc;

    std::vector<unsigned char> b(hd.sec[kSecKeys], 0);
    for (size_t k = 0; k < (size_t)hd.n_keys; k++) {
        unsigned char* p = b.data() + kKeyBytes * k;
        for (int a = 0; a < 6; a++) put<float>(p + 4 * a, h->kf.pose[6 * k + a]);
        put<double>(p + 24, h->kf.time[k]);
        put<int32_t>(p + 32, h->kf.frame[k].n);
    }
    if ((rc = host_section(kSecKeys, b))) return rc;
    if ((rc = stream_out(h, cloud_section(h), &sums[kSecCloud], write))) return rc;
    if (hd.n_desc > 0 && (rc = stream_out(h, desc_section(h, (size_t)hd.n_desc), &sums[kSecDesc], write))) return rc;

    b.assign(hd.sec[kSecLoops], 0);
    size_t at = 0;
    for (const auto& kv : h->loop.index) {                  // (a std::map: ascending in key_cur)
        put<int32_t>(b.data() + at, kv.first); put<int32_t>(b.data() + at + 4, kv.second);
        at += kPairBytes;
    }
    if ((rc = host_section(kSecLoops, b))) return rc;
    b.assign(hd.sec[kSecFactors], 0);
    for (size_t x = 0; x < h->pg.factors.size(); x++) encode_factor(h->pg.factors[x], b.data() + kFactorBytes * x);
    if ((rc = host_section(kSecFactors, b))) return rc;
    const size_t n = (size_t)hd.n_vars;
    b.assign(hd.sec[kSecVars], 0);
    if (n) memcpy(b.data(), h->pg.X.data(), kVarBytes * n);
    for (size_t k = 0; k < n; k++) put<uint32_t>(b.data() + kVarBytes * n + 4 * k, h->pg.has_init[k] ? 1u : 0u);
    if ((rc = host_section(kSecVars, b))) return rc;

    encode_footer(sums, header, footer);
    return write(footer, kFooterBytes);
}

int load_impl(s2m_context* h, s2m_session_read_fn r, void* user, s2m_session_info* out)
{
    auto read = [&](void* p, size_t bytes) -> int {
        if (bytes == 0) return S2M_OK;
        const int rc = r(user, p, bytes);
        if (rc == 0) return S2M_OK;
        return rc == S2M_ERR_FORMAT ? fail(h, S2M_ERR_FORMAT, "session load: the stream ends early") : fail(h, S2M_ERR_IO, "session load: the read callback failed");
    };
    auto bad = [&](const char* what) { return fail(h, S2M_ERR_FORMAT, what); };
    int rc;
    unsigned char header[kHeaderBytes], footer[kFooterBytes];
    Header hd;
    if ((rc = read(header, kHeaderBytes))) return rc;
    if (decode_header(header, hd)) return bad("session load: not a session of format version 1");
    if (check_counts(hd)) return bad("session load: the header's counts and sizes do not agree");
    Sum sums[kSecCount];
    std::vector<unsigned char> sec[kSecCount];
    auto host_section = [&](int k) -> int {
        sec[k].resize(hd.sec[k]);
        const int e = read(sec[k].data(), sec[k].size());
        if (e == S2M_OK) sum_words(sums[k], sec[k].data(), sec[k].size(), 0);
        return e;
    };
    // key frames: the records go to their places in freshly taken arena blocks
    if ((rc = host_section(kSecKeys))) return rc;
    if (check_keys(sec[kSecKeys].data(), hd)) return bad("session load: key poses, times or point counts");
    {
        const size_t n = (size_t)hd.n_keys;
        std::vector<float> pose(6 * n);
        std::vector<double> time(n);
        std::vector<int32_t> counts(n);
        for (size_t k = 0; k < n; k++) {
            const unsigned char* p = sec[kSecKeys].data() + kKeyBytes * k;
            for (int a = 0; a < 6; a++) pose[6 * k + a] = get<float>(p + 4 * a);
            time[k] = get<double>(p + 24);
            counts[k] = get<int32_t>(p + 32);
        }
        if ((rc = kf_install_keys(h, n, pose.data(), time.data(), counts.data()))) return rc;
    }
    if ((rc = stream_in(h, cloud_section(h), &sums[kSecCloud], read))) return rc;
    // descriptors: straight into the store's array; the store counts them only at the end
    if (hd.n_desc > 0) {
        if ((rc = sc_reserve(h, (size_t)hd.n_desc))) return rc;
        if ((rc = stream_in(h, desc_section(h, (size_t)hd.n_desc), &sums[kSecDesc], read))) return rc;
    }
    if ((rc = host_section(kSecLoops)) || (rc = host_section(kSecFactors)) || (rc = host_section(kSecVars))) return rc;
    if ((rc = read(footer, kFooterBytes))) return rc;
    if (check_footer(header, footer)) return fail(h, S2M_ERR_CHECKSUM, "session load: the header's checksum does not match");
    for (int k = 0; k < kSecCount; k++)
        if (!(sums[k] == footer_sum(footer, k))) return fail(h, S2M_ERR_CHECKSUM, "session load: a section's checksum does not match");
    if (check_pairs(sec[kSecLoops].data(), hd)) return bad("session load: loop pairs");
    if (check_graph(sec[kSecFactors].data(), sec[kSecVars].data(), hd)) return bad("session load: pose-graph factors or variables");

    // everything has arrived and holds: the derived state, then the counts
    if (hd.n_desc > 0) {
        session_launch_sc_keys(h->stream, h->sc.store_desc.as<double>(), h->sc.store_ring.as<float>(), h->sc.store_sector.as<double>(), 0, hd.n_desc);
        S2M_HIP(h, hipGetLastError());
        S2M_HIP(h, hipStreamSynchronize(h->stream));
    }
    h->sc.n = (size_t)hd.n_desc; h->sc.n_search = (size_t)hd.n_search; h->sc.counter = hd.counter;
    for (int32_t k = 0; k < hd.n_pairs; k++) {
        const unsigned char* p = sec[kSecLoops].data() + kPairBytes * (size_t)k;
        h->loop.index[get<int32_t>(p)] = get<int32_t>(p + 4);
    }
    auto& g = h->pg;
    const size_t n = (size_t)hd.n_vars;
    g.factors.resize((size_t)hd.n_factors);
    for (size_t x = 0; x < g.factors.size(); x++) g.factors[x] = decode_factor(sec[kSecFactors].data() + kFactorBytes * x);
    g.X.resize(12 * n);
    if (n) memcpy(g.X.data(), sec[kSecVars].data(), kVarBytes * n);
    g.has_init.resize(n);
    for (size_t k = 0; k < n; k++) g.has_init[k] = (char)get<uint32_t>(sec[kSecVars].data() + kVarBytes * n + 4 * k);
    g.dirty.assign(n, 1);                                   // the next optimise uploads every estimate and builds its tables
    g.dev_newer = false; g.topo_dirty = true; g.n_dev = 0;
    info_from(hd, out);
    return S2M_OK;
}

// ---- appending a session and placing it -------------------------------------------------

// A o X: R' = A_R R, t' = A_R t + A_t, every sum ((a0 b0 + a1 b1) + a2 b2); k_session_place's sess_compose on the host
void compose(const double A[12], const double X[12], double O[12])
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) O[i * 3 + j] = (A[i * 3] * X[j] + A[i * 3 + 1] * X[3 + j]) + A[i * 3 + 2] * X[6 + j];
        O[9 + i] = ((A[i * 3] * X[9] + A[i * 3 + 1] * X[10]) + A[i * 3 + 2] * X[11]) + A[9 + i];
    }
}

// L^-1 o X, summed as s2m_pg_add_odometry sums poseFrom.between(poseTo)
void between_of(const double L[12], const double X[12], double Z[12])
{
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) Z[a * 3 + b] = L[a] * X[b] + L[3 + a] * X[3 + b] + L[6 + a] * X[6 + b];
        Z[9 + a] = L[a] * (X[9] - L[9]) + L[3 + a] * (X[10] - L[10]) + L[6 + a] * (X[11] - L[11]);
    }
}

// X^-1: R^T, -(R^T t)
void inverse_of(const double X[12], double O[12])
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) O[i * 3 + j] = X[j * 3 + i];
        O[9 + i] = -((X[i] * X[9] + X[3 + i] * X[10]) + X[6 + i] * X[11]);
    }
}

// a prior's state or a GPS factor's position under the move A (a between factor is relative: unchanged)
void move_factor(const double A[12], PgFactor& f)
{
    if (f.type == kPgBetween) return;
    double X[12], O[12];
    std::copy(f.R, f.R + 9, X);
    std::copy(f.t, f.t + 3, X + 9);
    compose(A, X, O);
    if (f.type == kPgPrior) std::copy(O, O + 9, f.R);       // (GPS: the rotation block stays the identity it is stored as)
    std::copy(O + 9, O + 12, f.t);
}

bool finite6(const float* p) { for (int a = 0; a < 6; a++) if (!std::isfinite(p[a])) return false; return true; }

// One launch of k_session_place over `count` keys and the one wait for its results: the stored poses at `pose`, key k's estimate
// by est_of(k, X) (false: it has none). back: the staging block on the host, laid out as SessPlaced's out_*. Nothing of the
// store or the graph is touched; a result that is not finite is S2M_ERR_INVALID_ARG.
template <typename EstOf> int place_run(s2m_context* h, const double D[12], size_t count, const float* pose, EstOf est_of, std::vector<unsigned char>& back)
{
    const SessPlaced l{ count };
    std::vector<unsigned char> in(l.in_bytes(), 0);
    for (size_t k = 0; k < count; k++) {
        double S[12], X[12] = { 0 };
        pg_pose_to_state(pose + 6 * k, S);
        const int32_t has = est_of(k, X) ? 1 : 0;
        memcpy(in.data() + l.in_state() + 96 * k, S, 96);
        memcpy(in.data() + l.in_est() + 96 * k, X, 96);
        memcpy(in.data() + l.in_has() + 4 * k, &has, 4);
    }
    back.assign(l.out_bytes(), 0);
    int rc;
    if ((rc = ensure(h, h->sess.place_in, l.in_bytes())) || (rc = ensure(h, h->sess.place_out, l.out_bytes()))) return rc;
    SessMove A;
    std::copy(D, D + 12, A.a);
    unsigned char* out = h->sess.place_out.as<unsigned char>();
    S2M_HIP(h, hipMemcpyAsync(h->sess.place_in.p, in.data(), in.size(), hipMemcpyHostToDevice, h->stream));
    S2M_HIP(h, hipMemsetAsync(out + l.out_bad(), 0, 16, h->stream));
    session_launch_place(h->stream, A, h->sess.place_in.as<unsigned char>(), (int)count, out);
    S2M_HIP(h, hipGetLastError());
    S2M_HIP(h, hipMemcpyAsync(back.data(), out, back.size(), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    int32_t bad;
    memcpy(&bad, back.data() + l.out_bad(), 4);
    if (bad) return fail(h, S2M_ERR_INVALID_ARG, "session place: a moved pose or estimate is not finite; the handle is unchanged");
    return S2M_OK;
}

// the staged poses, positions and transforms of keys first .. first+count-1 into the store: on the device by copies behind the
// kernel on the same stream (no wait), on the host into the mirrors
int place_into_store(s2m_context* h, const std::vector<unsigned char>& back, size_t first, size_t count)
{
    const SessPlaced l{ count };
    const unsigned char* out = h->sess.place_out.as<unsigned char>();
    S2M_HIP(h, hipMemcpyAsync(h->kf.pos.as<float4>() + first, out + l.out_pos(), sizeof(float4) * count, hipMemcpyDeviceToDevice, h->stream));
    static_assert(offsetof(KfFrame, T) == 0, "the cached transform leads a KfFrame");
    S2M_HIP(h, hipMemcpy2DAsync(h->kf.frames.as<KfFrame>() + first, sizeof(KfFrame), out + l.out_T(), sizeof(float) * 12, sizeof(float) * 12, count,
                                hipMemcpyDeviceToDevice, h->stream));
    memcpy(h->kf.pose.data() + 6 * first, back.data() + l.out_pose(), sizeof(float) * 6 * count);
    for (size_t k = 0; k < count; k++) memcpy(h->kf.frame[first + k].T, back.data() + l.out_T() + 48 * k, 48);
    return S2M_OK;
}

PgFactor junction_factor(int32_t n0, const double L[12], const double X[12], const double var[6])
{
    PgFactor f{};
    f.type = kPgBetween; f.i = n0 - 1; f.j = n0; f.rows = 6; f.k = 0.0;
    double Z[12];
    between_of(L, X, Z);
    std::copy(Z, Z + 9, f.R);
    std::copy(Z + 9, Z + 12, f.t);
    for (int a = 0; a < 6; a++) f.sw[a] = 1.0 / std::sqrt(var[a]);
    return f;
}

const double kJunctionVar[6] = { 1.0, 1.0, 1.0, 1.0, 1.0, 1.0 };

int append_impl(s2m_context* h, s2m_session_read_fn r, void* user, const float* anchor, const double* jvar, s2m_session_append_info* out,
                const KfMark& mark)
{
    auto read = [&](void* p, size_t bytes) -> int {
        if (bytes == 0) return S2M_OK;
        const int rc = r(user, p, bytes);
        if (rc == 0) return S2M_OK;
        return rc == S2M_ERR_FORMAT ? fail(h, S2M_ERR_FORMAT, "session append: the stream ends early") : fail(h, S2M_ERR_IO, "session append: the read callback failed");
    };
    auto bad = [&](const char* what) { return fail(h, S2M_ERR_FORMAT, what); };
    int rc;
    unsigned char header[kHeaderBytes], footer[kFooterBytes];
    Header hd;
    if ((rc = read(header, kHeaderBytes))) return rc;
    if (decode_header(header, hd)) return bad("session append: not a session of format version 1");
    if (check_counts(hd)) return bad("session append: the header's counts and sizes do not agree");
    s2m_session_info have, blob;
    info_from(header_of(h), &have);
    info_from(hd, &blob);
    if (s2m_session_append_check_args(&have, &blob, anchor, jvar))
        return fail(h, S2M_ERR_INVALID_ARG, "session append: a handle with keys; at most 2^24 keys in all; with descriptors (variables) in the blob a "
                                            "ScanContext store (pose graph) of exactly as many as the handle has keys and no more of them than the blob has "
                                            "keys; a finite anchor; positive finite variances");
    if ((rc = pg_host_current(h))) return rc;              // the junction is measured from A's newest estimate
    const size_t N0 = mark.n_keys, nK = (size_t)hd.n_keys, nD = (size_t)hd.n_desc, nV = (size_t)hd.n_vars;
    Sum sums[kSecCount];
    std::vector<unsigned char> sec[kSecCount];
    auto host_section = [&](int k) -> int {
        sec[k].resize(hd.sec[k]);
        const int e = read(sec[k].data(), sec[k].size());
        if (e == S2M_OK) sum_words(sums[k], sec[k].data(), sec[k].size(), 0);
        return e;
    };
    // key frames: behind the store's own, the records to arena space taken by s2m_kf_add's rule
    if ((rc = host_section(kSecKeys))) return rc;
    if (check_keys(sec[kSecKeys].data(), hd)) return bad("session append: key poses, times or point counts");
    {
        std::vector<float> pose(6 * nK);
        std::vector<double> time(nK);
        std::vector<int32_t> counts(nK);
        for (size_t k = 0; k < nK; k++) {
            const unsigned char* p = sec[kSecKeys].data() + kKeyBytes * k;
            for (int a = 0; a < 6; a++) pose[6 * k + a] = get<float>(p + 4 * a);
            time[k] = get<double>(p + 24);
            counts[k] = get<int32_t>(p + 32);
        }
        if ((rc = kf_install_keys(h, nK, pose.data(), time.data(), counts.data()))) return rc;
    }
    if ((rc = stream_in(h, cloud_section(h, N0), &sums[kSecCloud], read))) return rc;
    // descriptors: behind the store's own; the store counts them only at the end
    if (nD > 0) {
        if ((rc = sc_reserve(h, N0 + nD))) return rc;
        if ((rc = stream_in(h, desc_section(h, nD, N0), &sums[kSecDesc], read))) return rc;
    }
    if ((rc = host_section(kSecLoops)) || (rc = host_section(kSecFactors)) || (rc = host_section(kSecVars))) return rc;
    if ((rc = read(footer, kFooterBytes))) return rc;
    if (check_footer(header, footer)) return fail(h, S2M_ERR_CHECKSUM, "session append: the header's checksum does not match");
    for (int k = 0; k < kSecCount; k++)
        if (!(sums[k] == footer_sum(footer, k))) return fail(h, S2M_ERR_CHECKSUM, "session append: a section's checksum does not match");
    if (check_pairs(sec[kSecLoops].data(), hd)) return bad("session append: loop pairs");
    if (check_graph(sec[kSecFactors].data(), sec[kSecVars].data(), hd)) return bad("session append: pose-graph factors or variables");
    const unsigned char* vars = sec[kSecVars].data();
    auto has_value = [&](size_t k) { return k < nV && get<uint32_t>(vars + kVarBytes * nV + 4 * k) != 0; };
    if (nV > 0 && (!has_value(0) || !h->pg.has_init[N0 - 1]))
        return fail(h, S2M_ERR_INVALID_ARG, "session append: the junction needs a value of the handle's last variable and of the blob's first");

    // everything has arrived and holds: the derived state, the placement, then - host only - the graph, the pairs and the counts
    if (nD > 0) {
        session_launch_sc_keys(h->stream, h->sc.store_desc.as<double>(), h->sc.store_ring.as<float>(), h->sc.store_sector.as<double>(), (int)N0, (int)nD);
        S2M_HIP(h, hipGetLastError());
        S2M_HIP(h, hipStreamSynchronize(h->stream));
    }
    std::vector<double> X(12 * nV);
    if (nV) memcpy(X.data(), vars, kVarBytes * nV);
    double A[12];
    if (anchor && nK > 0) {
        pg_pose_to_state(anchor, A);
        std::vector<unsigned char> back;
        auto est_of = [&](size_t k, double* o) { if (!has_value(k)) return false; std::copy(X.begin() + 12 * k, X.begin() + 12 * (k + 1), o); return true; };
        if ((rc = place_run(h, A, nK, h->kf.pose.data() + 6 * N0, est_of, back))) return rc;
        if ((rc = place_into_store(h, back, N0, nK))) return rc;
        const SessPlaced l{ nK };
        for (size_t k = 0; k < nV; k++) if (has_value(k)) memcpy(X.data() + 12 * k, back.data() + l.out_est() + 96 * k, 96);
    }
    auto& g = h->pg;
    const size_t nF = (size_t)hd.n_factors;
    g.factors.reserve(g.factors.size() + nF + 1);           // (nothing below throws: the containers end whole)
    g.X.reserve(g.X.size() + 12 * nV); g.has_init.reserve(N0 + nV); g.dirty.reserve(N0 + nV);
    int32_t junction = -1;
    if (nV > 0) {
        junction = (int32_t)g.factors.size();
        g.factors.push_back(junction_factor((int32_t)N0, g.X.data() + 12 * (N0 - 1), X.data(), jvar ? jvar : kJunctionVar));
        for (size_t x = 0; x < nF; x++) {
            PgFactor f = decode_factor(sec[kSecFactors].data() + kFactorBytes * x);
            f.i += (int32_t)N0;
            if (f.type == kPgBetween) f.j += (int32_t)N0;
            if (anchor) move_factor(A, f);
            g.factors.push_back(f);
        }
        g.X.insert(g.X.end(), X.begin(), X.end());
        for (size_t k = 0; k < nV; k++) { g.has_init.push_back(has_value(k) ? 1 : 0); g.dirty.push_back(1); }
        g.topo_dirty = true;
    }
    for (int32_t k = 0; k < hd.n_pairs; k++) {
        const unsigned char* p = sec[kSecLoops].data() + kPairBytes * (size_t)k;
        h->loop.index[get<int32_t>(p) + (int32_t)N0] = get<int32_t>(p + 4) + (int32_t)N0;
    }
    h->sc.n += nD;
    h->sess.app_first = (int32_t)N0; h->sess.app_count = (int32_t)nK; h->sess.app_junction = junction;
    if (out) { out->blob = blob; out->first_key = (int32_t)N0; out->junction_factor = junction; }
    return S2M_OK;
}

int place_impl(s2m_context* h, const float move[6])
{
    int rc;
    if ((rc = pg_host_current(h))) return rc;
    auto& g = h->pg;
    const size_t first = (size_t)h->sess.app_first, count = (size_t)h->sess.app_count;
    if (count == 0) return S2M_OK;
    double D[12];
    pg_pose_to_state(move, D);
    auto has_value = [&](size_t k) { return first + k < g.has_init.size() && g.has_init[first + k]; };
    auto est_of = [&](size_t k, double* o) { if (!has_value(k)) return false; std::copy(g.X.begin() + 12 * (first + k), g.X.begin() + 12 * (first + k + 1), o); return true; };
    std::vector<unsigned char> back;
    if ((rc = place_run(h, D, count, h->kf.pose.data() + 6 * first, est_of, back))) return rc;
    if ((rc = place_into_store(h, back, first, count))) return rc;
    const SessPlaced l{ count };
    for (size_t k = 0; k < count; k++) {
        if (!has_value(k)) continue;
        memcpy(g.X.data() + 12 * (first + k), back.data() + l.out_est() + 96 * k, 96);
        g.dirty[first + k] = 1;
    }
    for (PgFactor& f : g.factors)
        if (f.type != kPgBetween && (size_t)f.i >= first && (size_t)f.i < first + count) move_factor(D, f);
    const int32_t j = h->sess.app_junction;
    if (j >= 0 && (size_t)j < g.factors.size()) {          // measured again, at the new estimates; its variances stay
        PgFactor& f = g.factors[(size_t)j];
        double Z[12];
        between_of(g.X.data() + 12 * (first - 1), g.X.data() + 12 * first, Z);
        std::copy(Z, Z + 9, f.R);
        std::copy(Z + 9, Z + 12, f.t);
    }
    g.topo_dirty = true;
    return S2M_OK;
}

struct FileUser { FILE* f; };

int file_write(void* user, const void* data, size_t bytes) { return fwrite(data, 1, bytes, static_cast<FileUser*>(user)->f) == bytes ? 0 : -1; }

int file_read(void* user, void* data, size_t bytes)
{
    FILE* f = static_cast<FileUser*>(user)->f;
    if (fread(data, 1, bytes, f) == bytes) return 0;
    return feof(f) ? S2M_ERR_FORMAT : -1;
}

}  // namespace

int s2m_session_info_of(s2m_handle h, s2m_session_info* out)
{
    if (!h || !out) return S2M_ERR_INVALID_ARG;
    info_from(header_of(h), out);
    return S2M_OK;
}

int s2m_session_save(s2m_handle h, s2m_session_write_fn w, void* user)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!w) return fail(h, S2M_ERR_INVALID_ARG, "session save: null write callback");
    try {
        return save_impl(h, w, user);
    } catch (const std::bad_alloc&) {                       // (no exception crosses the boundary)
        drain(h);
        return fail(h, S2M_ERR_CAPACITY, "session save: out of host memory");
    }
}

int s2m_session_load(s2m_handle h, s2m_session_read_fn r, void* user, s2m_session_info* out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!r) return fail(h, S2M_ERR_INVALID_ARG, "session load: null read callback");
    int rc = session_busy(h);
    if (rc) return rc;
    if (!h->kf.time.empty() || !h->kf.blocks.empty() || h->sc.n != 0 || !h->loop.index.empty() || !h->pg.has_init.empty() || !h->pg.factors.empty())
        return fail(h, S2M_ERR_INVALID_ARG, "session load: the key-frame store, the ScanContext store, the loop container and the pose graph must be "
                                            "empty: s2m_kf_reset, s2m_sc_reset and s2m_pg_reset first");
    S2M_HIP(h, hipSetDevice(h->device));
    h->sess.forget_appended();
    try {
        rc = load_impl(h, r, user, out);
    } catch (const std::bad_alloc&) {                       // (a header that asks for more than the host has)
        rc = fail(h, S2M_ERR_CAPACITY, "session load: out of host memory");
    }
    if (rc) {                                               // never half filled: whatever arrived goes again
        const std::string why = h->err;
        drain(h);
        (void)s2m_kf_reset(h);
        (void)s2m_sc_reset(h);
        (void)s2m_pg_reset(h);
        h->err = why;
    }
    return rc;
}

int s2m_session_save_file(s2m_handle h, const char* path)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!path) return fail(h, S2M_ERR_INVALID_ARG, "session save: null path");
    FileUser u{ fopen(path, "wb") };
    if (!u.f) return fail(h, S2M_ERR_IO, "session save: the file cannot be opened for writing");
    int rc = s2m_session_save(h, file_write, &u);
    if (fclose(u.f) != 0 && rc == S2M_OK) rc = fail(h, S2M_ERR_IO, "session save: closing the file failed");
    return rc;
}

int s2m_session_load_file(s2m_handle h, const char* path, s2m_session_info* out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!path) return fail(h, S2M_ERR_INVALID_ARG, "session load: null path");
    FileUser u{ fopen(path, "rb") };
    if (!u.f) return fail(h, S2M_ERR_IO, "session load: the file cannot be opened");
    const int rc = s2m_session_load(h, file_read, &u, out);
    (void)fclose(u.f);
    return rc;
}

int s2m_session_append_check_args(const s2m_session_info* have, const s2m_session_info* blob_info, const float* anchor_xyzrpy, const double* junction_var)
{
    if (!have || !blob_info) return S2M_ERR_INVALID_ARG;
    const int64_t n0 = have->n_keys, nk = blob_info->n_keys;
    if (n0 < 1 || nk < 0 || n0 + nk > kMaxCount) return S2M_ERR_INVALID_ARG;
    if (blob_info->n_descriptors < 0 || blob_info->n_variables < 0) return S2M_ERR_INVALID_ARG;
    if (blob_info->n_descriptors > 0 && (have->n_descriptors != n0 || blob_info->n_descriptors > nk)) return S2M_ERR_INVALID_ARG;
    if (blob_info->n_variables > 0 && (have->n_variables != n0 || blob_info->n_variables > nk)) return S2M_ERR_INVALID_ARG;
    if (anchor_xyzrpy && !finite6(anchor_xyzrpy)) return S2M_ERR_INVALID_ARG;
    if (junction_var)
        for (int a = 0; a < 6; a++) if (!(junction_var[a] > 0.0) || !std::isfinite(junction_var[a])) return S2M_ERR_INVALID_ARG;
    return S2M_OK;
}

int s2m_session_append(s2m_handle h, s2m_session_read_fn r, void* user, const float* anchor_xyzrpy, const double* junction_var,
                       s2m_session_append_info* info_out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!r) return fail(h, S2M_ERR_INVALID_ARG, "session append: null read callback");
    int rc = session_busy(h);
    if (rc) return rc;
    S2M_HIP(h, hipSetDevice(h->device));
    const KfMark mark = kf_mark(h);
    try {
        rc = append_impl(h, r, user, anchor_xyzrpy, junction_var, info_out, mark);
    } catch (const std::bad_alloc&) {                       // (a header that asks for more than the host has)
        rc = fail(h, S2M_ERR_CAPACITY, "session append: out of host memory");
    }
    if (rc) {                                               // as before the call: the graph, the pairs and the counts were not reached
        drain(h);
        kf_truncate(h, mark);
    }
    return rc;
}

int s2m_session_append_file(s2m_handle h, const char* path, const float* anchor_xyzrpy, const double* junction_var, s2m_session_append_info* info_out)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!path) return fail(h, S2M_ERR_INVALID_ARG, "session append: null path");
    FileUser u{ fopen(path, "rb") };
    if (!u.f) return fail(h, S2M_ERR_IO, "session append: the file cannot be opened");
    const int rc = s2m_session_append(h, file_read, &u, anchor_xyzrpy, junction_var, info_out);
    (void)fclose(u.f);
    return rc;
}

int s2m_session_place(s2m_handle h, const float move_xyzrpy[6])
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (!move_xyzrpy || !finite6(move_xyzrpy)) return fail(h, S2M_ERR_INVALID_ARG, "session place: the move must be finite");
    if (h->sess.app_first < 0) return fail(h, S2M_ERR_INVALID_ARG, "session place: no appended session (s2m_session_append first)");
    int rc = session_busy(h);
    if (rc) return rc;
    S2M_HIP(h, hipSetDevice(h->device));
    try {
        return place_impl(h, move_xyzrpy);
    } catch (const std::bad_alloc&) {
        drain(h);
        return fail(h, S2M_ERR_CAPACITY, "session place: out of host memory");
    }
}

int s2m_session_appended(s2m_handle h, int32_t* first, int32_t* count)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (first) *first = h->sess.app_first;
    if (count) *count = h->sess.app_count;
    return S2M_OK;
}

int s2m_session_anchor_from_pairs(const float* pose_in_session, const float* pose_in_map, int32_t m, double tol_m, double tol_rad,
                                  float anchor_out[6], int32_t* n_inliers, int32_t* chosen)
{
    if (!pose_in_session || !pose_in_map || !anchor_out || m <= 0 || !(tol_m >= 0.0) || !std::isfinite(tol_m) || !(tol_rad >= 0.0) ||
        !std::isfinite(tol_rad)) return S2M_ERR_INVALID_ARG;
    for (int32_t i = 0; i < m; i++)
        if (!finite6(pose_in_session + 6 * (size_t)i) || !finite6(pose_in_map + 6 * (size_t)i)) return S2M_ERR_INVALID_ARG;
    try {
        std::vector<double> A(12 * (size_t)m);
        for (int32_t i = 0; i < m; i++) {                   // A_i = state(map_i) o state(session_i)^-1
            double S[12], M[12], Si[12];
            pg_pose_to_state(pose_in_session + 6 * (size_t)i, S);
            pg_pose_to_state(pose_in_map + 6 * (size_t)i, M);
            inverse_of(S, Si);
            compose(M, Si, A.data() + 12 * (size_t)i);
        }
        int32_t best = -1, best_n = 0;
        double best_sum = 0.0;
        for (int32_t i = 0; i < m; i++) {
            const double* a = A.data() + 12 * (size_t)i;
            int32_t n = 0;
            double sum = 0.0;
            for (int32_t j = 0; j < m; j++) {
                const double* b = A.data() + 12 * (size_t)j;
                const double dx = a[9] - b[9], dy = a[10] - b[10], dz = a[11] - b[11];
                const double dist = std::sqrt((dx * dx + dy * dy) + dz * dz);
                double tr = 0.0;
                for (int k = 0; k < 9; k++) tr += a[k] * b[k];                 // trace(A_i.R^T A_j.R), entry by entry, left to right
                const double ang = std::acos(std::min(1.0, std::max(-1.0, (tr - 1.0) / 2.0)));
                if (dist <= tol_m && ang <= tol_rad) { n++; sum += dist; }
            }
            if (best < 0 || n > best_n || (n == best_n && sum < best_sum)) { best = i; best_n = n; best_sum = sum; }
        }
        const double* P = A.data() + 12 * (size_t)best;     // k_pg_poses' read-out, with the host's libm
        const double s = std::fmin(1.0, std::fmax(-1.0, -P[6]));
        anchor_out[0] = (float)P[9]; anchor_out[1] = (float)P[10]; anchor_out[2] = (float)P[11];
        anchor_out[3] = (float)std::atan2(P[7], P[8]);
        anchor_out[4] = (float)std::asin(s);
        anchor_out[5] = (float)std::atan2(P[3], P[0]);
        if (n_inliers) *n_inliers = best_n;
        if (chosen) *chosen = best;
    } catch (const std::bad_alloc&) {
        return S2M_ERR_CAPACITY;
    }
    return S2M_OK;
}

int s2m_session_check(const void* blob, size_t bytes, s2m_session_info* out)
{
    if (!blob) return S2M_ERR_INVALID_ARG;
    const unsigned char* p = static_cast<const unsigned char*>(blob);
    Header hd;
    // the structure: what locates everything else
    if (bytes < kHeaderBytes + kFooterBytes || decode_header(p, hd) || hd.total != bytes) return S2M_ERR_FORMAT;
    const unsigned char* footer = p + bytes - kFooterBytes;
    if (check_footer(p, footer)) return S2M_ERR_CHECKSUM;
    uint64_t body = 0;
    for (uint64_t b : hd.sec) { if (b % 4 != 0 || b > bytes) return S2M_ERR_FORMAT; body += b; }
    if (body != bytes - kHeaderBytes - kFooterBytes) return S2M_ERR_FORMAT;
    const unsigned char* sec[kSecCount];
    const unsigned char* at = p + kHeaderBytes;
    for (int k = 0; k < kSecCount; k++) {
        sec[k] = at;
        Sum s;
        sum_words(s, at, (size_t)hd.sec[k], 0);
        if (!(s == footer_sum(footer, k))) return S2M_ERR_CHECKSUM;
        at += hd.sec[k];
    }
    // the content
    if (check_counts(hd) || check_keys(sec[kSecKeys], hd) || check_pairs(sec[kSecLoops], hd) || check_graph(sec[kSecFactors], sec[kSecVars], hd))
        return S2M_ERR_FORMAT;
    info_from(hd, out);
    return S2M_OK;
}

// ---- test hooks (include/liorf_s2m_debug.h) ---------------------------------------------------------------------

int s2m_debug_session_chunk(s2m_handle h, size_t chunk_bytes)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (chunk_bytes != 0 && (chunk_bytes < kChunkMin || chunk_bytes % kSessUnit != 0))
        return fail(h, S2M_ERR_INVALID_ARG, "session chunk: 0 (the default) or a multiple of 32 bytes, at least 1024");
    h->sess.chunk_bytes = chunk_bytes;
    return S2M_OK;
}

int s2m_debug_sc_keys(s2m_handle h, int32_t first, int32_t count, float* ring, double* sector)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (first < 0 || count < 0 || (size_t)first + (size_t)count > h->sc.n || (count > 0 && (!ring || !sector)))
        return fail(h, S2M_ERR_INVALID_ARG, "key range outside the descriptor store");
    if (count == 0) return S2M_OK;
    S2M_HIP(h, hipSetDevice(h->device));
    S2M_HIP(h, hipMemcpyAsync(ring, h->sc.store_ring.as<float>() + (size_t)first * S2M_SC_NUM_RING, sizeof(float) * S2M_SC_NUM_RING * (size_t)count,
                              hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipMemcpyAsync(sector, h->sc.store_sector.as<double>() + (size_t)first * S2M_SC_NUM_SECTOR,
                              sizeof(double) * S2M_SC_NUM_SECTOR * (size_t)count, hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    return S2M_OK;
}

int s2m_debug_kf_frame(s2m_handle h, int32_t key, float T_host[12], float T_device[12], float pos_device[4], int32_t* n_device)
{
    if (!h) return S2M_ERR_INVALID_ARG;
    if (key < 0 || (size_t)key >= h->kf.time.size() || !T_host || !T_device || !pos_device || !n_device)
        return fail(h, S2M_ERR_INVALID_ARG, "key outside the key-frame store, or a null output");
    S2M_HIP(h, hipSetDevice(h->device));
    KfFrame f;
    S2M_HIP(h, hipMemcpyAsync(&f, h->kf.frames.as<KfFrame>() + key, sizeof(f), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipMemcpyAsync(pos_device, h->kf.pos.as<float4>() + key, sizeof(float4), hipMemcpyDeviceToHost, h->stream));
    S2M_HIP(h, hipStreamSynchronize(h->stream));
    memcpy(T_host, h->kf.frame[(size_t)key].T, sizeof(float) * 12);
    memcpy(T_device, f.T, sizeof(float) * 12);
    *n_device = f.n;
    return S2M_OK;
}
