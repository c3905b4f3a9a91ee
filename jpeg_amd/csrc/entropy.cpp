// entropy.cpp -- host-side JPEG parsing + Huffman entropy decoding into Spectral planes.
//
// SURVEY.md section 8f-1/f-2 ("next" rows): the stage that FEEDS the GPU hot path.  It fills
// the same containers the reference's JPEG.Context fills (decode.swift:3554-3961): per
// component int16 [units_y][units_x][64] in zigzag order, plus the quantisation table bound to
// each component.  Entropy coding stays on the host CPU by design (north_star).
//
// Written from ITU-T T.81 (Annex F sequential, Annex G progressive); the reference behaviours
// that matter for parity of the hot path are mirrored and cited:
//   - plane geometry units = ceil(size * factor / (8 * scale))        decode.swift:2456-2495
//   - blocks an interleaved scan addresses beyond `units` are decoded and dropped  :1459-1475
//   - a component's quantisation table is bound at its first scan (sequential scan or
//     progressive DC-first scan) from whatever the DQT slot holds then   :3447-3473, 3486-3496
//   - coefficients are stored quantised, zigzag order                    :1434, 1466
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#include <emmintrin.h>
#define JA_X86_STREAMING 1
#else
#define JA_X86_STREAMING 0
#endif

#include "../../include/jpeg_amd.h"
#include "sparse_format.hpp"
#include "interval_plan.hpp"

namespace sparse_fmt = jpeg_amd::sparse;   // (Decoder::sparse is the output of a sparse decode)

namespace {

struct Huffman {
    // 9-bit first-level table: (length << 8) | symbol, 0 = longer than 9 bits
    uint16_t fast[512];
    // canonical decode for long codes (T.81 F.2.2.3)
    int32_t maxcode[18];
    int32_t valptr[17];
    int32_t mincode[17];
    uint8_t symbols[256];
    // Sequential scans (round 5): ONE lookup per symbol on a 10-bit window wherever code + magnitude bits fit in it.
    //   look_ac: bits 0-4 bits to skip (0 = take the general path), bits 5-9 coefficients to advance (run + 1; 16 for ZRL;
    //            0 = EOB), bit 10 a coefficient is stored, bits 16-31 its value.
    //   look_dc: bits 0-4 bits to skip (0 = general path), bits 8-31 the DC difference (signed).
    uint32_t look_ac[1024];
    int32_t look_dc[1024];
    bool defined = false;

    // Decoder subscript of the reference (decode.swift:1243-1261): the symbol and length of the codeword at the top
    // of a 16-bit window.  A window that matches no codeword decodes as SYMBOL 0 OF LENGTH 16 -- the reference
    // renders damaged streams that way instead of failing (tests/unit/tests.swift:424-430), and so does this decoder.
    inline int lookup(uint16_t window, int &len) const
    {
        const uint16_t f = fast[window >> 7];
        if (f) { len = f >> 8; return f & 0xff; }
        for (len = 10; len <= 16; ++len) {
            const int code = window >> (16 - len);
            if (code <= maxcode[len]) {
                if (code < mincode[len]) break;          // below the first code of this length: not a codeword
                return symbols[valptr[len] + code - mincode[len]];
            }
        }
        len = 16;
        return 0;
    }

    // Builds into a temporary and commits only on success: a malformed DHT leaves the previous table intact.
    bool build(const uint8_t counts[16], const uint8_t *syms, int nsyms)
    {
        Huffman t;
        if (!t.build_in_place(counts, syms, nsyms)) return false;
        *this = t;
        return true;
    }

    bool build_in_place(const uint8_t counts[16], const uint8_t *syms, int nsyms)
    {
        if (nsyms < 0 || nsyms > 256) return false;
        std::memset(fast, 0, sizeof fast);
        std::memcpy(symbols, syms, (size_t)nsyms);
        int code = 0, k = 0;
        for (int len = 1; len <= 16; ++len) {
            valptr[len] = k;
            mincode[len] = code;
            for (int i = 0; i < counts[len - 1]; ++i, ++k, ++code) {
                if (k >= nsyms) return false;
                if (len <= 9) {
                    const int lo = code << (9 - len), hi = lo + (1 << (9 - len));
                    if (hi > 512) return false;
                    for (int c = lo; c < hi; ++c) fast[c] = (uint16_t)((len << 8) | syms[k]);
                }
            }
            maxcode[len] = counts[len - 1] ? code - 1 : -1;
            if (code > (1 << len)) return false;
            code <<= 1;
        }
        maxcode[17] = 0x7fffffff;
        for (int w = 0; w < 1024; ++w) {
            int len;
            const int sym = lookup((uint16_t)(w << 6), len);
            look_ac[w] = 0; look_dc[w] = 0;
            if (len > 10) continue;                                     // (a window that is no codeword has length 16)
            auto magnitude = [&](int size) {                            // the `size` bits behind the code, extended (T.81 F.2.2.1)
                int v = (w >> (10 - len - size)) & ((1 << size) - 1);
                if (v < (1 << (size - 1))) v += 1 - (1 << size);
                return v;
            };
            const int run = sym >> 4, size = sym & 15;
            if (size == 0) look_ac[w] = run == 15 ? (uint32_t)(len | (16 << 5)) : run == 0 ? (uint32_t)len : 0u;   // ZRL, EOB
            else if (len + size <= 10) look_ac[w] = (uint32_t)(len + size) | ((uint32_t)(run + 1) << 5) | (1u << 10) | ((uint32_t)(uint16_t)(int16_t)magnitude(size) << 16);
            if (sym == 0) look_dc[w] = len;                            // difference 0
            else if (sym <= 16 && len + sym <= 10) look_dc[w] = (len + sym) | (magnitude(sym) * 256);
        }
        defined = true;
        return true;
    }
};

// MSB-first bit reader over one entropy-coded segment with byte stuffing removed on the fly.
// Past the end of the data it supplies 1-bits (a truncated stream then decodes as padding).
struct BitReader {
    const uint8_t *p, *end;
    uint64_t acc = 0;   // left-aligned bit buffer
    int nbits = 0;
    bool hit_marker = false;

    BitReader(const uint8_t *b, const uint8_t *e) : p(b), end(e) {}

    inline void refill()
    {
        // fast path: eight bytes loaded at once when none of them is 0xFF (no stuffing, no marker).  As many whole bytes as fit
        // are accounted for; the bits of the next, partial byte land below the valid region, where the next refill ORs the
        // same bits again.
        if (!hit_marker && p + 8 <= end) {
            uint64_t x;
            std::memcpy(&x, p, 8);
            const uint64_t inv = ~x;
            if (!((inv - 0x0101010101010101ull) & ~inv & 0x8080808080808080ull)) {
                const int nb = (64 - nbits) >> 3;
                acc |= nbits ? __builtin_bswap64(x) >> nbits : __builtin_bswap64(x);
                p += nb;
                nbits += 8 * nb;
                return;
            }
        }
        while (nbits <= 56) {
            uint32_t byte = 0xff;
            if (!hit_marker && p < end) {
                byte = *p;
                if (byte == 0xff) {
                    if (p + 1 < end && p[1] == 0x00) p += 2;          // stuffed 0xFF
                    else { hit_marker = true; byte = 0xff; }           // RSTn / next marker: stop
                } else {
                    ++p;
                }
            }
            acc |= (uint64_t)byte << (56 - nbits);
            nbits += 8;
        }
    }
    inline uint32_t peek(int n) { return (uint32_t)(acc >> (64 - n)); }
    inline void skip(int n) { acc <<= n; nbits -= n; }
    inline uint32_t get(int n)
    {
        if (n == 0) return 0;
        if (nbits < n) refill();
        const uint32_t v = peek(n);
        skip(n);
        return v;
    }
    inline int decode(const Huffman &h)
    {
        if (nbits < 16) refill();
        const uint16_t f = h.fast[peek(9)];
        if (f) { skip(f >> 8); return f & 0xff; }
        int len;
        const int sym = h.lookup((uint16_t)peek(16), len);
        skip(len);
        return sym;
    }
    // at a restart boundary: drop the padding bits and position on the byte after RSTn
    // (refill never reads past a marker, so everything buffered belongs to the old interval)
    void restart()
    {
        acc = 0; nbits = 0;
        while (p + 1 < end && !(p[0] == 0xff && p[1] >= 0xd0 && p[1] <= 0xd7)) ++p;
        if (p + 1 < end) p += 2;
        hit_marker = false;
    }
};

// ---- sequential scans: the fast path (round 5) -------------------------------------------------------------------------
// The entropy-coded bytes of one restart interval are first copied WITHOUT their stuffing (0xFF 0x00 -> 0xFF; the copy ends
// at the first marker) and followed by 16 bytes of 0xFF, so that the reader below needs no test for stuffing, markers or the
// end of the data: past the end it reads 1-bits, exactly what BitReader supplies there.
struct CleanReader {
    const uint8_t *p, *limit;   // limit: the last address a load may start at (all 0xFF from there on)
    uint64_t acc = 0;           // left-aligned; the bits below the valid ones are already those of the bytes that follow
    int nbits = 0;

    inline void refill()        // to >= 56 valid bits, without a branch
    {
        uint64_t x;
        std::memcpy(&x, p, 8);
        acc |= __builtin_bswap64(x) >> nbits;
        p += (63 - nbits) >> 3;
        nbits |= 56;
        p = p > limit ? limit : p;
    }
    inline uint32_t peek10() const { return (uint32_t)(acc >> 54); }
    inline void skip(int n) { acc <<= n; nbits -= n; }
    inline int symbol(const Huffman &h)                          // any code (<= 16 bits): call with >= 16 valid bits
    {
        int len;
        const int sym = h.lookup((uint16_t)(acc >> 48), len);
        skip(len);
        return sym;
    }
    inline int magnitude(int size)                               // 1 <= size <= 16 bits, extended (T.81 F.2.2.1)
    {
        const int v = (int)(acc >> (64 - size));
        skip(size);
        return v >= (1 << (size - 1)) ? v : v - (1 << size) + 1;
    }
};

// Removes the stuffing of [b, e) into `out` (grown as needed); returns the end of the clean bytes, which 16 bytes of 0xFF follow.
inline const uint8_t *unstuff(const uint8_t *b, const uint8_t *e, std::vector<uint8_t> &out)
{
    if (out.size() < (size_t)(e - b) + 16) out.resize((size_t)(e - b) + 16);
    uint8_t *o = out.data();
    while (b < e) {
        const uint8_t *ff = static_cast<const uint8_t *>(std::memchr(b, 0xff, (size_t)(e - b)));
        if (!ff) { std::memcpy(o, b, (size_t)(e - b)); o += e - b; break; }
        if (ff + 1 < e && ff[1] == 0x00) {                       // a stuffed 0xFF: data
            std::memcpy(o, b, (size_t)(ff + 1 - b));
            o += ff + 1 - b;
            b = ff + 2;
        } else {                                                 // RSTn, another marker, or a lone 0xFF at the end: stop
            std::memcpy(o, b, (size_t)(ff - b));
            o += ff - b;
            break;
        }
    }
    std::memset(o, 0xff, 16);
    return o;
}

// A finished block goes to its plane whole.  With `streaming` (16-byte aligned planes) by non-temporal stores: the plane is
// written once and read next by a DMA engine or another thread, so the lines need not be fetched, nor kept, by this core.
inline void store_block(int16_t *dst, const int16_t *tmp, bool streaming)
{
#if JA_X86_STREAMING
    if (streaming) {
        const __m128i *s = reinterpret_cast<const __m128i *>(tmp);
        __m128i *d = reinterpret_cast<__m128i *>(dst);
        for (int i = 0; i < 8; ++i) _mm_stream_si128(d + i, _mm_load_si128(s + i));
        return;
    }
#endif
    (void)streaming;
    std::memcpy(dst, tmp, 128);
}

// Several AC symbols per lookup: the table over a kChainBits window, composed from Huffman::look_ac, holds as many whole
// symbols as fit in the window and store at most two coefficients -- "3 -1 ZRL ZRL ZRL EOB" is one entry (the reference's
// encoder, and this library's, emit a ZRL for every complete run of 16 zeros, also in front of the EOB: encode.swift:917-958).
//   bits 0-3 bits to skip (0: the first symbol does not fit, take the general path), 4-10 / 11-17 offsets from k of the two
//   stores, 18-24 advance of k, bit 25 the block ends here (EOB), 26-31 the advance in front of the LAST symbol,
//   32-47 / 48-63 the two values.
// An entry always stores twice: one with a single coefficient stores it twice, one with none stores 0 at k, which is still 0
// in a block that is filled front to back.  It may only be used while k + (advance in front of the last symbol) <= 63: no
// symbol but the last may complete the block, because what follows a complete block is the next block's DC code.
#ifndef JA_CHAIN_BITS
#define JA_CHAIN_BITS 10
#endif
constexpr int kChainBits = JA_CHAIN_BITS, kChainSize = 1 << kChainBits;
static_assert(kChainBits >= 10 && kChainBits <= 15, "skip is a 4-bit field; look_ac is a 10-bit table");
inline void build_chain_table(const Huffman &h, uint64_t *t)
{
    for (int w = 0; w < kChainSize; ++w) {
        int pos = 0, advance = 0, guard = 0, stores = 0, eob = 0, symbols = 0;
        int at[2] = {0, 0}, val[2] = {0, 0};
        for (;;) {
            const uint32_t e = h.look_ac[((w << pos) & (kChainSize - 1)) >> (kChainBits - 10)];
            const int l = (int)(e & 31), n = (int)(e >> 5) & 31;
            if (!e || pos + l > kChainBits || advance > 63) break;
            if (n && (e & 1024) && stores == 2) break;
            guard = advance;
            pos += l;
            ++symbols;
            if (n == 0) { eob = 1; break; }
            if (e & 1024) { at[stores] = advance + n - 1; val[stores++] = (int)(e >> 16); }
            advance += n;
        }
        if (stores == 1) { at[1] = at[0]; val[1] = val[0]; }
        t[w] = symbols == 0 ? 0
             : (uint64_t)pos | ((uint64_t)at[0] << 4) | ((uint64_t)at[1] << 11) | ((uint64_t)advance << 18) | ((uint64_t)eob << 25)
               | ((uint64_t)guard << 26) | ((uint64_t)(uint16_t)val[0] << 32) | ((uint64_t)(uint16_t)val[1] << 48);
    }
}
// DC difference + "nothing but zeros behind it" (ZRLs, if any, and the EOB) over the same window: bits 0-3 bits to skip
// (0: general path), bit 6 the block is complete, bits 16-31 the difference.
inline void build_dc_table(const Huffman &d, const Huffman &a, uint32_t *t)
{
    for (int w = 0; w < kChainSize; ++w) {
        const int32_t e = d.look_dc[w >> (kChainBits - 10)];
        t[w] = 0;
        if (!e) continue;
        const int l = e & 31;
        t[w] = (uint32_t)l | ((uint32_t)(uint16_t)(int16_t)(e >> 8) << 16);
        int pos = l, k = 1;
        for (;;) {
            const uint32_t e2 = a.look_ac[((w << pos) & (kChainSize - 1)) >> (kChainBits - 10)];
            const int l2 = (int)(e2 & 31), n2 = (int)(e2 >> 5) & 31;
            if (!e2 || pos + l2 > kChainBits || (e2 & 1024) || k > 63) break;
            pos += l2;
            if (n2 == 0) { t[w] = (uint32_t)pos | 64u | ((uint32_t)(uint16_t)(int16_t)(e >> 8) << 16); break; }
            k += n2;                                            // ZRL
        }
    }
}

inline int extend(int v, int s) { return (s == 0 || v >= (1 << (s - 1))) ? v : v - (1 << s) + 1; }  // T.81 F.2.2.1

struct Component {
    int id = 0, fx = 1, fy = 1, tq = 0;
    int ux = 0, uy = 0;
    int16_t *coef = nullptr;
    bool bound = false;
    size_t first_block = 0;   // sparse output: index of the plane's block (0, 0) in the descriptor array
};

// Sparse output of a sequential file (jpeg_amd_jpeg_decode_sparse): the record of sparse_format.hpp instead of int16 planes.
// An eighth of the bytes to write on the host and to move across PCIe; k_expand_sparse (kernels_stage.hip) turns it into the
// planes on the device.
struct SparseOut {
    uint32_t *desc = nullptr;
    uint32_t *entries = nullptr;
    size_t ndesc = 0, capacity = 0, n = 0;
};
int16_t g_sparse_sentinel[1];   // what Component::coef points at in a sparse decode (never dereferenced)

// ---- one scan: what its header says, parsed once (Decoder::plan_scan) ----
struct ScanComp { Component *c; int td, ta; };
struct Slot { Component *c; int td, ta, bx, by; };   // one block of an MCU: its component and tables, its place in the MCU
enum class BlockKind { Sequential, DcFirst, DcRefine, AcFirst, AcRefine };
struct ScanPlan {
    int ns = 0;
    ScanComp sc[4];
    int ss = 0, se = 63, ah = 0, al = 0;
    bool progressive = false;
    BlockKind kind = BlockKind::Sequential;
    Slot slots[16];
    int nslots = 0;
    int mcux = 0, mcuy = 0;
    long total = 0, ri = 0, nintervals = 0;   // MCUs of the scan, MCUs of a restart interval (the whole scan without one)
};

// Where the block of slot `sl` of MCU (mx, my) lies in its component's plane.
struct BlockAt { int x, y; };
inline BlockAt block_at(const ScanPlan &plan, const Slot &sl, int mx, int my)
{
    return plan.ns > 1 ? BlockAt{mx * sl.c->fx + sl.bx, my * sl.c->fy + sl.by} : BlockAt{mx, my};
}

// Where the restart intervals of the entropy-coded segment [ecs, end) start: its first byte, then the byte behind every RSTn.
// As many entries as the scan has intervals only when every marker is where it should be.
inline std::vector<const uint8_t *> find_interval_starts(const uint8_t *ecs, const uint8_t *end, long nintervals)
{
    std::vector<const uint8_t *> starts{ecs};
    if (nintervals > 1)
        for (const uint8_t *q = ecs; q + 1 < end;) {
            q = static_cast<const uint8_t *>(std::memchr(q, 0xff, (size_t)(end - 1 - q)));
            if (!q) break;
            if (q[1] >= 0xd0 && q[1] <= 0xd7) starts.push_back(q + 2);
            q += q[1] == 0xff ? 1 : 2;          // 0xFF fill bytes may precede a marker
        }
    return starts;
}

// work(0) ... work(t_n - 1), each once: up to t_n - 1 of them on threads of their own, index 0 -- and every index whose thread
// could not be started -- on this thread; nothing is left joinable.  An exception inside work(t) becomes
// status[t] = JPEG_AMD_ENOMEM where a status array (t_n entries or more) is given, and never leaves its thread.
template <class Work>
void run_on_threads(int t_n, const Work &work, int *status = nullptr)
{
    auto guarded = [&](int t) {
        try {
            work(t);
        } catch (...) {
            if (status) status[t] = JPEG_AMD_ENOMEM;
        }
    };
    std::vector<std::thread> pool;
    int started = 1;
    try {
        pool.reserve((size_t)t_n);
        for (int t = 1; t < t_n; ++t) { pool.emplace_back(guarded, t); ++started; }
    } catch (...) {
    }
    for (int t = started; t < t_n; ++t) guarded(t);
    guarded(0);
    for (std::thread &th : pool) th.join();
}

struct Decoder {
    const uint8_t *data;
    size_t n;
    jpeg_amd_frame_info info{};
    std::vector<Component> comps;
    uint16_t qslots[4][64];
    bool qdefined[4] = {false, false, false, false};
    Huffman dc[4], ac[4];
    int restart_interval = 0;
    int nthreads = 1;            // host threads for restart-interval-parallel scans
    bool auto_threads = false;   // nthreads chosen by the library: only where a thread pays off
    int max_scans = 0x7fffffff;  // stop after this many scans (progressive previews, JPEG.Context-style)
    SparseOut *sparse = nullptr; // entries instead of planes (sequential scans with every restart marker in place only)
    // the planner of the device entropy decoder: nothing is decoded, every scan adds to the work list instead.  `refused`:
    // the file is well formed as far as the walk has come, but not for the device (the walk goes on: what is malformed
    // further on still decides)
    jpeg_amd::interval::FilePlan *intervals = nullptr;
    bool refused = false, scanned[JPEG_AMD_MAX_PLANES] = {false, false, false, false};
    int nscans = 0;

    static int units(int size, int stride) { return size / stride + (size % stride != 0 ? 1 : 0); }

    // ---- marker segments ----
    int parse_dqt(const uint8_t *s, size_t len)
    {
        size_t i = 0;
        while (i < len) {
            const int pq = s[i] >> 4, tq = s[i] & 15;
            ++i;
            if (tq > 3 || pq > 1 || i + (pq ? 128 : 64) > len) return JPEG_AMD_EINVAL;
            for (int z = 0; z < 64; ++z) {
                qslots[tq][z] = pq ? (uint16_t)((s[i] << 8) | s[i + 1]) : s[i];   // file order is zigzag
                i += pq ? 2 : 1;
            }
            qdefined[tq] = true;
        }
        return JPEG_AMD_OK;
    }
    int parse_dht(const uint8_t *s, size_t len)
    {
        size_t i = 0;
        while (i < len) {
            if (i + 17 > len) return JPEG_AMD_EINVAL;
            const int tc = s[i] >> 4, th = s[i] & 15;
            int total = 0;
            for (int k = 0; k < 16; ++k) total += s[i + 1 + k];
            if (tc > 1 || th > 3 || total > 256 || i + 17 + (size_t)total > len) return JPEG_AMD_EINVAL;
            if (!(tc ? ac[th] : dc[th]).build(s + i + 1, s + i + 17, total)) return JPEG_AMD_EINVAL;
            i += 17 + (size_t)total;
        }
        return JPEG_AMD_OK;
    }
    // clearing a large plane is worth sharing too (200 MB for an 8192 x 8192 image)
    void zero_plane(int16_t *p, size_t bytes) const
    {
        const size_t piece = (size_t)4 << 20;
        const int t_n = (int)std::min<size_t>((size_t)nthreads, bytes / piece);
        if (t_n < 2) { std::memset(p, 0, bytes); return; }
        const size_t per = (bytes / t_n + 63) & ~(size_t)63;
        run_on_threads(t_n, [=](int t) {
            const size_t lo = std::min(bytes, per * t), hi = t + 1 == t_n ? bytes : std::min(bytes, per * (t + 1));
            std::memset(reinterpret_cast<char *>(p) + lo, 0, hi - lo);
        });
    }

    // Height 0 in the frame header: the real height follows the FIRST scan in a DNL segment
    // (T.81 B.2.5; JPEG.Header.HeightRedefinition, decode.swift:837-860, Context.push(height:)).
    // The planes are sized before that scan is decoded, so the DNL is looked up ahead of time.
    int height_from_dnl(size_t pos) const
    {
        while (pos + 3 < n) {
            if (data[pos] != 0xff) return 0;
            const int m = data[pos + 1];
            if (m == 0xff) { ++pos; continue; }
            if (m == 0xd9) return 0;
            const size_t seglen = ((size_t)data[pos + 2] << 8) | data[pos + 3];
            if (seglen < 2 || pos + 2 + seglen > n) return 0;
            if (m != 0xda) { pos += 2 + seglen; continue; }
            size_t e = pos + 2 + seglen;                 // entropy-coded segment of the first scan
            while (e + 1 < n) {
                if (data[e] != 0xff) { ++e; continue; }
                const int k = data[e + 1];
                if (k == 0x00 || (k >= 0xd0 && k <= 0xd7)) { e += 2; continue; }
                if (k == 0xff) { ++e; continue; }
                break;
            }
            if (e + 5 < n && data[e + 1] == 0xdc && data[e + 2] == 0 && data[e + 3] == 4)
                return (data[e + 4] << 8) | data[e + 5];
            return 0;
        }
        return 0;
    }

    int parse_sof(int marker, const uint8_t *s, size_t len)
    {
        if (len < 6) return JPEG_AMD_EINVAL;
        info.process = marker == 0xc0 ? 0 : marker == 0xc1 ? 1 : 2;
        info.precision = s[0];
        info.height = (s[1] << 8) | s[2];
        info.width = (s[3] << 8) | s[4];
        const int nc = s[5];
        if (nc < 1 || nc > JPEG_AMD_MAX_PLANES || len < 6 + 3 * (size_t)nc) return JPEG_AMD_ENOSUP;
        if (info.height == 0) info.height = height_from_dnl((size_t)(s + len - data));
        if (info.width <= 0 || info.height <= 0) return JPEG_AMD_EINVAL;
        info.ncomponents = nc;
        comps.assign((size_t)nc, Component());
        int sx = 0, sy = 0;
        for (int c = 0; c < nc; ++c) {
            comps[c].id = s[6 + 3 * c];
            comps[c].fx = s[7 + 3 * c] >> 4;
            comps[c].fy = s[7 + 3 * c] & 15;
            comps[c].tq = s[8 + 3 * c];
            if (comps[c].fx < 1 || comps[c].fy < 1 || comps[c].tq > 3) return JPEG_AMD_EINVAL;
            if (comps[c].fx > sx) sx = comps[c].fx;
            if (comps[c].fy > sy) sy = comps[c].fy;
        }
        info.scale_x = sx; info.scale_y = sy;
        size_t blocks_before = 0;
        for (int c = 0; c < nc; ++c) {
            comps[c].ux = units(info.width * comps[c].fx, 8 * sx);
            comps[c].uy = units(info.height * comps[c].fy, 8 * sy);
            comps[c].first_block = blocks_before;
            blocks_before += (size_t)comps[c].ux * comps[c].uy;
            info.id[c] = comps[c].id;
            info.factor_x[c] = comps[c].fx; info.factor_y[c] = comps[c].fy;
            info.units_x[c] = comps[c].ux;  info.units_y[c] = comps[c].uy;
        }
        return JPEG_AMD_OK;
    }

    // ---- one scan (defined below, behind the readers it is made of) ----
    int plan_scan(const uint8_t *hdr, size_t hlen, ScanPlan *plan);
    int bind_tables(const ScanPlan &plan, uint16_t (*quanta_out)[64]);
    int decode_scan(const uint8_t *hdr, size_t hlen, const uint8_t *ecs, const uint8_t *end, uint16_t (*quanta_out)[64]);
    int plan_intervals(const ScanPlan &plan, int planned, const uint8_t *ecs, const uint8_t *end);

    // Walk the whole file.  coef == nullptr: headers only (fills info, counts scans).
    // Resumable: `pos`, `have_frame` and all tables live in the object.  With `streaming` set the
    // walk stops (status OK, nothing consumed) in front of the first segment or entropy-coded
    // segment that is not complete yet -- JPEG.Context fed by a growing byte stream
    // (decode.swift:3554-3961, examples/decode-online); `finished` is set at EOI.
    size_t pos = 0;
    size_t scan_search_segment = (size_t)-1, scan_search_from = 0;   // streaming: where the hunt for a scan's end stopped
    static constexpr long long kStreamMaxBlocks = 1LL << 25;
    bool have_frame = false, streaming = false, finished = false;
    std::vector<std::vector<int16_t>> own_planes;       // streaming: the decoder owns the planes
    uint16_t own_quanta[JPEG_AMD_MAX_PLANES][64];

    // The frame header is in.  The stream decoder OWNS the planes: an attacker-chosen frame size must not make it allocate
    // tens of gigabytes from a 20-byte header.  32 Mi blocks (4 GiB of coefficients, e.g. a 4:2:0 image of 37 000 x 37 000)
    // is the cap; larger frames go through the one-shot entry points, where the caller allocates.
    int own_the_planes()
    {
        long long blocks = 0;
        for (int c = 0; c < info.ncomponents; ++c) blocks += (long long)comps[c].ux * comps[c].uy;
        if (blocks > kStreamMaxBlocks) return JPEG_AMD_ENOMEM;
        have_frame = true;
        own_planes.assign((size_t)info.ncomponents, {});
        for (int c = 0; c < info.ncomponents; ++c) {
            own_planes[c].assign((size_t)64 * comps[c].ux * comps[c].uy, 0);
            comps[c].coef = own_planes[c].data();
            for (int z = 0; z < 64; ++z) own_quanta[c][z] = 1;
        }
        return JPEG_AMD_OK;
    }
    // The frame header is in, one-shot decode: the caller's planes, or the sparse record, become the components' output
    // (neither: an inspect-only pass).
    int bind_output(int16_t *const coef[])
    {
        have_frame = true;
        if (sparse) {
            if (info.process == 2) return JPEG_AMD_ENOSUP;      // progressive scans add to a block: planes only
            size_t frame_blocks = 0;
            for (const Component &c : comps) frame_blocks += (size_t)c.ux * c.uy;
            if (frame_blocks > sparse->ndesc || frame_blocks >= sparse_fmt::kAbsent) return JPEG_AMD_EINVAL;   // the caller's array is too small
            std::memset(sparse->desc, 0xff, frame_blocks * sizeof(uint32_t));
            for (int c = 0; c < info.ncomponents; ++c) comps[c].coef = g_sparse_sentinel;
        } else if (coef)
            for (int c = 0; c < info.ncomponents; ++c) {
                if (!coef[c]) return JPEG_AMD_EINVAL;
                comps[c].coef = coef[c];
                // progressive scans only add to a block; sequential ones clear it themselves
                if (info.process == 2 || max_scans != 0x7fffffff)
                    zero_plane(coef[c], (size_t)128 * comps[c].ux * comps[c].uy);
            }
        return JPEG_AMD_OK;
    }

    int run(int16_t *const coef[], uint16_t (*quanta_out)[64])
    {
        if (pos == 0) {
            if (n < 4) return streaming ? JPEG_AMD_OK : JPEG_AMD_EINVAL;
            if (data[0] != 0xff || data[1] != 0xd8) return JPEG_AMD_EINVAL;
            pos = 2;
        }
        while (pos + 1 < n && !finished) {
            const size_t segment_start = pos;
            if (data[pos] != 0xff) return JPEG_AMD_EINVAL;
            while (pos + 1 < n && data[pos + 1] == 0xff) ++pos;
            if (pos + 1 >= n) { if (streaming) pos = segment_start; break; }
            const int marker = data[pos + 1];
            pos += 2;
            if (marker == 0xd9) { finished = true; break; }              // EOI
            if (marker == 0x01 || (marker >= 0xd0 && marker <= 0xd7)) continue;
            if (pos + 2 > n) { if (streaming) { pos = segment_start; break; } return JPEG_AMD_EINVAL; }
            const size_t seglen = ((size_t)data[pos] << 8) | data[pos + 1];
            if (seglen < 2) return JPEG_AMD_EINVAL;
            if (pos + seglen > n) { if (streaming) { pos = segment_start; break; } return JPEG_AMD_EINVAL; }
            const uint8_t *seg = data + pos + 2;
            const size_t len = seglen - 2;
            pos += seglen;
            int st = JPEG_AMD_OK;
            switch (marker) {
                case 0xdb: st = parse_dqt(seg, len); break;
                case 0xc4: st = parse_dht(seg, len); break;
                case 0xc0: case 0xc1: case 0xc2:
                    if (have_frame) return JPEG_AMD_ENOSUP;
                    if (streaming && len >= 3 && seg[1] == 0 && seg[2] == 0 && height_from_dnl((size_t)(seg + len - data)) == 0) {
                        pos = segment_start;                                // height comes with a DNL not here yet
                        goto out_of_data;
                    }
                    st = parse_sof(marker, seg, len);
                    if (st == JPEG_AMD_OK)
                        for (int c = 0; c < info.ncomponents; ++c)     // the bound the device ABI puts on a plane (check_layout)
                            if ((long long)comps[c].ux * comps[c].uy > (1LL << 30)) return JPEG_AMD_EINVAL;
                    if (st == JPEG_AMD_OK) st = streaming ? own_the_planes() : bind_output(coef);
                    break;
                case 0xc3: case 0xc5: case 0xc6: case 0xc7: case 0xc9: case 0xca: case 0xcb:
                case 0xcd: case 0xce: case 0xcf:
                    return JPEG_AMD_ENOSUP;                                // lossless / hierarchical / arithmetic
                case 0xdd:
                    if (len < 2) return JPEG_AMD_EINVAL;
                    restart_interval = (seg[0] << 8) | seg[1];
                    break;
                case 0xda: {
                    if (!have_frame) return JPEG_AMD_EINVAL;
                    // entropy-coded data runs to the next marker that is not RSTn / stuffing.  A streaming decoder that
                    // comes back to the same scan with more bytes resumes the search where the last one gave up.
                    size_t e = (streaming && scan_search_segment == segment_start && scan_search_from > pos) ? scan_search_from : pos;
                    while (e + 1 < n) {
                        const void *ff = std::memchr(data + e, 0xff, n - 1 - e);
                        if (!ff) { e = n; break; }
                        e = (size_t)(static_cast<const uint8_t *>(ff) - data);
                        const int m = data[e + 1];
                        if (m == 0x00 || (m >= 0xd0 && m <= 0xd7)) { e += 2; continue; }
                        if (m == 0xff) { ++e; continue; }
                        break;
                    }
                    if (e + 1 >= n) {
                        if (streaming) {                                            // the scan's end is not here yet
                            scan_search_segment = segment_start;
                            scan_search_from = n > 0 ? n - 1 : 0;                   // the last byte may be half of a marker
                            pos = segment_start;
                            goto out_of_data;
                        }
                        e = n;
                    }
                    st = decode_scan(seg, len, data + pos, data + e, streaming ? own_quanta : quanta_out);
                    ++nscans;
                    pos = e;
                    if (nscans >= max_scans) pos = n;   // the caller wants the image as it stands now
                    break;
                }
                default: break;                                           // APPn, COM, ...: skipped; DNL: see parse_sof
            }
            if (st != JPEG_AMD_OK) return st;
        }
    out_of_data:
        if (!have_frame) return streaming ? JPEG_AMD_OK : JPEG_AMD_EINVAL;
        info.nscans = nscans;
        info.restart_interval = restart_interval;
        return JPEG_AMD_OK;
    }
};

// ---- the careful reader: any scan, byte by byte ------------------------------------------------------------------------
// One restart interval (or the whole scan): MCUs [mcu0, mcu1) from `br`, predictors and the EOB run starting from zero
// (T.81 E.2.4).  Intervals touch disjoint blocks.  The Huffman tables are checked block by block: a scan that names an
// undefined table fails at its first block.
struct CarefulInterval {
    const Decoder &d;
    const ScanPlan &plan;
    int pred[4] = {0, 0, 0, 0};
    int eobrun = 0;
    int16_t dummy[64];      // where the blocks go that an interleaved scan addresses beyond the plane

    // sequential: the blocks of this MCU row that belong to the interval (`span` MCUs from mx) are cleared here, a row at a
    // time -- large enough for the library's wide memset, small enough to still be in cache when they are filled (clearing the
    // whole plane up front costs a quarter of the decode time; clearing block by block, 128 bytes at a time, a third)
    void clear_mcu_row(int mx, int my, long span) const
    {
        for (int j = 0; j < plan.ns; ++j) {
            Component *c = plan.sc[j].c;
            const int fx = plan.ns > 1 ? c->fx : 1, fy = plan.ns > 1 ? c->fy : 1;
            const int x0 = std::min(mx * fx, c->ux), x1 = (int)std::min<long>((mx + span) * fx, c->ux);
            for (int y = my * fy; y < std::min(my * fy + fy, c->uy); ++y)
                if (x1 > x0) std::memset(c->coef + (size_t)64 * ((size_t)c->ux * y + x0), 0, (size_t)128 * (x1 - x0));
        }
    }

    // sequential: T.81 F.2.2, into a block that clear_mcu_row has cleared
    int sequential_block(BitReader &br, const Slot &sl, int16_t *blk, int &pred_c) const
    {
        if (!d.dc[sl.td].defined || !d.ac[sl.ta].defined) return JPEG_AMD_EINVAL;
        if (br.nbits < 32) br.refill();
        int diff;
        const int32_t ed = d.dc[sl.td].look_dc[br.peek(10)];
        if (ed) {                                           // code and difference in one lookup
            br.skip(ed & 31);
            diff = ed >> 8;
        } else {
            const int t = br.decode(d.dc[sl.td]);
            if (t < 0 || t > 16) return JPEG_AMD_EINVAL;
            diff = extend((int)br.get(t), t);
        }
        pred_c += diff;
        blk[0] = (int16_t)pred_c;
        const Huffman &h = d.ac[sl.ta];
        for (int k = 1; k < 64;) {
            if (br.nbits < 32) br.refill();
            const uint32_t e = h.look_ac[br.peek(10)];
            if (e) {                                        // run, size and value -- or EOB / ZRL -- in one lookup
                br.skip((int)(e & 31));
                const int adv = (int)(e >> 5) & 31;
                if (adv == 0) break;                        // EOB
                k += adv;
                if ((e & 1024) && k <= 64) blk[k - 1] = (int16_t)(e >> 16);
                continue;
            }
            const int rs = br.decode(h);
            if (rs < 0) return JPEG_AMD_EINVAL;
            const int r = rs >> 4, sz = rs & 15;
            if (sz == 0) {
                if (r == 15) { k += 16; continue; }
                break;
            }
            k += r;
            const int v = extend((int)br.get(sz), sz);
            if (k < 64) blk[k] = (int16_t)v;
            ++k;
        }
        return JPEG_AMD_OK;
    }

    // DC first: T.81 G.1.2.1
    int dc_first(BitReader &br, const Slot &sl, int16_t *blk, int &pred_c) const
    {
        if (!d.dc[sl.td].defined) return JPEG_AMD_EINVAL;
        const int t = br.decode(d.dc[sl.td]);
        if (t < 0 || t > 16) return JPEG_AMD_EINVAL;
        pred_c += extend((int)br.get(t), t);
        blk[0] = (int16_t)(pred_c * (1 << plan.al));
        return JPEG_AMD_OK;
    }

    // DC refinement: one bit per block
    void dc_refine(BitReader &br, int16_t *blk) const
    {
        if (br.get(1)) blk[0] = (int16_t)(blk[0] | (1 << plan.al));
    }

    // AC first: T.81 G.1.2.2
    int ac_first(BitReader &br, const Slot &sl, int16_t *blk)
    {
        if (eobrun > 0) { --eobrun; return JPEG_AMD_OK; }
        if (!d.ac[sl.ta].defined) return JPEG_AMD_EINVAL;
        const Huffman &h = d.ac[sl.ta];
        const int se = plan.se, al = plan.al;
        for (int k = plan.ss; k <= se;) {
            const int rs = br.decode(h);
            if (rs < 0) return JPEG_AMD_EINVAL;
            const int r = rs >> 4, s = rs & 15;
            if (s == 0) {
                if (r < 15) { eobrun = (1 << r) - 1; if (r) eobrun += (int)br.get(r); break; }
                k += 16;
                continue;
            }
            k += r;
            const int v = extend((int)br.get(s), s);
            if (k <= se) blk[k] = (int16_t)(v * (1 << al));
            ++k;
        }
        return JPEG_AMD_OK;
    }

    // AC refinement: T.81 G.1.2.3
    int ac_refine(BitReader &br, const Slot &sl, int16_t *blk)
    {
        if (!d.ac[sl.ta].defined) return JPEG_AMD_EINVAL;
        const Huffman &h = d.ac[sl.ta];
        const int se = plan.se, p1 = 1 << plan.al, m1 = -(1 << plan.al);
        int k = plan.ss;
        auto refine = [&](int16_t &cf) {
            if (br.get(1) && (cf & p1) == 0) cf = (int16_t)(cf >= 0 ? cf + p1 : cf + m1);
        };
        if (eobrun == 0) {
            for (; k <= se; ++k) {
                const int rs = br.decode(h);
                if (rs < 0) return JPEG_AMD_EINVAL;
                int r = rs >> 4;
                const int s = rs & 15;
                int val = 0;
                if (s) {
                    val = br.get(1) ? p1 : m1;
                } else if (r < 15) {
                    eobrun = 1 << r;
                    if (r) eobrun += (int)br.get(r);
                    break;
                }
                for (; k <= se; ++k) {
                    if (blk[k] != 0) refine(blk[k]);
                    else if (--r < 0) break;
                }
                if (s && k <= se) blk[k] = (int16_t)val;
            }
        }
        if (eobrun > 0) {
            for (; k <= se; ++k)
                if (blk[k] != 0) refine(blk[k]);
            --eobrun;
        }
        return JPEG_AMD_OK;
    }

    int run(BitReader &br, long mcu0, long mcu1)
    {
        const int mcux = plan.mcux;
        int my = (int)(mcu0 / mcux), mx = (int)(mcu0 - (long)my * mcux) - 1;
        for (long mcu = mcu0; mcu < mcu1; ++mcu) {
            if (++mx == mcux) { mx = 0; ++my; }
            if (!plan.progressive && (mx == 0 || mcu == mcu0))
                clear_mcu_row(mx, my, std::min<long>(mcux - mx, mcu1 - mcu));     // MCUs of this row inside the interval
            for (int si = 0; si < plan.nslots; ++si) {
                const Slot &sl = plan.slots[si];
                Component *c = sl.c;
                const BlockAt at = block_at(plan, sl, mx, my);
                const bool inside = at.x < c->ux && at.y < c->uy;
                int16_t *blk = inside ? c->coef + (size_t)64 * ((size_t)c->ux * at.y + at.x) : dummy;
                const int ci = (int)(c - d.comps.data());
                if (!inside) std::memset(dummy, 0, sizeof dummy);
                int st = JPEG_AMD_OK;
                switch (plan.kind) {
                    case BlockKind::Sequential: st = sequential_block(br, sl, blk, pred[ci]); break;
                    case BlockKind::DcFirst: st = dc_first(br, sl, blk, pred[ci]); break;
                    case BlockKind::DcRefine: dc_refine(br, blk); break;
                    case BlockKind::AcFirst: st = ac_first(br, sl, blk); break;
                    case BlockKind::AcRefine: st = ac_refine(br, sl, blk); break;
                }
                if (st != JPEG_AMD_OK) return st;
            }
        }
        return JPEG_AMD_OK;
    }
};

// ---- the fast reader: sequential scans whose restart markers are all in place (or that have none) -------------------------
// The chain and DC tables of a scan's slots, built once per scan.
struct FastTables {
    std::vector<uint64_t> pair_tables;
    std::vector<uint32_t> dc_tables;
    const uint64_t *pair_of[16];
    const uint32_t *dcx_of[16];

    int build(const Decoder &d, const ScanPlan &plan)
    {
        for (int si = 0; si < plan.nslots; ++si)
            if (!d.dc[plan.slots[si].td].defined || !d.ac[plan.slots[si].ta].defined) return JPEG_AMD_EINVAL;
        pair_tables.resize((size_t)kChainSize * 4);
        dc_tables.resize((size_t)kChainSize * 16);
        bool have_pair[4] = {false, false, false, false}, have_dcx[16] = {};
        for (int si = 0; si < plan.nslots; ++si) {
            const int td = plan.slots[si].td, ta = plan.slots[si].ta, both = td * 4 + ta;
            if (!have_pair[ta]) { build_chain_table(d.ac[ta], pair_tables.data() + (size_t)kChainSize * ta); have_pair[ta] = true; }
            if (!have_dcx[both]) { build_dc_table(d.dc[td], d.ac[ta], dc_tables.data() + (size_t)kChainSize * both); have_dcx[both] = true; }
            pair_of[si] = pair_tables.data() + (size_t)kChainSize * ta;
            dcx_of[si] = dc_tables.data() + (size_t)kChainSize * both;
        }
        return JPEG_AMD_OK;
    }
};

// What every interval of such a scan reads.  One restart interval comes from its own bytes [b, e), on a copy without
// stuffing.  A block is decoded into a local buffer (zero, then its few coefficients) and copied out whole, so the plane is
// written once, front to back, and never read -- or its coefficients go to the sparse record as entries.
struct FastScan {
    const Decoder &d;
    const ScanPlan &plan;
    const FastTables &tables;

    int interval(const uint8_t *b, const uint8_t *e, long mcu0, long mcu1, std::vector<uint8_t> &scratch) const;
};

// One restart interval in flight: where its reader is, and which block comes next.
struct Walk {
    CleanReader br{nullptr, nullptr};
    int pred[4] = {0, 0, 0, 0};
    long mcu = 0, mcu1 = 0;
    int mx = 0, my = 0, si = 0;
    bool streaming = false;
    uint32_t *ent = nullptr, *ent_end = nullptr;   // sparse output: the next entry, the end of the arena
    alignas(64) int16_t tmp[128];      // [64, 128): where the stores of a damaged stream land that run past the block

    Walk(const FastScan &fs, const uint8_t *b, const uint8_t *e, long mcu0, long mcu_end, std::vector<uint8_t> &scratch)
    {
        const uint8_t *clean_end = unstuff(b, e, scratch);
        br = CleanReader{scratch.data(), clean_end + 8};
        size_t plane_bytes = 0;
        streaming = true;
        for (int j = 0; j < fs.plan.ns; ++j) {
            const Component *c = fs.plan.sc[j].c;
            streaming = streaming && (reinterpret_cast<uintptr_t>(c->coef) & 15) == 0;
            plane_bytes += (size_t)128 * c->ux * c->uy;
        }
        streaming = streaming && plane_bytes >= ((size_t)1 << 20);     // smaller planes stay in this core's cache
        std::memset(tmp, 0, sizeof tmp);
        mcu = mcu0; mcu1 = mcu_end;
        my = (int)(mcu0 / fs.plan.mcux); mx = (int)(mcu0 - (long)my * fs.plan.mcux);
        si = 0;
    }

    // the next block of the walk (slot si of MCU mcu)
    template <bool SPARSE>
    __attribute__((always_inline)) int next(const FastScan &fs)
    {
        uint32_t *const ent0 = ent;
        if constexpr (SPARSE) {
            if (ent + jpeg_amd::kSparseDecoderHeadroom > ent_end) return JPEG_AMD_ENOSUP;      // the arena is full: the caller decodes this file densely
        }
        const Slot &sl = fs.plan.slots[si];
        Component *c = sl.c;
        const BlockAt at = block_at(fs.plan, sl, mx, my);
        const int x = at.x, y = at.y;
        const int ci = (int)(c - fs.d.comps.data());
        // ---- DC (T.81 F.2.2.1), together with an EOB right behind it where both fit the window ----
        br.refill();
        const uint32_t ed = fs.tables.dcx_of[si][br.acc >> (64 - kChainBits)];
        bool done = false;
        int budget = 0;                                      // valid bits a lookup may still count on
        if (ed & 15) {
            br.skip((int)(ed & 15));
            budget = 56 - (int)(ed & 15);
            pred[ci] += (int32_t)ed >> 16;
            done = (ed & 64) != 0;
        } else {
            const int t = br.symbol(fs.d.dc[sl.td]);
            if (t > 16) return JPEG_AMD_EINVAL;
            if (t) pred[ci] += br.magnitude(t);
        }
        if constexpr (SPARSE) *ent++ = sparse_fmt::make((uint16_t)(int16_t)pred[ci], 0);
        else tmp[0] = (int16_t)pred[ci];
        // ---- AC (T.81 F.2.2.2) ----
        int k = 1;
        if (!done) {
            const Huffman &h = fs.d.ac[sl.ta];
            const uint64_t *chains = fs.tables.pair_of[si];
            while (k < 64) {
                if (budget < kChainBits) { br.refill(); budget = 56; }
                uint64_t en = chains[br.acc >> (64 - kChainBits)];
                if (__builtin_expect(k + (int)((en >> 26) & 63) > 63, 0)) {
                    // a symbol in the middle of the entry would complete the block: one symbol at a time
                    const uint32_t e1 = h.look_ac[br.peek10()];
                    const uint64_t n1 = (e1 >> 5) & 31;
                    en = e1 == 0 ? 0 : (uint64_t)(e1 & 31) | (n1 << 18) | (n1 ? 0 : 1ull << 25)
                         | (e1 & 1024 ? ((n1 - 1) << 4) | ((n1 - 1) << 11) | ((uint64_t)(e1 >> 16) << 32) | ((uint64_t)(e1 >> 16) << 48) : 0);
                }
                const int n = (int)(en & 15);
                if (__builtin_expect(n == 0, 0)) {           // a code + magnitude longer than 10 bits: the long way
                    br.refill();
                    budget = 0;
                    const int rs = br.symbol(h);
                    const int r = rs >> 4, sz = rs & 15;
                    if (sz == 0) {
                        if (r != 15) break;
                        k += 16;
                        continue;
                    }
                    k += r;
                    if constexpr (SPARSE) *ent++ = sparse_fmt::make((uint16_t)(int16_t)br.magnitude(sz), (uint32_t)k);
                    else tmp[k] = (int16_t)br.magnitude(sz);  // k <= 63 + 15
                    ++k;
                    continue;
                }
                br.skip(n);
                budget -= n;
                if constexpr (SPARSE) {
                    // the entry's two stores: both written, the cursor advanced by the number that are real (a
                    // coefficient is never zero; an entry without one has value 0, one with a single one repeats it)
                    const uint32_t a1 = (uint32_t)(en >> 4) & 127, a2 = (uint32_t)(en >> 11) & 127;
                    const uint32_t v1 = (uint32_t)(en >> 32) & 0xffffu, v2 = (uint32_t)(en >> 48);
                    ent[0] = sparse_fmt::make(v1, (uint32_t)k + a1);
                    ent[1] = sparse_fmt::make(v2, (uint32_t)k + a2);
                    ent += (v1 != 0) + (a1 != a2);
                } else {
                    tmp[k + ((en >> 4) & 127)] = (int16_t)(en >> 32);
                    tmp[k + ((en >> 11) & 127)] = (int16_t)(en >> 48);
                }
                k += (int)(en >> 18) & 127;
                if (en & (1ull << 25)) break;
            }
        }
        if constexpr (SPARSE) {
            if (x < c->ux && y < c->uy) {
                if (__builtin_expect(k > 64, 0)) {                   // a damaged stream ran past the block: drop what lies beyond
                    uint32_t *keep = ent0;
                    for (const uint32_t *q = ent0; q < ent; ++q)
                        if ((*q >> sparse_fmt::kZigzagShift) < 64) *keep++ = *q;   // (the whole index: no flag is set yet)
                    ent = keep;                                      // (the DC entry is always kept)
                }
                ent[-1] |= sparse_fmt::kLast;
                fs.d.sparse->desc[c->first_block + (size_t)c->ux * y + x] = (uint32_t)(ent0 - fs.d.sparse->entries);
            } else {
                ent = ent0;                                          // decoded and dropped (decode.swift:1459-1475)
            }
        } else {
            if (x < c->ux && y < c->uy) store_block(c->coef + (size_t)64 * ((size_t)c->ux * y + x), tmp, streaming);
            std::memset(tmp, 0, 128);
        }
        if (++si == fs.plan.nslots) {
            si = 0;
            ++mcu;
            if (++mx == fs.plan.mcux) { mx = 0; ++my; }
        }
        return JPEG_AMD_OK;
    }

    void end() const
    {
#if JA_X86_STREAMING
        if (streaming) _mm_sfence();
#endif
    }
};

int FastScan::interval(const uint8_t *b, const uint8_t *e, long mcu0, long mcu1, std::vector<uint8_t> &scratch) const
{
    Walk w(*this, b, e, mcu0, mcu1, scratch);
    if (SparseOut *sparse = d.sparse) {                          // (one interval after the other: the arena is shared)
        w.ent = sparse->entries + sparse->n;
        w.ent_end = sparse->entries + sparse->capacity;
        while (w.mcu < w.mcu1) {
            const int st = w.next<true>(*this);
            if (st != JPEG_AMD_OK) return st;
        }
        sparse->n = (size_t)(w.ent - sparse->entries);
        return JPEG_AMD_OK;
    }
    while (w.mcu < w.mcu1) {
        const int st = w.next<false>(*this);
        if (st != JPEG_AMD_OK) return st;
    }
    w.end();
    return JPEG_AMD_OK;
}

// ---- one scan ----------------------------------------------------------------------------------------------------------
// The scan header into `plan`.  EINVAL: the header is malformed.  ENOSUP: more than 16 blocks in an MCU -- the geometry's
// verdict, which decode_scan holds back behind the table binding and the inspect-only return.
int Decoder::plan_scan(const uint8_t *hdr, size_t hlen, ScanPlan *plan)
{
    if (hlen < 1) return JPEG_AMD_EINVAL;
    const int ns = plan->ns = hdr[0];
    if (ns < 1 || ns > 4 || hlen < 4 + 2 * (size_t)ns) return JPEG_AMD_EINVAL;
    ScanComp *sc = plan->sc;
    for (int j = 0; j < ns; ++j) {
        const int cid = hdr[1 + 2 * j], tt = hdr[2 + 2 * j];
        Component *c = nullptr;
        for (Component &x : comps) if (x.id == cid) c = &x;
        if (!c) return JPEG_AMD_EINVAL;
        sc[j] = {c, tt >> 4, tt & 15};
        if (sc[j].td > 3 || sc[j].ta > 3) return JPEG_AMD_EINVAL;
    }
    const int ss = plan->ss = hdr[1 + 2 * ns], se = plan->se = hdr[2 + 2 * ns];
    const int ah = plan->ah = hdr[3 + 2 * ns] >> 4;
    plan->al = hdr[3 + 2 * ns] & 15;
    const bool progressive = plan->progressive = info.process == 2;
    if (se > 63 || ss > se) return JPEG_AMD_EINVAL;
    if (progressive && ss > 0 && ns != 1) return JPEG_AMD_EINVAL;
    // (a sequential scan is decoded as the full band whatever its header says of ss, se, ah and al)
    plan->kind = !progressive ? BlockKind::Sequential
               : ss == 0 ? (ah == 0 ? BlockKind::DcFirst : BlockKind::DcRefine)
               : (ah == 0 ? BlockKind::AcFirst : BlockKind::AcRefine);

    // MCU geometry
    plan->nslots = 0;
    if (ns > 1) {
        plan->mcux = units(info.width, 8 * info.scale_x);
        plan->mcuy = units(info.height, 8 * info.scale_y);
        for (int j = 0; j < ns; ++j)
            for (int by = 0; by < sc[j].c->fy; ++by)
                for (int bx = 0; bx < sc[j].c->fx; ++bx) {
                    if (plan->nslots >= 16) return JPEG_AMD_ENOSUP;
                    plan->slots[plan->nslots++] = {sc[j].c, sc[j].td, sc[j].ta, bx, by};
                }
    } else {
        plan->mcux = sc[0].c->ux; plan->mcuy = sc[0].c->uy;
        plan->slots[plan->nslots++] = {sc[0].c, sc[0].td, sc[0].ta, 0, 0};
    }
    plan->total = (long)plan->mcux * plan->mcuy;
    plan->ri = restart_interval ? restart_interval : plan->total;
    plan->nintervals = (plan->total + plan->ri - 1) / plan->ri;
    return JPEG_AMD_OK;
}

// Quantisation tables are bound at a component's first scan, from whatever the DQT slot holds then.
int Decoder::bind_tables(const ScanPlan &plan, uint16_t (*quanta_out)[64])
{
    if (plan.ah != 0 || plan.ss != 0) return JPEG_AMD_OK;
    for (int j = 0; j < plan.ns; ++j) {
        Component *c = plan.sc[j].c;
        if (!qdefined[c->tq]) return JPEG_AMD_EINVAL;
        if (quanta_out) std::memcpy(quanta_out[c - comps.data()], qslots[c->tq], 128);
        c->bound = true;
    }
    return JPEG_AMD_OK;
}

int Decoder::decode_scan(const uint8_t *hdr, size_t hlen, const uint8_t *ecs, const uint8_t *end, uint16_t (*quanta_out)[64])
{
    ScanPlan plan;
    const int planned = plan_scan(hdr, hlen, &plan);
    if (planned == JPEG_AMD_EINVAL) return planned;
    const int bound = bind_tables(plan, quanta_out);
    if (bound != JPEG_AMD_OK) return bound;
    if (intervals) return plan_intervals(plan, planned, ecs, end);
    if (!comps[0].coef) return JPEG_AMD_OK;   // inspect-only pass
    if (planned != JPEG_AMD_OK) return planned;

    const bool fast_sequential = !plan.progressive && max_scans == 0x7fffffff;
    if (sparse && !fast_sequential) return JPEG_AMD_ENOSUP;
    FastTables tables;
    if (fast_sequential) {
        const int st = tables.build(*this, plan);
        if (st != JPEG_AMD_OK) return st;
    }
    const FastScan fast{*this, plan, tables};
    const long total = plan.total, ri = plan.ri, nintervals = plan.nintervals;
    // a thread is worth starting for a few thousand blocks, not less
    const long useful = std::min<long>(nthreads, std::min<long>(nintervals, auto_threads ? total * plan.nslots / 4096 : nintervals));
    if (useful > 1 || fast_sequential) {
        // Restart-interval-parallel decoding: the intervals of a scan are independent bit streams separated
        // by RSTn markers.  Only when every marker is where it should be; a damaged stream takes the careful path below,
        // which resynchronises like the reference.
        const std::vector<const uint8_t *> starts = find_interval_starts(ecs, end, nintervals);
        if ((long)starts.size() == nintervals) {
            std::vector<int> status((size_t)nintervals, JPEG_AMD_OK);
            const int t_n = (int)std::max<long>(1, useful);
            run_on_threads(t_n, [&](int t) {             // (t < t_n <= nintervals: status[t] exists)
                std::vector<uint8_t> scratch;
                for (long k = t; k < nintervals; k += t_n) {
                    const uint8_t *b = starts[(size_t)k], *e = k + 1 < nintervals ? starts[(size_t)k + 1] - 2 : end;
                    const long mcu0 = k * ri, mcu1 = std::min(total, (k + 1) * ri);
                    if (fast_sequential) status[(size_t)k] = fast.interval(b, e, mcu0, mcu1, scratch);
                    else {
                        BitReader br(b, e);
                        status[(size_t)k] = CarefulInterval{*this, plan}.run(br, mcu0, mcu1);
                    }
                }
            }, status.data());
            for (int st : status) if (st != JPEG_AMD_OK) return st;
            return JPEG_AMD_OK;
        }
    }
    if (sparse) return JPEG_AMD_ENOSUP;          // a restart marker is missing: the resynchronising reader writes planes
    BitReader br(ecs, end);
    for (long k = 0; k < nintervals; ++k) {
        if (k) br.restart();
        const int st = CarefulInterval{*this, plan}.run(br, k * ri, std::min(total, (k + 1) * ri));
        if (st != JPEG_AMD_OK) return st;
    }
    return JPEG_AMD_OK;
}

// ---- the planner of the device entropy decoder ---------------------------------------------------------------------------
// One scan of a file that is planned, not decoded: its record, the tables it names as they stand now, and one work item per
// restart interval.  What decode_scan refuses as malformed is refused here with the same status; what it would decode, but the
// device route does not take, sets `refused` and lets the walk go on.
int Decoder::plan_intervals(const ScanPlan &plan, int planned, const uint8_t *ecs, const uint8_t *end)
{
    namespace iv = jpeg_amd::interval;
    if (planned != JPEG_AMD_OK || plan.progressive) { refused = true; return JPEG_AMD_OK; }
    for (int si = 0; si < plan.nslots; ++si)
        if (!dc[plan.slots[si].td].defined || !ac[plan.slots[si].ta].defined) return JPEG_AMD_EINVAL;
    if (refused) return JPEG_AMD_OK;
    // a component that a second scan writes again: the host decodes the scans one after the other, the device all at once
    for (int j = 0; j < plan.ns; ++j) {
        const int ci = (int)(plan.sc[j].c - comps.data());
        if (scanned[ci]) { refused = true; return JPEG_AMD_OK; }
        scanned[ci] = true;
    }
    if (plan.nintervals > (long)JPEG_AMD_MAX_DEVICE_INTERVALS - (long)intervals->work.size()) { refused = true; return JPEG_AMD_OK; }
    const std::vector<const uint8_t *> starts = find_interval_starts(ecs, end, plan.nintervals);
    if ((long)starts.size() != plan.nintervals) { refused = true; return JPEG_AMD_OK; }   // a restart marker is missing, or one too many

    auto table_of = [&](const Huffman &h) {
        iv::IntervalTable t;
        std::memset(&t, 0, sizeof t);
        std::memcpy(t.fast, h.fast, sizeof t.fast);
        std::memcpy(t.maxcode + 1, h.maxcode + 1, sizeof(int32_t) * 17);      // ([0] is never set, nor read)
        std::memcpy(t.mincode + 1, h.mincode + 1, sizeof(int32_t) * 16);
        std::memcpy(t.valptr + 1, h.valptr + 1, sizeof(int32_t) * 16);
        const int nsyms = h.valptr[16] + (h.maxcode[16] >= 0 ? h.maxcode[16] - h.mincode[16] + 1 : 0);
        std::memcpy(t.symbols, h.symbols, (size_t)std::min(std::max(nsyms, 0), 256));
        for (size_t k = 0; k < intervals->tables.size(); ++k)
            if (std::memcmp(&intervals->tables[k], &t, sizeof t) == 0) return (int32_t)k;
        intervals->tables.push_back(t);
        return (int32_t)(intervals->tables.size() - 1);
    };
    iv::IntervalScan s{};
    s.ns = plan.ns;
    s.mcux = plan.mcux;
    s.mcus = (int32_t)plan.total;
    for (int j = 0; j < plan.ns; ++j) {
        const Component *c = plan.sc[j].c;
        s.c[j] = iv::IntervalComp{(int32_t)(c - comps.data()), table_of(dc[plan.sc[j].td]), table_of(ac[plan.sc[j].ta]),
                                  plan.ns > 1 ? c->fx : 1, plan.ns > 1 ? c->fy : 1, c->ux, c->uy};
    }
    const uint32_t scan = (uint32_t)intervals->scans.size();
    intervals->scans.push_back(s);
    intervals->bytes.push_back(iv::ScanBytes{(size_t)(ecs - data), (size_t)(end - data)});
    for (long k = 0; k < plan.nintervals; ++k) {
        const uint8_t *b = starts[(size_t)k], *e = k + 1 < plan.nintervals ? starts[(size_t)k + 1] - 2 : end;
        intervals->work.push_back(iv::IntervalWork{scan, (uint32_t)(k * plan.ri), (uint32_t)std::min(plan.total, (k + 1) * plan.ri), 0,
                                                   (uint64_t)(b - data), (uint64_t)(e - data)});
    }
    return JPEG_AMD_OK;
}

}  // namespace

int jpeg_amd::interval::plan_file(const uint8_t *data, size_t nbytes, FilePlan *plan)
{
    *plan = FilePlan{};
    Decoder d{data, nbytes};
    d.nthreads = 1;
    d.intervals = plan;
    const int st = d.run(nullptr, plan->quanta);
    if (st != JPEG_AMD_OK) return st;
    for (const Component &c : d.comps)
        if (!c.bound) return JPEG_AMD_EINVAL;   // a component no scan ever touched
    if (d.refused) return JPEG_AMD_ENOSUP;
    plan->info = d.info;
    return JPEG_AMD_OK;
}

extern "C" {

int jpeg_amd_huffman_lookup(const uint8_t counts[16], const uint8_t *values, int nvalues,
                            uint16_t window, int32_t *symbol, int32_t *length)
{
    if (!counts || (!values && nvalues > 0) || !symbol || !length || nvalues < 0 || nvalues > 256) return JPEG_AMD_EINVAL;
    int total = 0;
    for (int l = 0; l < 16; ++l) total += counts[l];
    if (total != nvalues) return JPEG_AMD_EINVAL;
    Huffman h;
    if (!h.build(counts, values, nvalues)) return JPEG_AMD_EINVAL;
    int len = 0;
    *symbol = h.lookup(window, len);
    *length = len;
    return JPEG_AMD_OK;
}

// The header promises plain C: no C++ exception (std::bad_alloc from a vector, std::system_error from a thread that
// cannot be started) may leave an entry point.
#define JA_NOTHROW_BEGIN try {
#define JA_NOTHROW_END                                      \
    } catch (const std::bad_alloc &) { return JPEG_AMD_ENOMEM; } \
    catch (...) { return JPEG_AMD_ENOMEM; }

int jpeg_amd_jpeg_inspect(const uint8_t *data, size_t nbytes, jpeg_amd_frame_info *info)
{
    if (!data || !info) return JPEG_AMD_EINVAL;
    JA_NOTHROW_BEGIN
    Decoder d{data, nbytes};
    const int st = d.run(nullptr, nullptr);
    if (st != JPEG_AMD_OK) return st;
    *info = d.info;
    return JPEG_AMD_OK;
    JA_NOTHROW_END
}

// The EXIF orientation of a file: JPEG.EXIF.parse and its subscript(tag:) (metadata.swift:440-560) for the one field that
// changes pixels -- the TIFF header's byte order and IFD0's offset, then IFD0's 12-byte entries, of which the first with tag
// 0x0112, type SHORT or LONG and count 1 gives the value, read in the file's byte order from the start of the value field.
// A marker walk from SOI to the first SOS; the first APP1 whose payload begins "Exif\0\0" is the one looked at, IFD0 the only
// directory.  Everything that is not a well-formed value in 1 .. 8 -- no segment, no tag, another type or count, an offset, an
// entry count or a segment length that leaves its container, a buffer that is no JPEG -- is orientation 1 and OK: whether the
// file can be decoded is jpeg_amd_jpeg_inspect's verdict, and a broken EXIF block never fails a decode.  No byte at or behind
// nbytes is read.
int jpeg_amd_jpeg_orientation(const uint8_t *data, size_t nbytes, int32_t *orientation)
{
    if (!data || !orientation) return JPEG_AMD_EINVAL;
    *orientation = 1;
    if (nbytes < 4 || data[0] != 0xFF || data[1] != 0xD8) return JPEG_AMD_OK;
    size_t at = 2;
    while (nbytes - at >= 4) {   // a marker and a length
        if (data[at] != 0xFF) return JPEG_AMD_OK;
        const uint8_t marker = data[at + 1];
        if (marker == 0xFF) { ++at; continue; }                                    // fill bytes in front of a marker
        if (marker == 0xD8 || marker == 0x01 || (marker >= 0xD0 && marker <= 0xD7)) { at += 2; continue; }   // no length
        if (marker == 0xDA || marker == 0xD9) return JPEG_AMD_OK;                  // the first scan, or the end
        const size_t length = ((size_t)data[at + 2] << 8) | data[at + 3];          // counts its own two bytes
        if (length < 2 || length > nbytes - at - 2) return JPEG_AMD_OK;            // the segment leaves the file
        const uint8_t *seg = data + at + 4;
        const size_t n = length - 2;
        at += 2 + length;
        if (marker != 0xE1 || n < 6 || std::memcmp(seg, "Exif\0\0", 6) != 0) continue;
        const uint8_t *tiff = seg + 6;
        const size_t m = n - 6;
        if (m < 8) return JPEG_AMD_OK;
        bool big;
        if (tiff[0] == 'I' && tiff[1] == 'I' && tiff[2] == 42 && tiff[3] == 0) big = false;
        else if (tiff[0] == 'M' && tiff[1] == 'M' && tiff[2] == 0 && tiff[3] == 42) big = true;
        else return JPEG_AMD_OK;
        const auto u16 = [&](size_t i) -> uint32_t { return big ? ((uint32_t)tiff[i] << 8) | tiff[i + 1] : ((uint32_t)tiff[i + 1] << 8) | tiff[i]; };
        const auto u32 = [&](size_t i) -> uint32_t { return big ? (u16(i) << 16) | u16(i + 2) : (u16(i + 2) << 16) | u16(i); };
        const size_t ifd = u32(4);
        if (ifd > m - 2) return JPEG_AMD_OK;                                        // the offset leaves the segment
        const size_t count = u16(ifd);
        if (count > (m - 2 - ifd) / 12) return JPEG_AMD_OK;                         // the entries leave the segment
        for (size_t e = 0; e < count; ++e) {
            const size_t entry = ifd + 2 + 12 * e;
            const uint32_t type = u16(entry + 2);
            if (u16(entry) != 0x0112 || (type != 3 && type != 4) || u32(entry + 4) != 1) continue;
            const uint32_t value = type == 3 ? u16(entry + 8) : u32(entry + 8);
            if (value >= 1 && value <= 8) *orientation = (int32_t)value;
            return JPEG_AMD_OK;                                                     // the first such entry decides
        }
        return JPEG_AMD_OK;
    }
    return JPEG_AMD_OK;
}

// The writer's script of a file (what jpeg_amd_jpeg_encode_spectral takes to write it again): a marker walk that decodes no
// entropy-coded data.  Table keys: every DQT table DEFINITION is a key, numbered in file order; a component's key is the
// definition its frame selector points at when its first scan starts (the inverse of JPEG.Layout's slot allocation,
// jpeg.swift:1383-1442).  Metadata: the APPn / COM segments in front of the frame header.
int jpeg_amd_jpeg_script(const uint8_t *data, size_t nbytes, jpeg_amd_scan *scans, int scan_capacity, int *nscans,
                         int32_t quanta_key[JPEG_AMD_MAX_PLANES], jpeg_amd_metadata *metadata, int metadata_capacity,
                         int *nmetadata)
{
    if (!data || !nscans || !quanta_key || !nmetadata || scan_capacity < 0 || metadata_capacity < 0) return JPEG_AMD_EINVAL;
    if (nbytes < 4 || data[0] != 0xff || data[1] != 0xd8) return JPEG_AMD_EINVAL;
    int ids[JPEG_AMD_MAX_PLANES], tq[JPEG_AMD_MAX_PLANES], key[JPEG_AMD_MAX_PLANES];
    int slot_key[4] = {-1, -1, -1, -1};
    int ncomp = 0, ndefs = 0, ns_total = 0, nm = 0, process = -1;
    size_t pos = 2;
    while (pos + 1 < nbytes) {
        if (data[pos] != 0xff) return JPEG_AMD_EINVAL;
        while (pos + 1 < nbytes && data[pos + 1] == 0xff) ++pos;      // fill bytes
        if (pos + 1 >= nbytes) break;
        const int m = data[pos + 1];
        pos += 2;
        if (m == 0xd9) break;                                            // EOI
        if (m == 0x01 || (m >= 0xd0 && m <= 0xd7)) continue;
        if (pos + 2 > nbytes) return JPEG_AMD_EINVAL;
        const size_t seglen = ((size_t)data[pos] << 8) | data[pos + 1];
        if (seglen < 2 || pos + seglen > nbytes) return JPEG_AMD_EINVAL;
        const uint8_t *s = data + pos + 2;
        const size_t len = seglen - 2;
        pos += seglen;
        if (process < 0 && ((m >= 0xe0 && m <= 0xef) || m == 0xfe)) {
            if (metadata && nm < metadata_capacity) {
                jpeg_amd_metadata &md = metadata[nm];
                md = jpeg_amd_metadata{};
                md.kind = m == 0xfe ? 2 : 1;
                md.app = m == 0xfe ? 0 : m - 0xe0;
                md.data = s;
                md.size = len;
            }
            ++nm;
        } else if (m == 0xc0 || m == 0xc1 || m == 0xc2) {
            if (process >= 0 || len < 6) return JPEG_AMD_EINVAL;
            process = m - 0xc0;
            ncomp = s[5];
            if (ncomp < 1 || ncomp > JPEG_AMD_MAX_PLANES || len < 6 + 3 * (size_t)ncomp) return JPEG_AMD_ENOSUP;
            for (int c = 0; c < ncomp; ++c) {
                ids[c] = s[6 + 3 * c];
                tq[c] = s[8 + 3 * c] & 3;
                key[c] = -1;
            }
        } else if (m == 0xdb) {
            size_t i = 0;
            while (i < len) {
                const int pq = s[i] >> 4, slot = s[i] & 15;
                if (pq > 1 || slot > 3 || i + 1 + (pq ? 128 : 64) > len) return JPEG_AMD_EINVAL;
                slot_key[slot] = ndefs++;
                i += 1 + (pq ? 128 : 64);
            }
        } else if (m == 0xda) {
            if (process < 0 || len < 1) return JPEG_AMD_EINVAL;
            const int ns = s[0];
            if (ns < 1 || ns > ncomp || len < 4 + 2 * (size_t)ns) return JPEG_AMD_EINVAL;
            jpeg_amd_scan sc{};
            sc.ncomponents = ns;
            for (int k = 0; k < ns; ++k) {
                int c = 0;
                while (c < ncomp && ids[c] != s[1 + 2 * k]) ++c;
                if (c == ncomp) return JPEG_AMD_EINVAL;
                if (key[c] < 0) {
                    if (slot_key[tq[c]] < 0) return JPEG_AMD_EINVAL;    // no table defined for the component yet
                    key[c] = slot_key[tq[c]];
                }
                // ascending plane order (insertion)
                int j = k;
                while (j > 0 && sc.component[j - 1] > c) {
                    sc.component[j] = sc.component[j - 1]; sc.dc[j] = sc.dc[j - 1]; sc.ac[j] = sc.ac[j - 1];
                    --j;
                }
                sc.component[j] = c;
                sc.dc[j] = s[2 + 2 * k] >> 4;
                sc.ac[j] = s[2 + 2 * k] & 15;
            }
            if (process == 2) {
                const int ss = s[1 + 2 * ns], se = s[2 + 2 * ns], ah = s[3 + 2 * ns] >> 4, al = s[3 + 2 * ns] & 15;
                sc.band_lo = ss; sc.band_hi = se + 1; sc.bit = al; sc.refine = ah ? 1 : 0;
            }
            if (scans && ns_total < scan_capacity) scans[ns_total] = sc;
            ++ns_total;
            // the entropy-coded segment runs to the next marker that is not RSTn / stuffing
            while (pos + 1 < nbytes && !(data[pos] == 0xff && data[pos + 1] != 0x00 && !(data[pos + 1] >= 0xd0 && data[pos + 1] <= 0xd7)))
                ++pos;
            if (pos + 1 >= nbytes) break;
        }
    }
    if (process < 0 || ns_total == 0) return JPEG_AMD_EINVAL;
    for (int c = 0; c < ncomp; ++c) {
        if (key[c] < 0) return JPEG_AMD_EINVAL;                          // a component no scan reaches
        quanta_key[c] = key[c];
    }
    *nscans = ns_total;
    *nmetadata = nm;
    if ((scans && ns_total > scan_capacity) || (metadata && nm > metadata_capacity)) return JPEG_AMD_EINVAL;
    return JPEG_AMD_OK;
}

int jpeg_amd_jpeg_decode_spectral(const uint8_t *data, size_t nbytes, int16_t *const h_coef[],
                                  uint16_t h_quanta[][64], jpeg_amd_frame_info *info)
{
    return jpeg_amd_jpeg_decode_spectral_mt(data, nbytes, h_coef, h_quanta, info, 1);
}

int jpeg_amd_jpeg_decode_spectral_mt(const uint8_t *data, size_t nbytes, int16_t *const h_coef[],
                                     uint16_t h_quanta[][64], jpeg_amd_frame_info *info, int nthreads)
{
    return jpeg_amd_jpeg_decode_spectral_partial(data, nbytes, h_coef, h_quanta, info, nthreads, 0);
}

int jpeg_amd_jpeg_decode_spectral_partial(const uint8_t *data, size_t nbytes, int16_t *const h_coef[],
                                          uint16_t h_quanta[][64], jpeg_amd_frame_info *info, int nthreads,
                                          int max_scans)
{
    if (!data || !h_coef || !h_quanta || max_scans < 0) return JPEG_AMD_EINVAL;
    JA_NOTHROW_BEGIN
    Decoder d{data, nbytes};
    d.nthreads = nthreads > 0 ? nthreads : (int)std::max(1u, std::thread::hardware_concurrency());
    d.auto_threads = nthreads <= 0;
    if (max_scans > 0) {
        d.max_scans = max_scans;
        // a component no scan has reached yet is all zeros: any table dequantises it to mid-grey
        for (int c = 0; c < JPEG_AMD_MAX_PLANES; ++c)
            for (int z = 0; z < 64; ++z) h_quanta[c][z] = 1;
    }
    const int st = d.run(h_coef, h_quanta);
    if (st != JPEG_AMD_OK) return st;
    for (const Component &c : d.comps)
        if (!c.bound && max_scans == 0) return JPEG_AMD_EINVAL;   // a component no scan ever touched
    if (info) *info = d.info;
    return JPEG_AMD_OK;
    JA_NOTHROW_END
}

int jpeg_amd_jpeg_decode_sparse(const uint8_t *data, size_t nbytes, uint32_t *h_desc, size_t ndesc, uint32_t *h_entries,
                                size_t capacity, size_t *nentries, uint16_t h_quanta[][64], jpeg_amd_frame_info *info)
{
    if (!data || !h_desc || !h_entries || !nentries || !h_quanta) return JPEG_AMD_EINVAL;
    JA_NOTHROW_BEGIN
    SparseOut out;
    out.desc = h_desc; out.ndesc = ndesc; out.entries = h_entries; out.capacity = capacity;
    Decoder d{data, nbytes};
    d.nthreads = 1;
    d.sparse = &out;
    const int st = d.run(nullptr, h_quanta);
    if (st != JPEG_AMD_OK) return st;
    for (const Component &c : d.comps)
        if (!c.bound) return JPEG_AMD_EINVAL;   // a component no scan ever touched
    *nentries = out.n;
    if (info) *info = d.info;
    return JPEG_AMD_OK;
    JA_NOTHROW_END
}

int jpeg_amd_jpeg_plan_intervals(const uint8_t *data, size_t nbytes, jpeg_amd_frame_info *info, int32_t *nscans, int64_t *nintervals)
{
    if (!data || !info || !nscans || !nintervals) return JPEG_AMD_EINVAL;
    JA_NOTHROW_BEGIN
    jpeg_amd::interval::FilePlan plan;
    const int st = jpeg_amd::interval::plan_file(data, nbytes, &plan);
    if (st != JPEG_AMD_OK) return st;
    *info = plan.info;
    *nscans = (int32_t)plan.scans.size();
    *nintervals = (int64_t)plan.work.size();
    return JPEG_AMD_OK;
    JA_NOTHROW_END
}

// The host instantiation of huffman_interval.hpp over the planner's work list, one interval after the other, straight from
// the file's bytes: what k_huffman_intervals computes, without a device.
int jpeg_amd_jpeg_decode_intervals_host(const uint8_t *data, size_t nbytes, int16_t *const h_coef[], uint16_t h_quanta[][64],
                                        jpeg_amd_frame_info *info)
{
    if (!data || !h_coef || !h_quanta) return JPEG_AMD_EINVAL;
    JA_NOTHROW_BEGIN
    namespace iv = jpeg_amd::interval;
    iv::FilePlan plan;
    const int st = iv::plan_file(data, nbytes, &plan);
    if (st != JPEG_AMD_OK) return st;
    int16_t *planes[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int c = 0; c < plan.info.ncomponents; ++c) {
        if (!h_coef[c]) return JPEG_AMD_EINVAL;
        planes[c] = h_coef[c];
        std::memcpy(h_quanta[c], plan.quanta[c], 128);
    }
    if (info) *info = plan.info;
    // the file's block exactly as a launch uploads it (write_file_block: only the entropy-coded bytes, the intervals' ranges
    // rebased onto them), in an allocation of exactly its size, and every interval decoded from there
    for (const iv::IntervalWork &w : plan.work)
        if (!iv::work_fits(w, plan.scans[w.scan], nbytes)) return JPEG_AMD_EINVAL;
    const iv::FileBlock b = iv::file_block(plan);
    std::vector<char> block(b.size);
    iv::write_file_block(plan, b, data, block.data());
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(block.data() + b.bytes_at);
    int first = JPEG_AMD_OK;
    for (size_t k = 0; k < plan.work.size(); ++k) {
        iv::IntervalWork w;
        std::memcpy(&w, block.data() + b.work_at + k * sizeof w, sizeof w);
        iv::IntervalScan s;
        std::memcpy(&s, block.data() + b.scans_at + w.scan * sizeof s, sizeof s);
        if (!iv::work_fits(w, s, b.nbytes)) return JPEG_AMD_EINVAL;
        const int is = iv::decode_interval(s, reinterpret_cast<const iv::IntervalTable *>(block.data() + b.tables_at), planes,
                                           bytes + w.begin, bytes + w.end, w.mcu0, w.mcu1);
        if (is != JPEG_AMD_OK && first == JPEG_AMD_OK) first = is;
    }
    return first;
    JA_NOTHROW_END
}

// ---- a decoder fed by a growing byte stream (JPEG.Context, examples/decode-online) ------------
struct jpeg_amd_stream {
    std::vector<uint8_t> bytes;
    Decoder dec{nullptr, 0};
    int failed = JPEG_AMD_OK;   // the first error is final: a decoder that has seen a malformed segment is not fed again
};

jpeg_amd_stream *jpeg_amd_stream_create(void)
{
    jpeg_amd_stream *s = new (std::nothrow) jpeg_amd_stream;
    if (s) s->dec.streaming = true;
    return s;
}

void jpeg_amd_stream_destroy(jpeg_amd_stream *s) { delete s; }

int jpeg_amd_stream_push(jpeg_amd_stream *s, const uint8_t *h_bytes, size_t nbytes, int *scans_done, int *finished)
{
    if (!s || (nbytes && !h_bytes)) return JPEG_AMD_EINVAL;
    if (s->failed != JPEG_AMD_OK) return s->failed;
    int st = JPEG_AMD_OK;
    try {
        s->bytes.insert(s->bytes.end(), h_bytes, h_bytes + nbytes);
        s->dec.data = s->bytes.data();               // the buffer may have moved: the decoder keeps offsets only
        s->dec.n = s->bytes.size();
        st = s->dec.run(nullptr, nullptr);
    } catch (const std::bad_alloc &) {
        st = JPEG_AMD_ENOMEM;
    } catch (...) {
        st = JPEG_AMD_ENOMEM;
    }
    if (st != JPEG_AMD_OK) s->failed = st;
    if (scans_done) *scans_done = s->dec.nscans;
    if (finished) *finished = s->dec.finished ? 1 : 0;
    return st;
}

int jpeg_amd_stream_info(const jpeg_amd_stream *s, jpeg_amd_frame_info *info)
{
    if (!s || !info) return JPEG_AMD_EINVAL;
    if (!s->dec.have_frame) return JPEG_AMD_EINVAL;   // no frame header yet
    *info = s->dec.info;
    info->nscans = s->dec.nscans;
    return JPEG_AMD_OK;
}

int jpeg_amd_stream_snapshot(const jpeg_amd_stream *s, int16_t *const h_coef[], uint16_t h_quanta[][64])
{
    if (!s || !h_coef || !h_quanta || !s->dec.have_frame) return JPEG_AMD_EINVAL;
    for (int c = 0; c < s->dec.info.ncomponents; ++c) {
        if (!h_coef[c]) return JPEG_AMD_EINVAL;
        std::memcpy(h_coef[c], s->dec.own_planes[(size_t)c].data(), s->dec.own_planes[(size_t)c].size() * 2);
        std::memcpy(h_quanta[c], s->dec.own_quanta[c], 128);
    }
    return JPEG_AMD_OK;
}

}  // extern "C"
