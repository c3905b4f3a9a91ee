// huffman_interval.hpp -- the sequential-scan Huffman decode of ONE restart interval, stated once for the host and the device.
//
// The contract is CarefulInterval::sequential_block + BitReader of entropy.cpp, value for value (T.81 F.2.2):
//   - bits come MSB first, a stuffed FF 00 is the byte FF; from the first FF that no 00 follows, and behind the interval's
//     last byte, the reader supplies 1-bits;
//   - a 16-bit window that is no codeword is symbol 0 of length 16 (Huffman::lookup);
//   - DC: extend() of T.81 F.2.2.1, a DC symbol above 16 is JPEG_AMD_EINVAL;
//   - AC: ZRL advances 16, EOB ends the block, a coefficient whose index lands at or behind 64 is dropped;
//   - blocks an interleaved MCU addresses outside a component's plane are decoded and dropped;
//   - the predictors start from zero in every interval.
// One path only (a 9-bit first level, then the canonical maxcode / mincode / valptr search): the host's fused 10-bit tables
// decode the same symbols from the same bits, so there is nothing here for the results to depend on.
//
// What keeps hostile bytes harmless, and where to see it:
//   - bytes: IntervalBits reads p only under `p < end` (refill's byte loop) or `end - p >= 4` (its four-byte step), p only
//     grows, and begin <= end is the caller's clamp: no byte outside the interval's own [begin, end) is read, so the buffer
//     needs NO padding behind it;
//   - loops: refill runs at most 8 rounds; a block is 1 DC step and at most 63 AC steps, each of which advances k by at
//     least one or ends the block; an interval is (mcu1 - mcu0) MCUs x at most 4 components x hy x hx blocks, all of it
//     geometry that the host planned (kMaxBlocksPerAxis bounds hx and hy once more);
//   - stores: a block is written only under x < ux && y < uy of its own component, at k < 64.
// Nothing else depends on the stream: garbage in gives garbage coefficients in the interval's own blocks, no more.
//
// No std::, no allocation, no recursion: the same text is instantiated by k_huffman_intervals (kernels_entropy.hip) and by
// jpeg_amd_jpeg_decode_intervals_host (entropy.cpp).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JA_HD __host__ __device__ __forceinline__
#else
#define JA_HD inline
#endif

namespace jpeg_amd {
namespace interval {

constexpr int kOk = 0, kInvalid = -1;          // JPEG_AMD_OK, JPEG_AMD_EINVAL (include/jpeg_amd.h)
constexpr int kMaxBlocksPerAxis = 16;         // an MCU holds 16 blocks at most (the planner refuses more): 16 x 1 is the widest

// A DHT table as the decoder reads it: Huffman of entropy.cpp without its fused tables.  1488 bytes, no padding inside.
struct IntervalTable {
    uint16_t fast[512];      // 9-bit first level: (length << 8) | symbol, 0 = longer than 9 bits
    int32_t maxcode[18];     // T.81 F.2.2.3; [17] is a stop
    int32_t mincode[17];
    int32_t valptr[17];
    uint8_t symbols[256];
};
static_assert(sizeof(IntervalTable) == 1488, "the table is uploaded as it lies in memory");

// One component of a scan: which plane, which tables (indices into the file's table array), how many blocks of it an MCU
// holds (1 x 1 in a scan of one component, the sampling factors otherwise) and the plane's size in blocks.
struct IntervalComp {
    int32_t plane, td, ta, hx, hy, ux, uy;
};
struct IntervalScan {
    int32_t ns, mcux, mcus, reserved;    // components; MCUs in a row; MCUs in all
    IntervalComp c[4];
};
// One file of a launch: its whole planes, int16 [uy][ux][64] zigzag, and where its block lies in the launch's buffer (byte
// offsets from the buffer's base; the arrays 16-byte aligned): its scans, its tables, its intervals and its entropy-coded bytes.
struct IntervalFile {
    int16_t *plane[4];
    uint64_t scans_at, tables_at, work_at, bytes_at, nbytes;
    uint32_t nscans, ntables, nwork, reserved[3];
};
// One restart interval: MCUs [mcu0, mcu1) of the file's scan `scan` from bytes [begin, end) of the file's entropy-coded bytes.
struct IntervalWork {
    uint32_t scan, mcu0, mcu1, reserved;
    uint64_t begin, end;
};
static_assert(sizeof(IntervalScan) % 16 == 0 && sizeof(IntervalFile) % 16 == 0 && sizeof(IntervalWork) % 16 == 0 &&
              sizeof(IntervalTable) % 16 == 0, "the arrays of a file's block follow one another, each 16-byte aligned");

struct IntervalBits {
    const uint8_t *p, *end;
    uint64_t acc;        // left-aligned; the bits below the valid ones are zero
    int nbits;
    bool marker;         // an FF that no 00 follows has been met: 1-bits from here on

    // to at least 32 valid bits: call with nbits < 32
    JA_HD void refill()
    {
        if (!marker && end - p >= 4) {                     // four bytes at once where none is FF (no stuffing, no marker)
            uint32_t x;
            __builtin_memcpy(&x, p, 4);
            const uint32_t inv = ~x;
            if (!((inv - 0x01010101u) & ~inv & 0x80808080u)) {
                acc |= (uint64_t)__builtin_bswap32(x) << (32 - nbits);
                nbits += 32;
                p += 4;
                return;
            }
        }
        for (int round = 0; round < 8 && nbits <= 56; ++round) {
            uint32_t byte = 0xff;
            if (!marker && p < end) {
                byte = *p;
                if (byte != 0xff) ++p;
                else if (end - p >= 2 && p[1] == 0x00) p += 2;   // a stuffed FF
                else marker = true;                               // RSTn, another marker, or a lone FF at the end
            }
            acc |= (uint64_t)byte << (56 - nbits);
            nbits += 8;
        }
    }
    JA_HD uint32_t peek16() const { return (uint32_t)(acc >> 48); }
    JA_HD void skip(int n) { acc <<= n; nbits -= n; }
    JA_HD uint32_t get(int n)    // 1 <= n <= 16 of the valid bits
    {
        const uint32_t v = (uint32_t)(acc >> (64 - n));
        skip(n);
        return v;
    }
};

// Huffman::lookup: the symbol and length of the codeword at the top of a 16-bit window.
JA_HD int lookup(const IntervalTable &h, uint32_t window, int &len)
{
    const uint32_t f = h.fast[window >> 7];
    if (f) { len = (int)(f >> 8); return (int)(f & 0xff); }
    for (len = 10; len <= 16; ++len) {
        const int code = (int)(window >> (16 - len));
        if (code <= h.maxcode[len]) {
            if (code < h.mincode[len]) break;              // below the first code of this length: not a codeword
            return h.symbols[(h.valptr[len] + code - h.mincode[len]) & 255];
        }
    }
    len = 16;
    return 0;
}

JA_HD int extend(int v, int s) { return v >= (1 << (s - 1)) ? v : v - (1 << s) + 1; }   // T.81 F.2.2.1, 1 <= s <= 16

// The 64 zeros a block starts from.  On the device the planes are 16-byte aligned (the calls require it).
JA_HD void zero_block(int16_t *blk)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint4 *q = reinterpret_cast<uint4 *>(blk);
    for (int i = 0; i < 8; ++i) q[i] = make_uint4(0, 0, 0, 0);
#else
    for (int i = 0; i < 64; ++i) blk[i] = 0;
#endif
}

// One block (T.81 F.2.2) into blk, zeroed here first, then its coefficients one by one; blk == nullptr: decoded and dropped.
JA_HD int decode_block(IntervalBits &br, const IntervalTable &dc, const IntervalTable &ac, int16_t *blk, uint32_t &pred)
{
    if (blk) zero_block(blk);
    if (br.nbits < 32) br.refill();                        // a code and its magnitude: 32 bits at most
    int len;
    const int t = lookup(dc, br.peek16(), len);
    br.skip(len);
    if (t > 16) return kInvalid;
    if (t) pred += (uint32_t)extend((int)br.get(t), t);    // (modulo 2^32: only the low 16 bits are kept)
    if (blk) blk[0] = (int16_t)pred;
    int k = 1;
    for (int step = 0; step < 63 && k < 64; ++step) {      // every step advances k or ends the block
        if (br.nbits < 32) br.refill();
        const int rs = lookup(ac, br.peek16(), len);
        br.skip(len);
        const int r = rs >> 4, sz = rs & 15;
        if (sz == 0) {
            if (r != 15) break;                            // EOB
            k += 16;                                       // ZRL
            continue;
        }
        k += r;
        const int v = extend((int)br.get(sz), sz);
        if (k < 64 && blk) blk[k] = (int16_t)v;
        ++k;
    }
    return kOk;
}

// MCUs [mcu0, mcu1) of scan s from [begin, end).  The caller has clamped begin <= end to its buffer, mcu1 to s.mcus and the
// table indices to its table array.
JA_HD int decode_interval(const IntervalScan &s, const IntervalTable *tables, int16_t *const planes[4], const uint8_t *begin,
                          const uint8_t *end, uint32_t mcu0, uint32_t mcu1)
{
    IntervalBits br{begin, end, 0, 0, false};
    uint32_t pred0 = 0, pred1 = 0, pred2 = 0, pred3 = 0;   // per scan component (named: no indexed array in registers)
    const uint32_t mcux = (uint32_t)s.mcux;
    uint32_t my = mcu0 / mcux, mx = mcu0 - my * mcux;
    for (uint32_t mcu = mcu0; mcu < mcu1; ++mcu) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < 4; ++j) {
            if (j >= s.ns) break;
            const IntervalComp &c = s.c[j];
            uint32_t &pred = j == 0 ? pred0 : j == 1 ? pred1 : j == 2 ? pred2 : pred3;
            const int hx = c.hx < kMaxBlocksPerAxis ? c.hx : kMaxBlocksPerAxis, hy = c.hy < kMaxBlocksPerAxis ? c.hy : kMaxBlocksPerAxis;
            for (int by = 0; by < hy; ++by)
                for (int bx = 0; bx < hx; ++bx) {
                    const uint64_t x = (uint64_t)mx * (uint32_t)hx + (uint32_t)bx, y = (uint64_t)my * (uint32_t)hy + (uint32_t)by;
                    const bool inside = x < (uint64_t)c.ux && y < (uint64_t)c.uy;
                    int16_t *blk = inside ? planes[c.plane & 3] + 64 * ((uint64_t)c.ux * y + x) : nullptr;
                    const int st = decode_block(br, tables[c.td], tables[c.ta], blk, pred);
                    if (st != kOk) return st;
                }
        }
        if (++mx == mcux) { mx = 0; ++my; }
    }
    return kOk;
}

}  // namespace interval
}  // namespace jpeg_amd
