// fused_common.hpp -- device helpers of the decode, encode and resample kernels.  What is here, and who uses it:
//   - kThreads, FastDiv, make_srd, resident_workgroups_of, lds_address: every file that includes this one (the two strip walks
//     kernels_fused.hip and kernels_quad.hip, kernels_generic.hip, kernels_encode.hip, the tile kernels through tile_decode.hpp,
//     the resample kernels through resample.hpp / tensor_sink.hpp / antialias.hpp);
//   - clamp + truncate + pack under round-toward-zero (trunc_pack*, trunc_bytes8): the strip walks, the tile kernels, the encoder;
//   - LDS-DMA issue (lds_dma16*), the split arrive / wait on LDS counters (lds_arrive, lds_wait_ge*), and "the strip walks'
//     shared stages" -- block fetch from LDS, table modulation, counted wait, 2x chroma rows, colour matrix, pixel store path:
//     k_luma_fused and k_quad420 only, which differ in how a strip gets its chroma and are one text in everything else;
//   - the per-phase cycle counters of the development build (-DJA_PHASE_PROFILE, tools/phase_profile.py): k_quad420.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "dct.hpp"        // modulate_entry, zigzag_of
#include "kernels.hpp"    // u32x4_t
#include "upsample.hpp"   // ubyte_magic, lerp_row_2x, w31, kMagic

namespace jpeg_amd {

constexpr int kThreads = 256;

// Division by a launch-invariant: q = mulhi(n, floor((2^32 - 1) / d)) is the quotient or one below it for every n < 2^32, one
// compare fixes it.  The strip walks divide a dozen times per trip (strip -> image, row, column; strips left); as true
// divisions that is ~400 mostly scalar, serial instructions at the head of every trip.
struct FastDiv {
    uint32_t d, m;
    __device__ __forceinline__ void set(uint32_t div) { d = div; m = 0xffffffffu / div; }
    __device__ __forceinline__ uint32_t div(uint32_t n, uint32_t &r) const
    {
        uint32_t q = __umulhi(n, m);
        r = n - q * d;
        if (r >= d) { ++q; r -= d; }
        return q;
    }
};

// A raw buffer resource (V#) for `bytes` bytes at `p`, built from wave-uniform values: base[47:0], stride 0, num_records = bytes,
// word 3 = 0x00020000 (gfx950: 32-bit data format, no swizzle).  buffer_load / buffer_store address base + soffset + voffset
// (+ the instruction's 12-bit offset) and range-check voffset (+ offset) against num_records - soffset: out-of-range loads
// return 0, out-of-range stores are dropped (tools/probe_buffer.hip, profiles/r05_probe_buffer.txt).
typedef int i32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ i32x4_t make_srd(const void *p, uint32_t bytes)
{
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    i32x4_t r;
    r.x = (int)(uint32_t)a;
    r.y = (int)((uint32_t)(a >> 32) & 0xffffu);
    r.z = (int)bytes;
    r.w = 0x00020000;
    return r;
}

// One 16-byte-per-lane LDS-DMA: lane l's 16 B at `g` land at LDS byte address lds + 16 l.
// Issued from inline asm on purpose: hipcc cannot tell which LDS array a DMA targets, so
// after a __builtin_amdgcn_global_load_lds it makes the NEXT LDS read of any array wait with
// vmcnt(0) -- i.e. for the prefetch it was supposed to overlap.  Hidden from the compiler, the
// DMA is only waited for by the explicit s_waitcnt at the top of the next strip.  (Extra
// outstanding VM operations can only make the compiler's own counted waits longer, never
// shorter, because loads retire in order.)
__device__ __forceinline__ void lds_dma16(const void *g, uint32_t lds)
{
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off nt" ::"v"(g), "s"(lds) : "memory");
}
// The same without the `nt` hint: for coefficients that neighbouring strips fetch again soon
// (the chroma blocks around a 4:2:0 strip) and should therefore stay in L2.
__device__ __forceinline__ void lds_dma16_keep(const void *g, uint32_t lds)
{
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(lds) : "memory");
}
// A RUN of N consecutive 1 KiB pieces (a contiguous source, a contiguous destination) through a buffer resource: the
// instruction's offset field moves the source AND the LDS destination (tools/probe_dma_offset.hip), so the whole run needs one
// M0 write and one scalar offset.  Piece j takes the per-lane offset v0 (even j) or v1 (odd j): the source-side swizzle
// alternates.  source = srd.base + soff + per-lane offset (+ 1 KiB per piece), hardware range check
// against srd.num_records -- a lane whose 16 bytes lie outside the resource transfers ZEROS (tools/probe_buffer.hip T2), so
// block rows above / below a plane and runs that overhang its end need no clamped addresses.  `soff` must be a true,
// non-negative byte offset (or one that is out of range as an unsigned number).  s_nop 3: M0 is read one wait state after its
// write, and an SGPR operand the compiler happened to produce with v_readfirstlane five.
template <int N, bool NT>
__device__ __forceinline__ void lds_dma16_brun(i32x4_t srd, uint32_t soff, uint32_t v0, uint32_t v1, uint32_t lds)
{
    static_assert(N == 1 || N == 2 || N == 4, "runs of 1, 2 or 4 KiB");
#define JA_BL(v, off, hint) "buffer_load_dwordx4 " v ", %0, %1 offen" off hint " lds"
    if constexpr (N == 1) {
        if constexpr (NT) asm volatile("s_mov_b32 m0, %4\n\ts_nop 3\n\t" JA_BL("%2", "", " nt") ::"s"(srd), "s"(soff), "v"(v0), "v"(v1), "s"(lds) : "memory");
        else asm volatile("s_mov_b32 m0, %4\n\ts_nop 3\n\t" JA_BL("%2", "", "") ::"s"(srd), "s"(soff), "v"(v0), "v"(v1), "s"(lds) : "memory");
    } else if constexpr (N == 2) {
        if constexpr (NT) asm volatile("s_mov_b32 m0, %4\n\ts_nop 3\n\t" JA_BL("%2", "", " nt") "\n\t" JA_BL("%3", " offset:1024", " nt")
                                       ::"s"(srd), "s"(soff), "v"(v0), "v"(v1), "s"(lds) : "memory");
        else asm volatile("s_mov_b32 m0, %4\n\ts_nop 3\n\t" JA_BL("%2", "", "") "\n\t" JA_BL("%3", " offset:1024", "")
                          ::"s"(srd), "s"(soff), "v"(v0), "v"(v1), "s"(lds) : "memory");
    } else {
        if constexpr (NT) asm volatile("s_mov_b32 m0, %4\n\ts_nop 3\n\t" JA_BL("%2", "", " nt") "\n\t" JA_BL("%3", " offset:1024", " nt") "\n\t"
                                       JA_BL("%2", " offset:2048", " nt") "\n\t" JA_BL("%3", " offset:3072", " nt")
                                       ::"s"(srd), "s"(soff), "v"(v0), "v"(v1), "s"(lds) : "memory");
        else asm volatile("s_mov_b32 m0, %4\n\ts_nop 3\n\t" JA_BL("%2", "", "") "\n\t" JA_BL("%3", " offset:1024", "") "\n\t"
                          JA_BL("%2", " offset:2048", "") "\n\t" JA_BL("%3", " offset:3072", "")
                          ::"s"(srd), "s"(soff), "v"(v0), "v"(v1), "s"(lds) : "memory");
    }
#undef JA_BL
}

// Resident workgroups of a persistent kernel on the CURRENT device: workgroups per CU (what the occupancy query says for this
// instantiation) x CUs.  One cache per KERNEL -- the kernel's address is the template argument: all instantiations of a
// kernel template share one function TYPE, so a cache keyed by type would hand the first instantiation's answer to all of
// them -- and per device, filled once under std::call_once: contexts of several devices, and first calls from several host
// threads, see their own device's value.
constexpr int kMaxDevices = 64;
template <auto Kernel>
inline int resident_workgroups_of(int fallback_per_cu)
{
    struct PerDevice { std::once_flag once; int value = 0; };
    static PerDevice cache[kMaxDevices];   // one array per kernel instantiation
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    auto query = [&]() {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kernel, kThreads, 0) != hipSuccess || per_cu < 1) per_cu = fallback_per_cu;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
        return per_cu * cus;
    };
    if (dev >= kMaxDevices) return query();
    std::call_once(cache[dev].once, [&]() { cache[dev].value = query(); });
    return cache[dev].value;
}

// LDS byte address of a __shared__ object (low 32 bits of its flat address), wave-uniform
template <typename T>
__device__ __forceinline__ uint32_t lds_address(T *p)
{
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(__attribute__((address_space(3))) T *)p);
}

// Split arrive / wait on an LDS counter (the 4:2:0 stack walk).  The LDS executes one wave's operations in issue order, so a
// ds_add issued behind the wave's tile writes (or its last tile reads) is performed behind them: no s_waitcnt at the arrive.
// The waiting side polls with plain LDS reads; what it reads from the tile after the poll has succeeded is issued, and
// therefore performed, after the read that saw the counter.  Relaxed atomics + compiler barriers on purpose: a release /
// acquire at workgroup scope would make hipcc wait with vmcnt(0) -- for the coefficient DMA in flight and for the pixel stores.
// One lane adds, selected by narrowing EXEC around the ds_add (the compiler's form of "if (lane == 0) atomicAdd" is a dozen
// instructions: compare, save EXEC, count the active lanes, multiply, restore).  EXEC is saved and restored, not assumed:
// the helper is correct from a divergent region as long as lane 0 is active there (every call site runs with all 64 lanes).
__device__ __forceinline__ void lds_arrive(uint32_t *counter)
{
    const uint32_t addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)counter;
#ifdef JA_DEBUG_ASSERTS   // the precondition, checked in debug builds: lane 0 is active here
    if (!(__builtin_amdgcn_read_exec() & 1ull)) __builtin_trap();
#endif
    uint64_t saved;
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, 1\n\tds_add_u32 %1, %2\n\ts_mov_b64 exec, %0" : "=&s"(saved) : "v"(addr), "v"(1u) : "memory");
}
__device__ __forceinline__ uint32_t lds_peek(uint32_t *counter)
{
    return __hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_wait_ge(uint32_t *counter, uint32_t target)
{
    asm volatile("" ::: "memory");
    while ((uint32_t)__builtin_amdgcn_readfirstlane((int)lds_peek(counter)) < target) __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");
}
// the same when the counter was already read a while ago (`seen`, any lane's copy): the common case costs no LDS round trip
__device__ __forceinline__ void lds_wait_ge_seen(uint32_t *counter, uint32_t target, uint32_t seen)
{
    if ((uint32_t)__builtin_amdgcn_readfirstlane((int)seen) < target) lds_wait_ge(counter, target);
    asm volatile("" ::: "memory");
}

// ---- clamp [0, 255] + truncate + pack, the reference's float -> byte conversion (decode.swift:4121-4122, jpeg.swift:343-354)
// in ONE instruction per sample.  v_cvt_pk_u8_f32 saturates and rounds in the wave's f32 rounding mode
// (tools/probe_cvt_round.hip, profiles/r03_probe_cvt_round.txt): under round-toward-zero it truncates, where the default
// mode needs a v_floor_f32 in front of it (two half-rate instructions per sample).  The mode is switched and restored
// inside one asm statement, so nothing the compiler schedules can land between the two s_setreg; the f32 instructions
// right before and right after the statement keep round-to-nearest (tools/probe_cvt_round2.hip).
// c: 4 n floats, d: n dwords (byte i of d[k] = c[4 k + i]).
// Precondition of every trunc_* helper: the wave runs in the default f32 rounding mode (round to nearest even, MODE[1:0] =
// 0) -- the statement restores THAT, not a saved value (s_getreg + s_setreg_b32 would cost two more scalar slots per
// pack; no kernel of this library ever leaves another mode set).
#define JA_RTZ_ON "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3\n\t"
#define JA_RTZ_OFF "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0"
__device__ __forceinline__ void trunc_pack8(const float *c, uint32_t *d)
{
    asm volatile(JA_RTZ_ON
                 "v_cvt_pk_u8_f32 %0, %2, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %0, %3, 1, %0\n\t"
                 "v_cvt_pk_u8_f32 %0, %4, 2, %0\n\t"
                 "v_cvt_pk_u8_f32 %0, %5, 3, %0\n\t"
                 "v_cvt_pk_u8_f32 %1, %6, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %1, %7, 1, %1\n\t"
                 "v_cvt_pk_u8_f32 %1, %8, 2, %1\n\t"
                 "v_cvt_pk_u8_f32 %1, %9, 3, %1\n\t"
                 JA_RTZ_OFF
                 : "=&v"(d[0]), "=&v"(d[1])
                 : "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(c[4]), "v"(c[5]), "v"(c[6]), "v"(c[7]));
}
__device__ __forceinline__ void trunc_pack16(const float *c, uint32_t *d)
{
    asm volatile(JA_RTZ_ON
                 "v_cvt_pk_u8_f32 %0, %4, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %0, %5, 1, %0\n\t"
                 "v_cvt_pk_u8_f32 %0, %6, 2, %0\n\t"
                 "v_cvt_pk_u8_f32 %0, %7, 3, %0\n\t"
                 "v_cvt_pk_u8_f32 %1, %8, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %1, %9, 1, %1\n\t"
                 "v_cvt_pk_u8_f32 %1, %10, 2, %1\n\t"
                 "v_cvt_pk_u8_f32 %1, %11, 3, %1\n\t"
                 "v_cvt_pk_u8_f32 %2, %12, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %2, %13, 1, %2\n\t"
                 "v_cvt_pk_u8_f32 %2, %14, 2, %2\n\t"
                 "v_cvt_pk_u8_f32 %2, %15, 3, %2\n\t"
                 "v_cvt_pk_u8_f32 %3, %16, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %3, %17, 1, %3\n\t"
                 "v_cvt_pk_u8_f32 %3, %18, 2, %3\n\t"
                 "v_cvt_pk_u8_f32 %3, %19, 3, %3\n\t"
                 JA_RTZ_OFF
                 : "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2]), "=&v"(d[3])
                 : "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(c[4]), "v"(c[5]), "v"(c[6]), "v"(c[7]), "v"(c[8]), "v"(c[9]), "v"(c[10]), "v"(c[11]), "v"(c[12]), "v"(c[13]), "v"(c[14]), "v"(c[15]));
}
__device__ __forceinline__ void trunc_pack24(const float *c, uint32_t *d)
{
    asm volatile(JA_RTZ_ON
                 "v_cvt_pk_u8_f32 %0, %6, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %0, %7, 1, %0\n\t"
                 "v_cvt_pk_u8_f32 %0, %8, 2, %0\n\t"
                 "v_cvt_pk_u8_f32 %0, %9, 3, %0\n\t"
                 "v_cvt_pk_u8_f32 %1, %10, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %1, %11, 1, %1\n\t"
                 "v_cvt_pk_u8_f32 %1, %12, 2, %1\n\t"
                 "v_cvt_pk_u8_f32 %1, %13, 3, %1\n\t"
                 "v_cvt_pk_u8_f32 %2, %14, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %2, %15, 1, %2\n\t"
                 "v_cvt_pk_u8_f32 %2, %16, 2, %2\n\t"
                 "v_cvt_pk_u8_f32 %2, %17, 3, %2\n\t"
                 "v_cvt_pk_u8_f32 %3, %18, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %3, %19, 1, %3\n\t"
                 "v_cvt_pk_u8_f32 %3, %20, 2, %3\n\t"
                 "v_cvt_pk_u8_f32 %3, %21, 3, %3\n\t"
                 "v_cvt_pk_u8_f32 %4, %22, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %4, %23, 1, %4\n\t"
                 "v_cvt_pk_u8_f32 %4, %24, 2, %4\n\t"
                 "v_cvt_pk_u8_f32 %4, %25, 3, %4\n\t"
                 "v_cvt_pk_u8_f32 %5, %26, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %5, %27, 1, %5\n\t"
                 "v_cvt_pk_u8_f32 %5, %28, 2, %5\n\t"
                 "v_cvt_pk_u8_f32 %5, %29, 3, %5\n\t"
                 JA_RTZ_OFF
                 : "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2]), "=&v"(d[3]), "=&v"(d[4]), "=&v"(d[5])
                 : "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(c[4]), "v"(c[5]), "v"(c[6]), "v"(c[7]), "v"(c[8]), "v"(c[9]), "v"(c[10]), "v"(c[11]), "v"(c[12]), "v"(c[13]), "v"(c[14]), "v"(c[15]), "v"(c[16]), "v"(c[17]), "v"(c[18]), "v"(c[19]), "v"(c[20]), "v"(c[21]), "v"(c[22]), "v"(c[23]));
}
// eight samples, each into byte 0 of its own dword (the other bytes 0)
__device__ __forceinline__ void trunc_bytes8(const float *c, uint32_t *d)
{
    asm volatile(JA_RTZ_ON
                 "v_cvt_pk_u8_f32 %0, %8, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %1, %9, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %2, %10, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %3, %11, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %4, %12, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %5, %13, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %6, %14, 0, 0\n\t"
                 "v_cvt_pk_u8_f32 %7, %15, 0, 0\n\t"
                 JA_RTZ_OFF
                 : "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2]), "=&v"(d[3]), "=&v"(d[4]), "=&v"(d[5]), "=&v"(d[6]), "=&v"(d[7])
                 : "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(c[4]), "v"(c[5]), "v"(c[6]), "v"(c[7]));
}

// ---- the strip walks' shared stages (k_luma_fused, kernels_fused.hip; k_quad420, kernels_quad.hip) --------------------------
// A strip is BX x BY luma blocks, BX * BY = 64, one block per work-item of a wave.  The two walks differ in how a strip gets its
// chroma samples; what follows is the same in both.  Every helper is inlined into the kernel's trip: the statement order inside
// a helper is the order the kernels were tuned in.

// (The source swizzle of the coefficient DMA, sgpr() and the buffer resource over a strip's block rows stay in the two kernels:
// hoisted, they change the instructions of k_luma_fused -- profiles/strip_walk_shared_isa.txt.)

// The work-item's block (32 dwords) out of the LDS image of the coefficient DMA: slot u = 64 i + lane of the wave's buffer holds
// chunk (u & 7) ^ ((b >> 1) & 7) of block b = u >> 3, so the eight ds_read_b128 of a lane (stride 128 B between lanes) are
// bank-conflict-free.
__device__ __forceinline__ void read_block(const uint32_t *coef_w, int lane, uint32_t (&w)[32])
{
    const uint4 *cw = reinterpret_cast<const uint4 *>(coef_w) + 8 * lane;
    const int sw = (lane >> 1) & 7;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 v = cw[i ^ sw];
        w[4 * i + 0] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
}
// one entry per lane of the modulated table of quantisation table `qi` of image `img` -- TRANSPOSED ([8 k + h], dct.hpp TransposedTable)
__device__ __forceinline__ void modulate_table(float *table, const uint16_t *quanta, int img, size_t quanta_stride, int qi, int lane)
{
    const int qk = lane & 7, qh = lane >> 3;
    table[8 * qk + qh] = modulate_entry(qk, qh, 0.125f, quanta[img * quanta_stride + 64 * qi + zigzag_of(qk, qh)]);
}
// Wait for the coefficient DMA.  VM operations retire in issue order and the DMA was issued BEFORE the previous strip's pixel
// stores: when that strip took the branch-free store path (exactly 2 store instructions per pixel row, StripStore) only the
// DMA has to be waited for, not the 16 stores behind it.
__device__ __forceinline__ void wait_dma(int stores_behind_dma)
{
    if (stores_behind_dma == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// One patch row of a chroma plane that is subsampled 2x in x, from its three tile dwords (the dword left of the block's four
// samples, the samples, the dword right of them): conversion + horizontal interpolation.  The samples enter as
// 2^15 + p + 1/32 (ubyte_magic, upsample.hpp) so that the 3a + b steps are exact and the final rounding needs no floor.
__device__ __forceinline__ void hconv_2x(const uint32_t (&r)[3], float (&o)[8])
{
    const float p[6] = {ubyte_magic<3>(r[0]), ubyte_magic<0>(r[1]), ubyte_magic<1>(r[1]),
                        ubyte_magic<2>(r[1]), ubyte_magic<3>(r[1]), ubyte_magic<0>(r[2])};
    lerp_row_2x(p, o);
}
// Final chroma value of one pixel from the weighted sum v of DIV / 4 magic samples: floor(v / DIV + 1/2) [- 128 for RGB],
// without a floor.  DIV = 4 (one subsampled axis, v = 3a + b): V = 2^17 + v + 1/8 arrives exact, and fma(V, 1/4, 1.5 * 2^23 -
// 2^15 [- 128]) is ONE rounding of 1.5 * 2^23 [- 128] + v / 4 + 1/32 to a float whose ulp is 1; v / 4 + 1/32 is never half-way,
// and at v / 4 = n + 1/2 the 1/32 tips it up like the reference's round-half-away.  DIV = 16 (4:2:0): upsample.hpp.
// tests/test_colour_rounding.py enumerates every input.  An FMA and a subtraction instead of an FMA and a v_floor_f32 (half
// rate): -128 slow instructions per strip.
template <int MODE, int DIV>
__device__ __forceinline__ float chroma_finish(float v)
{
    return __builtin_fmaf(v, 1.0f / DIV, kMagic - 32768.0f - (MODE == 1 ? 128.0f : 0.0f)) - kMagic;
}
// One pixel row of a plane that is subsampled 2x in y, from the sliding window hw over its patch rows: slots hold rows (y >> 1),
// (y >> 1) + 1, (y >> 1) + 2.  The nearer patch row (the middle of the window) weighs 3, the farther one (above for even y,
// below for odd) 1.  On odd rows the row requested two pixel rows ago (rawn) is converted into the third slot first (hconv:
// the kernel's conversion of a patch row) and the window slides afterwards.
template <int MODE, int DIV, class HConv>
__device__ __forceinline__ void window_row(int y, HConv hconv, const uint32_t (&rawn)[3], float (&hw)[3][8], float (&cv)[8])
{
    if ((y & 1) == 1) hconv(rawn, hw[2]);
#pragma unroll
    for (int x = 0; x < 8; ++x) cv[x] = chroma_finish<MODE, DIV>(w31(hw[1][x], hw[(y & 1) ? 2 : 0][x]));
    if ((y & 1) == 1) {
#pragma unroll
        for (int x = 0; x < 8; ++x) { hw[0][x] = hw[1][x]; hw[1][x] = hw[2][x]; }
    }
}
// Colour of one pixel (MODE 1: RGB, 0: YCbCr) from integer-valued floats; pb, pr arrive as cb - 128, cr - 128 for RGB.
// jpeg.swift:441-453: x = (y + m_cb cb) + m_cr cr (the 0.0 * c terms are exact no-ops), clamped and TRUNCATED -- the caller's
// trunc_pack24.  One FMA for R and B, two for G in this association (the other one is NOT exact): after the truncation every
// one of the 2^16 / 2^24 input combinations gives the reference's byte (tests/test_colour_rounding.py enumerates them).
template <int MODE>
__device__ __forceinline__ void colour_pixel(float yy, float pb, float pr, float *c)
{
    if constexpr (MODE == 1) {
        c[0] = __builtin_fmaf(1.40200f, pr, yy);
        c[1] = __builtin_fmaf(-0.71414f, pr, __builtin_fmaf(-0.34414f, pb, yy));
        c[2] = __builtin_fmaf(1.77200f, pb, yy);
    } else {
        c[0] = yy; c[1] = pb; c[2] = pr;
    }
}

// voffset of a chunk: its place `base` where d < 0, an out-of-range value (0x80000000) elsewhere
__device__ __forceinline__ uint32_t place(uint32_t base, int d)
{
    const uint32_t m = (uint32_t)(d >> 31);               // all ones where d < 0
    return (base & m) | (0x80000000u & ~m);               // one v_bfi_b32
}

// Two 16-byte chunks per lane through the buffer resource srd, row offset soff (scalar): the store instructions of a pixel row.
// (The chunks arrive BY VALUE: taken by reference, the same statement compiles to another order of the walk's scalar copies.)
__device__ __forceinline__ void store_chunk_pair(uint4 c0, uint32_t voff0, uint4 c1, uint32_t voff1, i32x4_t srd, uint32_t soff)
{
    const u32x4_t q0 = {c0.x, c0.y, c0.z, c0.w}, q1 = {c1.x, c1.y, c1.z, c1.w};
    asm volatile("buffer_store_dwordx4 %0, %1, %4, %5 offen nt\n\t"
                 "buffer_store_dwordx4 %2, %3, %4, %5 offen nt\n\t"
                 "s_nop 0"   // a store of more than 64 bits with an SGPR offset: one wait state before its data registers may be rewritten
                 ::"v"(q0), "v"(voff0), "v"(q1), "v"(voff1), "s"(srd), "s"(soff) : "memory");
}

// The pixel store path of a strip.  Per pixel row the strip's BY segments (one per block row, 24 B per block) are 96 chunks of
// 16 B; a lane stores chunk `lane` (and lanes 0..31 also chunk 64 + lane).  Byte offsets relative to the strip's first pixel
// are computed once per strip; the row advance is scalar.  Both store instructions of a row cover whole 128-byte lines
// (segments are 768 or 384 B).
// The strip's rows go through a BUFFER RESOURCE (round 5): base = the strip's first pixel, num_records = the bytes from there to
// the end of the strip's last row INSIDE the image: a row below the image is out of range and the hardware drops its store
// (range check: voffset >= num_records - soffset, tools/probe_buffer.hip); a chunk right of the image gets a voffset that is
// out of range for every row.  No predicate, no branch and no 64-bit address per row: the row is the scalar soffset.
// (num_records <= 32 rows x 3 x 65 535 B: the resource describes a strip, not the image, which may exceed 4 GiB.)
// FAST (W % 16 == 0, 16-byte aligned rows): every chunk is whole or outside.  Otherwise (any width: rows start at any byte
// address, which buffer stores take) a chunk is whole, outside, or -- in the strip column that holds the image's right edge --
// the PARTIAL last chunk of its row segment (1 .. 15 bytes), which goes dword- and byte-wise (store_tail).
// LAUNDER: hide the segment of chunk `lane` from the optimiser (k_luma_fused does, k_quad420 does not: each kernel's measured form).
template <int BX, bool FAST, bool LAUNDER>
struct StripStore {
    static constexpr int BY = 64 / BX, SEG_DW = BX * 6, CPS = SEG_DW / 4;   // dwords / chunks per segment
    int nb;                       // bytes per row segment to write
    uint32_t pitch;
    uint8_t *strip_out;
    uint32_t strip_bytes;
    i32x4_t out_srd;
    int rem0, rem1;               // bytes of the lane's chunks inside the image
    uint32_t base0, base1, voff0, voff1;

    // a: the kernel's arguments (W, H, out, out_stride); the strip at strip row syi, strip column sxi of image img
    template <class Args>
    __device__ __forceinline__ StripStore(const Args &a, int img, int syi, int sxi, int lane)
    {
        const int tile_px = min(BX * 8, a.W - BX * 8 * sxi);    // pixels of this strip inside the image
        nb = 3 * tile_px;
        pitch = 3u * a.W;
        strip_out = a.out + img * a.out_stride + ((size_t)(8 * BY * syi) * a.W + BX * 8 * sxi) * 3;
        int sg0, sg1;   // segments of chunk `lane` and of chunk 64 + lane (the latter for lanes 0..31)
        if constexpr (BX == 32) {   // (lane >= 48 ? 1 : 0, without a select)
            sg0 = 1 + ((lane - 48) >> 31); sg1 = 1;
            if constexpr (LAUNDER) asm volatile("" : "+v"(sg0));
        } else { sg0 = (int)((unsigned)lane / CPS); sg1 = (int)((64u + (unsigned)lane) / CPS); }
        const int j0 = lane - CPS * sg0, j1 = 64 + lane - CPS * sg1;
        // inside the image: 16 j < nb (and, for the second chunk, lane < 32) -- as the SIGN of a difference, so that what depends on it
        // is formed with shifts and v_bfi instead of v_cndmask_b32 (ten times slower than either on gfx950)
        const int in0 = 16 * j0 - nb, in1 = max(16 * j1 - nb, lane - 32);            // negative: inside
        const bool col0 = in0 < 0, col1 = in1 < 0;
        const int rows_here = min(8 * BY, a.H - 8 * BY * syi);
        strip_bytes = (uint32_t)rows_here * pitch;
        out_srd = make_srd(strip_out, strip_bytes);
        rem0 = col0 ? nb - 16 * j0 : 0; rem1 = col1 ? nb - 16 * j1 : 0;
        base0 = sg0 * 8u * pitch + 16u * j0; base1 = sg1 * 8u * pitch + 16u * j1;
        // (d of place(): FAST in0 / in1; else "fewer than 16 bytes of the chunk are inside")
        voff0 = place(base0, FAST ? in0 : in0 + 15); voff1 = place(base1, FAST ? in1 : max(16 * j1 - nb + 15, lane - 32));
    }
    // FAST = false, right-edge column: the first `rem` (1 .. 15) bytes of a chunk -- up to three dwords, then up to three
    // bytes; a lane without a partial chunk carries out-of-range offsets throughout (rem outside 1 .. 15)
    __device__ __forceinline__ void store_tail(const uint4 &v, uint32_t base, int rem, uint32_t soff) const
    {
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(strip_out, 0, (int)strip_bytes, 0x00020000);
        const bool part = rem > 0 && rem < 16;
        const int nd = rem >> 2, nbytes = rem & 3;
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 3; ++k)
            __builtin_amdgcn_raw_buffer_store_b32(d[k], rsrc, (part && k < nd) ? base + 4u * k : 0x80000000u, soff, 0);
        const uint32_t w = nd == 0 ? v.x : nd == 1 ? v.y : nd == 2 ? v.z : v.w;
#pragma unroll
        for (int b = 0; b < 3; ++b)
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(w >> (8 * b)), rsrc, (part && b < nbytes) ? base + 4u * nd + b : 0x80000000u, soff, 0);
    }
    // pixel row yy of every block row of the strip: chunk `lane` from every lane, chunk 64 + lane from lanes 0 .. 31 (the others
    // carry an out-of-range voffset): exactly two store instructions per pixel row, whatever the strip's place in the image
    __device__ __forceinline__ void store_row(int yy, uint4 pv0, uint4 pv1) const
    {
        const uint32_t soff = (uint32_t)yy * pitch;   // scalar
        store_chunk_pair(pv0, voff0, pv1, voff1, out_srd, soff);
        if constexpr (!FAST) {
            if (nb & 15) {   // wave-uniform: this strip column holds the image's right edge
                store_tail(pv0, base0, rem0, soff);
                store_tail(pv1, base1, rem1, soff);
            }
        }
    }
    // Stage the 24 bytes d of a pixel row of the work-item's block (seg, lbx) in the wave's staging row and read the row back
    // as the lane's chunks (LDS operations of one wave execute in order).  The rows are software-pipelined: the chunks are
    // stored (store_row) only after the arithmetic of the next row, right before that row is staged.
    __device__ __forceinline__ void stage_row(const uint32_t (&d)[6], uint32_t *stage_w, int seg, int lbx, int lane, uint4 &pv0, uint4 &pv1) const
    {
        uint2 *sw = reinterpret_cast<uint2 *>(stage_w + seg * SEG_DW + lbx * 6);
        sw[0] = make_uint2(d[0], d[1]);
        sw[1] = make_uint2(d[2], d[3]);
        sw[2] = make_uint2(d[4], d[5]);
        pv0 = *reinterpret_cast<const uint4 *>(stage_w + 4 * lane);
        pv1 = *reinterpret_cast<const uint4 *>(stage_w + 4 * (64 + (lane & 31)));
    }
};

#ifdef JA_PHASE_PROFILE
// development aid (tools/phase_profile.py): wall cycles each wave spends per phase of a strip
constexpr int kPhaseSlots = 16;   // 0..13 phases, 14 the wave's life in shader cycles, 15 in ticks of the 100 MHz counter
// each translation unit that profiles holds its own copy (no relocatable device code): JA_PHASE_STORAGE at namespace scope
#define JA_PHASE_STORAGE                                                                                \
    __device__ unsigned long long g_phase_cycles[4096 * kPhaseSlots];                                   \
    __device__ unsigned long long g_wave_info[4096 * 4];   /* start tick, end tick (100 MHz counter), HW_ID, XCC_ID */
#define JA_PHASE_DECL                                                                                   \
    unsigned long long phase_acc[kPhaseSlots] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};      \
    unsigned long long t_prev = __builtin_readcyclecounter();                                           \
    const unsigned long long t_first = t_prev, r_first = __builtin_amdgcn_s_memrealtime();
#define JA_PHASE(i)                                                       \
    {                                                                     \
        const unsigned long long t_now = __builtin_readcyclecounter();    \
        phase_acc[i] += t_now - t_prev;                                   \
        t_prev = t_now;                                                   \
    }
#define JA_PHASE_FLUSH(slot, lane)                                                                       \
    {                                                                                                    \
        phase_acc[14] = __builtin_readcyclecounter() - t_first;                                          \
        phase_acc[15] = __builtin_amdgcn_s_memrealtime() - r_first;                                      \
        if ((lane) == 0 && (slot) < 4096) {                                                              \
            for (int i_ = 0; i_ < kPhaseSlots; ++i_) g_phase_cycles[(slot) * kPhaseSlots + i_] = phase_acc[i_]; \
            unsigned long long *wi_ = g_wave_info + (slot) * 4;                                          \
            wi_[0] = r_first; wi_[1] = r_first + phase_acc[15];                                          \
            unsigned hw_, xcc_;                                                                          \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_));                            \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));                          \
            wi_[2] = hw_; wi_[3] = xcc_ & 15u;                                                           \
        }                                                                                                \
    }
#else
#define JA_PHASE_STORAGE
#define JA_PHASE_DECL
#define JA_PHASE(i)
#define JA_PHASE_FLUSH(slot, lane)
#endif

}  // namespace jpeg_amd
