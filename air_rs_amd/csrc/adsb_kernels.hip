// adsb_kernels.hip -- gfx950 (MI355X / CDNA4) kernels for the air_rs IQ -> packet path.
//
// What the reference computes per received buffer (src/adsb.rs:95-116), in closed form:
//   m[k]   = floor(sqrt(I^2+Q^2))                                  (src/utils.rs:46-52)
//   gate(i)= min m[i+{0,2,7,9}] >= max m[i+{1,3,4,5,6,8,10..15}]   (src/adsb/demod.rs:23-36)
//            && min m[i+16+{0,3,5,7,8}] >= max m[i+16+{1,2,4,6,9}] (src/adsb/demod.rs:45-54)
//   bit_k  = m[i+16+2k] > m[i+17+2k], k = 0..111, MSB first        (demod.rs:92-131,180-201)
//   s      = CRC24(bytes[0..11]) ^ bytes[11..14]                   (src/adsb/crc.rs:10-40)
//   emit at every i in [0, N-240) where gate(i) and (s == 0 or s is the syndrome of one of the
//   88 data bits, which is then flipped)                            (src/adsb/crc.rs:49-65)
// Every offset is independent (the `_i += 240` at adsb.rs:113 has no effect).
//
// Mapping to the machine (no MFMA: an elementwise / stencil path; HBM-bound by design, VALU-issue-bound as measured --
// DESIGN.md section 5).  A launch is two kernels:
//   demod_tiles (the SCAN: every IQ byte is read once)
//   * one workgroup = one tile of kTile offsets; the tile's raw IQ is read coalesced, 16 B per lane, all loads in flight
//     before the first use, through a bounds-checked buffer descriptor (tails read as zero); which tile a workgroup takes is
//     XCD-aware (tile_of_workgroup: eight contiguous ranges of tiles, one per XCD, so a tile's halo is an L2 hit);
//   * phase 1: magnitudes in registers (v_dot4_i32_i8 -> v_sqrt_f32 -> v_cvt_pk_u8_f32), parked in LDS as u8 (i8 input)
//     or u16 (CS16);
//   * phase 2: the gate runs "transposed": each lane slides along its own run of kRun consecutive offsets, two runs
//     packed in the halves of one VGPR so every min/max is one packed instruction for two offsets (3-input
//     v_pk_maximum3_f16 / v_pk_minimum3_f16 on the magnitudes as f16 bit patterns); running maxima / minima are shared
//     between neighbouring offsets: 8 VALU per step of two offsets; the DF17 part only where some lane of the wave passes
//     the preamble part;
//   * phase 3: the few survivors (LDS bitmap -> unordered list; prefix sums when dense) are sliced by 16-lane groups, one
//     lane per frame byte, straight from the LDS magnitudes; offset + 14 bytes go to the survivor's slot (every tile owns
//     kQuota slots; more come from a shared pool).  No CRC here.
//   finish_order (latency-bound, ~10 us): one LANE per survivor -- CRC-24 by byte table, single-bit repair by binary
//   search of the 88 sorted syndromes, rank inside the tile by DPP rotations, the tile's place from an exchange of
//   per-workgroup counts inside the kernel -- writes the frames in ascending (channel, offset) order, the order the
//   reference's mpsc channel would deliver them in.
// Buffers of at most 32 tiles (the reference's own 20 000-sample buffers) take ONE dispatch (demod_small: the tile body
// per workgroup, the last workgroup to arrive runs the finishing block and writes into pinned host memory).
// This file is the product: one i8 scan (kScanRoot), CS16's, finish_order, the small-buffer kernel and the launchers.  The
// laboratory scans measured against the root scan (kScanNsq, kScanReg, kScanCode, kScanSieve: bit-exact, none faster) live
// in ab/nsq.inc, ab/reg.inc, ab/code.inc and ab/sieve.inc, included in one place below; their kernels are compiled with
// -DADSB_AB_KERNELS=1 only.  They share the root scan's tile prologue and survivor hand-over (tile_prologue, hand_over).
#include <hip/hip_ext.h>
#include <utility>
#include <cstdlib>

#include "adsb_kernels.h"
#include "adsb_synth.h"

namespace adsbk {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// [phase:2 gate: min/max (helpers)]
// ---- small device helpers -------------------------------------------------------------------
__device__ __forceinline__ uint32_t pkmin(uint32_t a, uint32_t b)
{
    u16x2 r = __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b));
    return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ uint32_t pkmax(uint32_t a, uint32_t b)
{
    u16x2 r = __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b));
    return __builtin_bit_cast(uint32_t, r);
}
// Three-input packed max/min.  F16 = every value is below 0x7C00, i.e. a non-negative finite f16 BIT PATTERN
// (denormal or normal), whose numeric order is its integer order: gfx950's v_pk_maximum3_f16 /
// v_pk_minimum3_f16 then reduce three packed pairs in one instruction.  True for i8 input always (magnitudes
// <= 181) and for a CS16 tile whose largest magnitude is below 31744 (checked per tile in phase 1); otherwise
// (CS16 magnitudes reach 46340: infinities, NaNs, negative patterns) two integer v_pk_max_u16 / v_pk_min_u16.
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
template <bool F16> __device__ __forceinline__ uint32_t pkmax3(uint32_t a, uint32_t b, uint32_t c)
{
    if (F16) {
        f16x2 r = __builtin_elementwise_maximum(
            __builtin_elementwise_maximum(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b)),
            __builtin_bit_cast(f16x2, c));
        return __builtin_bit_cast(uint32_t, r);
    }
    return pkmax(pkmax(a, b), c);
}
template <bool F16> __device__ __forceinline__ uint32_t pkmin3(uint32_t a, uint32_t b, uint32_t c)
{
    if (F16) {
        f16x2 r = __builtin_elementwise_minimum(
            __builtin_elementwise_minimum(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b)),
            __builtin_bit_cast(f16x2, c));
        return __builtin_bit_cast(uint32_t, r);
    }
    return pkmin(pkmin(a, b), c);
}

// [phase:1 magnitude (helpers)]  (markers read by tools/isa_slots.py)
// Eight dots per 16-byte load (8 samples) for mags8_i8, as VOP3P v_dot4_i32_i8 with the accumulator c in an SGPR.  Per
// dword x = (I0,Q0,I1,Q1): a = x . (x & 0xFFFF) = c + n0 (masked) and b = x . x = c + n0 + n1 (no mask); the odd sample's
// n1 is their difference, taken inside the packed FMA mags8_i8 pays for anyway: four masks where one dot per sample
// needs eight.  Why asm: for the builtin hipcc picks the VOP2 v_dot4c form, which needs a v_mov per call to preload the
// constant accumulator.  gfx950 needs 3 wait states between a DOT writing a VGPR and a different VALU reading it;
// hipcc pads nothing for asm, so the block ends in s_nop 2 (the eight dots themselves may issue back to back).
__device__ __forceinline__ void dot4x8_pair_sacc(u32x4 v, int c, int a[4], int b[4])
{
    const uint32_t m0 = v.x & 0xFFFFu, m1 = v.y & 0xFFFFu, m2 = v.z & 0xFFFFu, m3 = v.w & 0xFFFFu;
    asm("v_dot4_i32_i8 %0, %8, %12, %16\n\t"
        "v_dot4_i32_i8 %1, %9, %13, %16\n\t"
        "v_dot4_i32_i8 %2, %10, %14, %16\n\t"
        "v_dot4_i32_i8 %3, %11, %15, %16\n\t"
        "v_dot4_i32_i8 %4, %8, %8, %16\n\t"
        "v_dot4_i32_i8 %5, %9, %9, %16\n\t"
        "v_dot4_i32_i8 %6, %10, %10, %16\n\t"
        "v_dot4_i32_i8 %7, %11, %11, %16\n\t"
        "s_nop 2"
        : "=&v"(a[0]), "=&v"(a[1]), "=&v"(a[2]), "=&v"(a[3]), "=&v"(b[0]), "=&v"(b[1]), "=&v"(b[2]), "=&v"(b[3])
        : "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w), "v"(m0), "v"(m1), "v"(m2), "v"(m3), "s"(c));
}

// CRC-24 syndrome table (used by count_candidate only -- tiles that lost their slots are counted in place, a cold
// path; finish_order has its own byte table and sorted syndromes): kSyn[j] = x^(111-j) mod 0x1FFF409, j = 0..111 (bit j
// MSB-first of the 112-bit frame).  XOR over the set bits of a frame is CRC24(data) ^ crc_field; for j < 88 it is
// also the syndrome of a single error in data bit j (the 88 values are distinct and non-zero,
// which is why the reference's ordered brute force, crc.rs:49-65, has at most one match).
struct SynTable {
    uint32_t v[112];
};
constexpr SynTable make_syn()
{
    SynTable t{};
    uint32_t r = 1; // x^0
    for (int e = 0; e < 112; ++e) {
        t.v[111 - e] = r;
        r <<= 1;
        if (r & 0x1000000u) r ^= 0x1FFF409u;
    }
    return t;
}
__constant__ SynTable kSyn = make_syn();

// ---- magnitude ------------------------------------------------------------------------------
// floor(sqrt(n)) for n = I^2+Q^2 <= 32768 (i8 input), exact:
// sqrt(n + 0.5) is at least 1.3e-3 away from every integer for n <= 32768, far more than the
// 1-ulp error of v_sqrt_f32, so truncating it gives floor(sqrt(n)) -- the value the reference
// gets from f64 sqrt + `as u32` (utils.rs:48).  n + 0.5 is formed without an int->float
// convert: the dot product accumulates onto 0x4B000000 (2^23 as float bits), so the integer
// result reinterpreted as float is 2^23 + n, and one subtraction of (2^23 - 0.5) is exact.
// mags8_i8 masks only the even sample of each dword.  With A = 2^23 + n0 (masked dot) and B = 2^23 + n0 + n1
// (whole dword; < 2^24, exact as a float), the odd sample's argument is fma(A, -(1 - 2^-24), B) =
// n1 + 0.5 + n0 * 2^-24 (the product is exact inside the FMA), i.e. n1 + d with d in [0.5, 0.502] before the
// result is rounded (to nearest, or toward zero under MAGMODE 1) onto a grid no coarser than 2^-8.
// floor(sqrt(n + d)) = floor(sqrt(n)) for any d in (0, 1); sqrt(n1 + d) stays 1.376e-3 away from every integer
// (every n1 <= 32768, both roundings, root +-2 ulp: tests/test_pair_dot_model.py), the margin n + 0.5 has.
template <int MAGMODE> __device__ __forceinline__ float mag_root_i8(int n_plus_2p23)
{
    float f = __builtin_bit_cast(float, n_plus_2p23) - 8388607.5f;
    float r = __builtin_amdgcn_sqrtf(f);
    if (MAGMODE == 2) r -= 0.5f; // converter rounds to nearest: land in (k-0.5, k+0.5)
    return r;
}

// 8 consecutive i8 IQ samples (16 bytes) -> 8 magnitudes packed as bytes in two dwords.
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int MAGMODE>
__device__ __forceinline__ void mags8_i8(u32x4 v, uint32_t &lo, uint32_t &hi)
{
    int a[4], b[4];
    dot4x8_pair_sacc(v, 0x4B000000, a, b);
    // two dwords per packed instruction: even samples n0 + 0.5 (v_pk_add_f32), odd samples n1 + 0.5 + n0 * 2^-24
    // (v_pk_fma_f32; see mag_root_i8 for the constants).  Sample 2k is f[2k], sample 2k + 1 is f[2k + 1].
    float f[8];
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
        f32x2 ta = {__builtin_bit_cast(float, a[k]), __builtin_bit_cast(float, a[k + 1])};
        f32x2 tb = {__builtin_bit_cast(float, b[k]), __builtin_bit_cast(float, b[k + 1])};
        f32x2 te = ta - (f32x2){8388607.5f, 8388607.5f};
        f32x2 to = __builtin_elementwise_fma(ta, (f32x2){-0x1.fffffep-1f, -0x1.fffffep-1f}, tb);
        f[2 * k] = te.x;
        f[2 * k + 1] = to.x;
        f[2 * k + 2] = te.y;
        f[2 * k + 3] = to.y;
    }
    float r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        r[k] = __builtin_amdgcn_sqrtf(f[k]);
        if (MAGMODE == 2) r[k] -= 0.5f; // converter rounds to nearest: land in (k-0.5, k+0.5)
    }
    lo = __builtin_amdgcn_cvt_pk_u8_f32(r[0], 0, 0u);
    lo = __builtin_amdgcn_cvt_pk_u8_f32(r[1], 1, lo);
    lo = __builtin_amdgcn_cvt_pk_u8_f32(r[2], 2, lo);
    lo = __builtin_amdgcn_cvt_pk_u8_f32(r[3], 3, lo);
    hi = __builtin_amdgcn_cvt_pk_u8_f32(r[4], 0, 0u);
    hi = __builtin_amdgcn_cvt_pk_u8_f32(r[5], 1, hi);
    hi = __builtin_amdgcn_cvt_pk_u8_f32(r[6], 2, hi);
    hi = __builtin_amdgcn_cvt_pk_u8_f32(r[7], 3, hi);
}

// floor(sqrt(I^2+Q^2)) for one i16 sample (n <= 2^31): n by one v_dot2_i32_i16, a float estimate rounded to
// the nearest integer, and one exact integer correction.
// Error budget of sqrtf((float)n) at s = sqrt(n) <= 46341: conversion to float 2^-24 relative (2^-25 after
// the root), v_sqrt_f32 one ulp (2^-23): |e| <= 46341 * 1.5e-7 < 0.007.  v_cvt_rpi_i32_f32 is floor(x + 0.5),
// so the estimate is floor(s) or floor(s) + 1 (either of them when the fraction of s is within 0.007 of one
// half), and r * r > n tells which (r <= 46341: r * r < 2^32).
// gfx950 does not interlock a transcendental result against the next VALU instruction (one wait state is
// required) and hipcc pads nothing inside or around inline asm: the s_nops in mags4_i16 below are load-bearing.
__device__ __forceinline__ uint32_t mag_i16_fix(uint32_t r, uint32_t n)
{
    return r - ((__umul24(r, r) > n) ? 1u : 0u); // r < 2^24: the 24-bit multiply is exact and full rate
}
// four samples (one 16-byte load) -> two words of packed u16 magnitudes; each group of four like instructions
// issues back to back, which also covers the wait states between a group and the next
__device__ __forceinline__ void mags4_i16(u32x4 v, uint32_t &lo, uint32_t &hi)
{
    uint32_t n0, n1, n2, n3, r0, r1, r2, r3; // n = 2^31 for (-32768, -32768): the i32 result wraps to the right bits
    // (VOP3P form with the inline constant 0 as accumulator: for the builtin hipcc picks v_dot2c, which needs
    // a v_mov per call to preload it; gfx950 wants 3 wait states between a DOT and a VALU reading it)
    asm("v_dot2_i32_i16 %0, %8, %8, 0\n\t"
        "v_dot2_i32_i16 %1, %9, %9, 0\n\t"
        "v_dot2_i32_i16 %2, %10, %10, 0\n\t"
        "v_dot2_i32_i16 %3, %11, %11, 0\n\t"
        "s_nop 2\n\t"
        "v_cvt_f32_u32 %4, %0\n\t"
        "v_cvt_f32_u32 %5, %1\n\t"
        "v_cvt_f32_u32 %6, %2\n\t"
        "v_cvt_f32_u32 %7, %3\n\t"
        "v_sqrt_f32 %4, %4\n\t"
        "v_sqrt_f32 %5, %5\n\t"
        "v_sqrt_f32 %6, %6\n\t"
        "v_sqrt_f32 %7, %7\n\t"
        "v_cvt_rpi_i32_f32 %4, %4\n\t"
        "v_cvt_rpi_i32_f32 %5, %5\n\t"
        "v_cvt_rpi_i32_f32 %6, %6\n\t"
        "s_nop 0\n\t"
        "v_cvt_rpi_i32_f32 %7, %7\n\t"
        "s_nop 0"
        : "=&v"(n0), "=&v"(n1), "=&v"(n2), "=&v"(n3), "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3)
        : "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
    // low halves of two registers into one (one v_perm; the magnitudes are < 2^16)
    lo = __builtin_amdgcn_perm(mag_i16_fix(r1, n1), mag_i16_fix(r0, n0), 0x05040100u);
    hi = __builtin_amdgcn_perm(mag_i16_fix(r3, n3), mag_i16_fix(r2, n2), 0x05040100u);
}

// [phase:end]
// ---- probe: how does v_cvt_pk_u8_f32 round here? --------------------------------------------
__global__ void probe_cvt_kernel(uint32_t *out)
{
    if (threadIdx.x != 0) return;
    float a = 0.75f, b = 2.5f, c = 180.9986f;
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c));
    uint32_t r0 = __builtin_amdgcn_cvt_pk_u8_f32(a, 0, 0u);
    r0 = __builtin_amdgcn_cvt_pk_u8_f32(b, 1, r0);
    r0 = __builtin_amdgcn_cvt_pk_u8_f32(c, 2, r0);
    out[0] = r0;
    // MODE.fp_round: bits [1:0] = f32 rounding; 3 = toward zero
    __builtin_amdgcn_s_setreg((1 | (0 << 6) | ((2 - 1) << 11)), 3);
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c));
    uint32_t r1 = __builtin_amdgcn_cvt_pk_u8_f32(a, 0, 0u);
    r1 = __builtin_amdgcn_cvt_pk_u8_f32(b, 1, r1);
    r1 = __builtin_amdgcn_cvt_pk_u8_f32(c, 2, r1);
    out[1] = r1;
    __builtin_amdgcn_s_setreg((1 | (0 << 6) | ((2 - 1) << 11)), 0);
    out[2] = 0xC0DEu;
    out[3] = 0;
}

hipError_t probe_cvt(hipStream_t s, uint32_t *dev_scratch4, uint32_t host_out[4])
{
    hipLaunchKernelGGL(probe_cvt_kernel, dim3(1), dim3(64), 0, s, dev_scratch4);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(host_out, dev_scratch4, 16, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(s);
}

// ---- the fused tile kernel ------------------------------------------------------------------
template <int ST> struct MagT;
template <> struct MagT<ADSB_SAMPLE_I8> { typedef uint8_t type; };
template <> struct MagT<ADSB_SAMPLE_I16> { typedef uint16_t type; };

template <int ST> struct Lds {
    typedef typename MagT<ST>::type mag_t;
    static constexpr int kMagBytes = (TileCfg<ST>::kMagT * (int)sizeof(mag_t) + 15) & ~15;
    static constexpr int kOffCand = kMagBytes;                 // one word per run of 32 offsets: survivor bitmap
    static constexpr int kOffList = kOffCand + 2 * kThreads * 4 * ((TileCfg<ST>::kRunT + 31) / 32); // kListCap x u16
    static constexpr int kOffMisc = kOffList + kListCap * 2;   // 16 x u32
    static constexpr int kTotal = kOffMisc + 64;
};

// [phase:2 gate: unpack (helpers)]
// Packed pair for sample k of a lane's two runs: low half = run A, high half = run B.
template <int ST>
__device__ __forceinline__ uint32_t pair_at(const uint32_t *ra, const uint32_t *rb, int k)
{
    if (ST == ADSB_SAMPLE_I8) {
        // bytes: [A.k, 0, B.k, 0]; selectors 0-3 pick from the 2nd operand, 4-7 from the 1st
        const uint32_t sel = 0x0C000C00u | (uint32_t)(k & 3) | ((uint32_t)(4 + (k & 3)) << 16);
        return __builtin_amdgcn_perm(rb[k >> 2], ra[k >> 2], sel);
    } else {
        const uint32_t sel = (k & 1) ? 0x07060302u : 0x05040100u;
        return __builtin_amdgcn_perm(rb[k >> 1], ra[k >> 1], sel);
    }
}

// Same value as pair_at with the two source operands exchanged (selectors adjusted): used on the
// rarely taken DF17 path so that hipcc does not merge these with the main path's next-step pair
// and grow a phi (extra exec juggling on every step).
template <int ST>
__device__ __forceinline__ uint32_t pair_at_cold(const uint32_t *ra, const uint32_t *rb, int k)
{
    if (ST == ADSB_SAMPLE_I8) {
        const uint32_t sel = 0x0C000C00u | (uint32_t)(4 + (k & 3)) | ((uint32_t)(k & 3) << 16);
        return __builtin_amdgcn_perm(ra[k >> 2], rb[k >> 2], sel);
    } else {
        const uint32_t sel = (k & 1) ? 0x03020706u : 0x01000504u;
        return __builtin_amdgcn_perm(ra[k >> 1], rb[k >> 1], sel);
    }
}

// [phase:3 decode_candidate: DPP helpers]
// XOR / sum over each row of 16 lanes (a decode group), result in every lane: four DPP steps (VALU
// latency each) instead of four ds_bpermute round trips through the LDS.
#define ADSB_DPP(v, ctrl) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), (ctrl), 0xF, 0xF, true))
__device__ __forceinline__ uint32_t row16_xor(uint32_t v)
{
    v ^= ADSB_DPP(v, 0xB1);  // quad_perm [1,0,3,2]
    v ^= ADSB_DPP(v, 0x4E);  // quad_perm [2,3,0,1]
    v ^= ADSB_DPP(v, 0x141); // row_half_mirror
    v ^= ADSB_DPP(v, 0x140); // row_mirror
    return v;
}

// ---- PPM slice + CRC-24 + single-bit repair of one candidate by a 16-lane group --------------------------
// Lane l slices frame byte l (magnitudes off+16+16l .. +15, demod.rs:97-101).  The 24-byte record
// {offset, bytes[14], status, fixed_bit} is written to `rec` (LDS); returns (on every lane) whether the
// frame is valid (CRC matched, or one data bit repaired: crc.rs:49-65).
// [phase:3 slice_byte (helper; inlined twice)]
// The PPM slice of one frame byte (demod.rs:92-131 + 180-201 in closed form): bit (7-k) = m[16 lb + 2k] > m[16 lb + 2k + 1]
// over the magnitudes off+16+16*lb .. +15 of the tile in LDS; strict, a tie gives 0.
template <int ST>
__device__ __forceinline__ uint32_t slice_byte(const typename MagT<ST>::type *mag, const uint32_t off, const uint32_t lb)
{
    uint32_t byte = 0;
    if (ST == ADSB_SAMPLE_I16) {
        const typename MagT<ST>::type *mp = mag + off + 16 + 16 * lb;
#pragma unroll
        for (int k = 0; k < 8; ++k) // b - a is negative exactly when a > b (magnitudes < 2^16)
            byte |= (((uint32_t)mp[2 * k + 1] - (uint32_t)mp[2 * k]) >> 31) << (7 - k);
    } else {
        const uint32_t pidx = off + 16 + 16 * lb;
        const uint32_t *mw = reinterpret_cast<const uint32_t *>(mag) + (pidx >> 2);
        const uint32_t sh = pidx & 3;
        const uint32_t d0 = mw[0], d1 = mw[1], d2 = mw[2], d3 = mw[3], d4 = mw[4];
        uint32_t w[4] = {__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
                         __builtin_amdgcn_alignbyte(d3, d2, sh), __builtin_amdgcn_alignbyte(d4, d3, sh)};
        // dword k = [a0, b0, a1, b1] holds pairs 2k and 2k+1, bit = (a > b), MSB first: one SDWA byte compare per
        // pair into its own SGPR pair, then byte = byte + byte + carry-in per pair (v_addc): 16 VALU instead of 33 for
        // the packed-subtract form, no v_cndmask (which issues four times slower here).  All eight compares come
        // first: gfx950 wants 2 wait states between a VALU writing an SGPR and a VALU reading it, and hipcc pads
        // nothing inside asm.
        uint64_t m0, m1, m2, m3, m4, m5, m6, m7;
        asm("v_cmp_gt_u32_sdwa %1, %9, %9 src0_sel:BYTE_0 src1_sel:BYTE_1\n\t"
            "v_cmp_gt_u32_sdwa %2, %9, %9 src0_sel:BYTE_2 src1_sel:BYTE_3\n\t"
            "v_cmp_gt_u32_sdwa %3, %10, %10 src0_sel:BYTE_0 src1_sel:BYTE_1\n\t"
            "v_cmp_gt_u32_sdwa %4, %10, %10 src0_sel:BYTE_2 src1_sel:BYTE_3\n\t"
            "v_cmp_gt_u32_sdwa %5, %11, %11 src0_sel:BYTE_0 src1_sel:BYTE_1\n\t"
            "v_cmp_gt_u32_sdwa %6, %11, %11 src0_sel:BYTE_2 src1_sel:BYTE_3\n\t"
            "v_cmp_gt_u32_sdwa %7, %12, %12 src0_sel:BYTE_0 src1_sel:BYTE_1\n\t"
            "v_cmp_gt_u32_sdwa %8, %12, %12 src0_sel:BYTE_2 src1_sel:BYTE_3\n\t"
            "v_addc_co_u32_e64 %0, vcc, %0, %0, %1\n\t"
            "v_addc_co_u32_e64 %0, vcc, %0, %0, %2\n\t"
            "v_addc_co_u32_e64 %0, vcc, %0, %0, %3\n\t"
            "v_addc_co_u32_e64 %0, vcc, %0, %0, %4\n\t"
            "v_addc_co_u32_e64 %0, vcc, %0, %0, %5\n\t"
            "v_addc_co_u32_e64 %0, vcc, %0, %0, %6\n\t"
            "v_addc_co_u32_e64 %0, vcc, %0, %0, %7\n\t"
            "v_addc_co_u32_e64 %0, vcc, %0, %0, %8"
            : "+v"(byte), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3), "=&s"(m4), "=&s"(m5), "=&s"(m6), "=&s"(m7)
            : "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3])
            : "vcc");
    }
    return byte;
}

// [phase:3 count_candidate (tiles without slots only: cold)]
// Slot-store overflow (pathological input): the host re-plans from exact counts, so such a tile's
// survivors are decoded in place only to be COUNTED.  A 16-lane group, one lane per frame byte (`byte` = this
// lane's sliced byte, lanes 14/15 contribute nothing): syndrome = XOR of kSyn over the set bits; valid when it is
// zero or the syndrome of one of the 88 data bits (crc.rs:49-65).  Returns the verdict on every lane of the group.
__device__ __forceinline__ bool count_candidate(const bool have, const uint32_t byte, const uint32_t l, const uint32_t lane)
{
    const uint32_t lb = l < 14 ? l : 13;
    uint32_t s = 0;
    const uint32_t *sy = kSyn.v + 8 * lb;
    const int sb = (int)(l < 14 ? byte : 0u);
#pragma unroll
    for (int k = 0; k < 8; ++k) s ^= sy[k] & (uint32_t)((sb << (24 + k)) >> 31); // mask = -bit k (MSB first)
    s = row16_xor(s);
    int found = -1;
    if (s != 0 && l < 11) {
#pragma unroll
        for (int k = 0; k < 8; ++k) found = (sy[k] == s) ? k : found;
    }
    const unsigned long long fm = __ballot(found >= 0);
    const uint32_t gbits = (uint32_t)(fm >> (lane & 48u)) & 0xFFFFu;
    return have && (s == 0 || gbits != 0);
}

// [phase:end]
// Where a tile sits: global tile id -> channel, first sample, number of valid offsets.
struct TilePos {
    uint32_t ch;
    uint64_t sample0;
    uint32_t n_valid;
};
template <int TILE = kTile>
__device__ __forceinline__ TilePos tile_pos(const DemodArgs &p, uint32_t tile)
{
    TilePos t;
    t.ch = tile / p.tiles_per_channel;
    const uint32_t tch = tile - t.ch * p.tiles_per_channel;
    t.sample0 = (uint64_t)tch * TILE;
    const uint64_t left = (p.n_samples - kWindow) - t.sample0; // offsets 0..n-241 exist (adsb.rs:98)
    t.n_valid = left < (uint64_t)TILE ? (uint32_t)left : (uint32_t)TILE;
    return t;
}

// Bounds-checked descriptor over one tile's samples (+halo): reads past the channel end return 0,
// so ragged tails need no branches.  `tile` must be wave-uniform.
template <int BPS, int MAG = kMag>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const DemodArgs &p, const TilePos &t, bool live = true)
{
    const char *base = (const char *)p.iq + ((uint64_t)t.ch * p.channel_stride + t.sample0) * BPS;
    const uint64_t remain = (p.n_samples - t.sample0) * BPS; // bytes to the end of this channel
    const uint32_t nrec = remain > (uint64_t)(MAG * BPS) ? (uint32_t)(MAG * BPS) : (uint32_t)remain;
    return __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, live ? (int)nrec : 0, 0x00020000);
}

// Diagnostic build (-DADSB_TILE_STAMPS=1; measurement only): lane 0 of waves 0 and 3 of every workgroup store the
// shader cycles (s_memtime) they spent in each segment of a tile to DemodArgs::stamps: 16 u32 per tile (8 per
// wave: prologue up to the loads issued, phase 1 arithmetic, barrier, phase 2, barrier, phase 3, wait for the
// loads, and the low word of s_memrealtime at the start), plain stores at the end of the tile.
#ifndef ADSB_TILE_STAMPS
#define ADSB_TILE_STAMPS 0
#endif
#if ADSB_TILE_STAMPS
#define TSTAMP(k)                                                                                              \
    do {                                                                                                       \
        if ((tid & 63u) == 0 && (wave == 0 || wave == 3)) {                                                    \
            __builtin_amdgcn_sched_barrier(0);                                                                 \
            const unsigned long long now_ = __builtin_amdgcn_s_memtime();                                      \
            if ((k) >= 0) ts_seg[(k)] = (uint32_t)(now_ - ts_prev);                                            \
            ts_prev = now_;                                                                                    \
            __builtin_amdgcn_sched_barrier(0);                                                                 \
        }                                                                                                      \
    } while (0)
#else
#define TSTAMP(k) do { } while (0)
#endif

// The product library carries ONE i8 scan kernel (kScanRoot; x its three magnitude modes) and CS16's.  The kernels round 3 and
// round 4 measured against it -- kScanNsq, kScanReg, kScanCode, kScanSieve (ab/*.inc): all bit-exact, none faster -- are compiled only with
// -DADSB_AB_KERNELS=1 (build.sh puts that build in air_rs_amd/lib/variants/libadsb_hip_ab.so; tests/test_gpu_ab_kernels.py
// runs one parity smoke per kernel through it; tools/gpu/ab.sh times them).
#ifndef ADSB_AB_KERNELS
#define ADSB_AB_KERNELS 0
#endif
bool ab_kernels_built() { return ADSB_AB_KERNELS != 0; }

// survivor bitmap words -> the lane's survivors appended (unordered) to the LDS list, behind a gate's steps: the nsq scan's
// (ab/nsq.inc); gate_phase appends where it finds them
template <int RUN, int NT>
__device__ __forceinline__ void gate_collect(uint32_t *candA, uint32_t *candB, uint16_t *list, uint32_t *count,
                                             const uint32_t tid, const uint32_t n_valid)
{
    constexpr int WPR = (RUN + 31) / 32; // (runs of 16: one word per run, its low half used)
    const uint32_t sa = tid * RUN, sb = (tid + NT) * RUN;
    const uint32_t va = n_valid > sa ? (n_valid - sa) : 0u, vb = n_valid > sb ? (n_valid - sb) : 0u;
    uint32_t words[2 * WPR];
    uint32_t nz = 0, c = 0;
#pragma unroll
    for (int k = 0; k < WPR; ++k) {
        words[k] = candA[k];
        words[WPR + k] = candB[k];
    }
    if (n_valid < (uint32_t)(2 * NT * RUN)) { // (wave-uniform) the ragged last tile of a channel
#pragma unroll
        for (int k = 0; k < WPR; ++k) {
            const uint32_t la = va > 32u * k ? va - 32u * k : 0u, lb = vb > 32u * k ? vb - 32u * k : 0u;
            words[k] &= la >= 32u ? 0xFFFFFFFFu : ((1u << la) - 1u);
            words[WPR + k] &= lb >= 32u ? 0xFFFFFFFFu : ((1u << lb) - 1u);
            candA[k] = words[k]; // the dense path of phase 3 reads the bitmap itself
            candB[k] = words[WPR + k];
        }
    }
#pragma unroll
    for (int k = 0; k < 2 * WPR; ++k) {
        nz |= words[k];
        c += __builtin_popcount(words[k]);
    }
    // Survivors are rare (a handful per tile): the few lanes that have any append their offsets,
    // unordered, to the list (ordering happens later).  The bitmap above is only read if there
    // turn out to be more than kSparseCap.
    if (nz) {
        uint32_t pos = atomicAdd(count, c);
#pragma unroll
        for (int k = 0; k < 2 * WPR; ++k) {
            uint32_t bits = words[k];
            const uint32_t base = (k < WPR ? sa : sb) + (k % WPR) * 32;
            while (bits) {
                const uint32_t b = __builtin_ctz(bits);
                bits &= bits - 1;
                if (pos < (uint32_t)kSparseCap) list[pos] = (uint16_t)(base + b);
                ++pos;
            }
        }
    }
}

// One survivor, appended (unordered) to the LDS list by the lane that found it; *count is the tile's survivor number
// whether or not the list holds them all (more than kSparseCap: phase 3 draws them from the bitmap).
__device__ __forceinline__ void gate_append(uint16_t *list, uint32_t *count, const uint32_t off, const uint32_t n_valid)
{
    if (off < n_valid) { // (offsets at or beyond n_valid do not exist in the reference loop, adsb.rs:98)
        // (the returning LDS add by hand: hipcc's atomicAdd gathers the wave's lanes into one add first, with three more
        // registers than the unrolled steps around this block leave free; a handful of lanes add one each instead)
        uint32_t pos = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)count;
        const uint32_t one = 1u;
        asm volatile("ds_add_rtn_u32 %0, %0, %1\n\ts_waitcnt lgkmcnt(0)" : "+v"(pos) : "v"(one) : "memory");
        if (pos < (uint32_t)kSparseCap) list[pos] = (uint16_t)off;
    }
}

// The ragged last tile of a channel: bits of offsets at or beyond n_valid leave the lane's bitmap words.
template <int RUN, int NT>
__device__ __forceinline__ void gate_mask_tail(uint32_t *candA, uint32_t *candB, const uint32_t tid, const uint32_t n_valid)
{
    constexpr int WPR = (RUN + 31) / 32;
    const uint32_t sa = tid * RUN, sb = (tid + NT) * RUN;
    const uint32_t va = n_valid > sa ? (n_valid - sa) : 0u, vb = n_valid > sb ? (n_valid - sb) : 0u;
#pragma unroll
    for (int k = 0; k < WPR; ++k) {
        const uint32_t la = va > 32u * k ? va - 32u * k : 0u, lb = vb > 32u * k ? vb - 32u * k : 0u;
        candA[k] &= la >= 32u ? 0xFFFFFFFFu : ((1u << la) - 1u);
        candB[k] &= lb >= 32u ? 0xFFFFFFFFu : ((1u << lb) - 1u);
    }
}

// ---- the gate (phase 2 of the tile kernels) --------------------------------------------------
// Preamble + DF17 ordering test (demod.rs:17-57) for the 2 x kRun offsets this lane owns:
// run A = offsets [tid*RUN, +RUN), run B = [(tid+NT)*RUN, +RUN) of the tile whose magnitudes
// are in `mag`.  Survivors are OR-ed into the lane's words of the LDS bitmap `cand` and appended, where they are found,
// unordered, to `list` (their number is added to *count).  `list` and `count` must be LDS: gate_append adds with a DS
// instruction.  No barriers inside; `tid` < NT; 2 NT RUN = kTile.
// [phase:2 gate: set-up]
template <int ST, int RUN, int NT, bool F16OK = (ST == ADSB_SAMPLE_I8)>
__device__ __forceinline__ void gate_phase(const typename MagT<ST>::type *mag, uint32_t *cand, uint16_t *list,
                                           uint32_t *count, const uint32_t tid, const uint32_t n_valid)
{
    static_assert(RUN == 16 || RUN == 32 || RUN == 64, "1 or 2 bitmap words per run");
    constexpr int WPR = (RUN + 31) / 32; // bitmap words per run (a run of 16 uses the low half of its word)
    constexpr int SPG = 16 / (int)sizeof(typename MagT<ST>::type); // magnitudes per 16-byte LDS granule
    // Survivor bitmap: WPR words per run (offset min(RUN, 32) w + b of the tile is bit b of word w), owned by this
    // lane.  The rare path ORs bits straight into LDS so the unrolled steps carry no mask registers.
    uint32_t *candA = cand + WPR * tid, *candB = cand + WPR * (tid + NT);
#pragma unroll
    for (int k = 0; k < WPR; ++k) candA[k] = candB[k] = 0u;
    constexpr int kGran = (RUN + 26 + SPG - 1) / SPG + 1; // granules a run may touch
    const u32x4 *ga = reinterpret_cast<const u32x4 *>(mag + tid * RUN);
    const u32x4 *gb = reinterpret_cast<const u32x4 *>(mag + (tid + NT) * RUN);
    uint32_t ra[kGran * 4], rb[kGran * 4];
    constexpr int kAhead = 48 / SPG; // granules resident ahead of the current block
#pragma unroll
    for (int g = 0; g < kAhead; ++g) {
        u32x4 a = ga[g], b = gb[g];
        ra[4 * g] = a.x; ra[4 * g + 1] = a.y; ra[4 * g + 2] = a.z; ra[4 * g + 3] = a.w;
        rb[4 * g] = b.x; rb[4 * g + 1] = b.y; rb[4 * g + 2] = b.z; rb[4 * g + 3] = b.w;
    }

    // Sliding state shared by neighbouring offsets (all indices are compile-time after
    // unrolling).  With F[j] = max N[j + {0,2,3,4,5}] the twelve low slots of offset o are
    // F[o+1] u F[o+8] u {o+13,14,15}: one new W3, one new F and one 3-input max per offset.
    //   N[j]  sample pair             H2[j] = min(N[j], N[j+2])
    //   W3[j] = max(N[j..j+2])        F[j]  = max(N[j], W3[j+2], N[j+5])
    uint32_t N[RUN + 26], H2[RUN + 8], W3[RUN + 16], F[RUN + 9];
#pragma unroll
    for (int k = 0; k < 25; ++k) N[k] = pair_at<ST>(ra, rb, k);
#pragma unroll
    for (int j = 0; j < 7; ++j) H2[j] = pkmin(N[j], N[j + 2]);
#pragma unroll
    for (int j = 3; j < 13; ++j) W3[j] = pkmax3<F16OK>(N[j], N[j + 1], N[j + 2]);
#pragma unroll
    for (int j = 1; j < 8; ++j) F[j] = pkmax3<F16OK>(N[j], W3[j + 2], N[j + 5]);

    // [phase:2 gate: steps]
    // Every step ends in one wave-uniform test: the common path takes one scalar branch per step (what the
    // many-waves-per-SIMD tile kernel wants: other waves fill the gaps between a step's 8 min/max instructions).
#pragma unroll
    for (int o = 0; o < RUN; ++o) {
        if (o % SPG == 0) { // keep 48 samples resident ahead of the block that starts here
            const int g = o / SPG + kAhead;
            if (g * SPG < RUN + 26) {
                u32x4 a = ga[g], b = gb[g];
                ra[4 * g] = a.x; ra[4 * g + 1] = a.y; ra[4 * g + 2] = a.z; ra[4 * g + 3] = a.w;
                rb[4 * g] = b.x; rb[4 * g + 1] = b.y; rb[4 * g + 2] = b.z; rb[4 * g + 3] = b.w;
            }
        }
        // pairs are unpacked 26 samples ahead so the (rare) DF17 check below finds its ten
        // samples already in registers
        N[o + 25] = pair_at<ST>(ra, rb, o + 25);
        W3[o + 13] = pkmax3<F16OK>(N[o + 13], N[o + 14], N[o + 15]);
        F[o + 8] = pkmax3<F16OK>(N[o + 8], W3[o + 10], N[o + 13]);           // lows 8,10,11,12,13
        const uint32_t lo = pkmax3<F16OK>(F[o + 1], F[o + 8], W3[o + 13]);   // + 1,3,4,5,6 + 13,14,15
        H2[o + 7] = pkmin(N[o + 7], N[o + 9]);
        const uint32_t hi = pkmin(H2[o], H2[o + 7]);                      // highs 0,2,7,9
        const bool pa = (uint16_t)hi >= (uint16_t)lo;
        const bool pb = (hi >> 16) >= (lo >> 16);
        // (the compares' own scalar masks, for the cold block: taken here, next to the compares, they are no instruction)
        const unsigned long long mpa = __builtin_amdgcn_ballot_w64(pa), mpb = __builtin_amdgcn_ballot_w64(pb);
        // [phase:2 gate: DF17 (cold)]
        // wave-uniform test (a scalar branch, no exec juggling; the wave-wide OR is one ballot, an s_or of the compare
        // masks): the block below is entered by the whole wave when any lane passes; its effects are masked by pa/pb anyway
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(pa | pb) != 0, 0)) {
            // DF17 part of the gate (demod.rs:45-54)
            const uint32_t dh = pkmin3<F16OK>(pkmin3<F16OK>(N[o + 16], N[o + 19], N[o + 21]), N[o + 23], N[o + 24]);
            const uint32_t dl = pkmax3<F16OK>(pkmax3<F16OK>(N[o + 17], N[o + 18], N[o + 20]), N[o + 22], N[o + 25]);
            // (the verdicts as scalar masks, ANDed on the scalar side -- a ballot of a combined predicate costs hipcc a
            // v_cndmask and a v_cmp; dh and dl are dead from here, their registers serve the append)
            const unsigned long long sva = mpa & __builtin_amdgcn_ballot_w64((uint16_t)dh >= (uint16_t)dl);
            const unsigned long long svb = mpb & __builtin_amdgcn_ballot_w64((dh >> 16) >= (dl >> 16));
            if (__builtin_expect((sva | svb) != 0, 0)) { // a survivor: about eight times per tile, in one wave
                // (the masks back as lane predicates: an exec mask each, no vector instruction)
                const bool va = __builtin_amdgcn_inverse_ballot_w64(sva), vb = __builtin_amdgcn_inverse_ballot_w64(svb);
                // (offsets at or beyond n_valid are masked out of the bitmap words after the loop, in the one
                // tile per channel that has any; the append tests them itself, one compare executed only here)
                uint32_t bit = 1u << (o & 31);
                asm("" : "+v"(bit)); // one v_mov for both stores (hipcc rematerialises the constant per exec region)
                if (va) atomicOr(candA + (o >> 5), bit);
                if (vb) atomicOr(candB + (o >> 5), bit);
                // (the lane's number taken afresh here: as a product hoisted out of the steps it would hold a
                // register through all of them)
                uint32_t t = tid;
                asm("" : "+v"(t));
                if (va) gate_append(list, count, t * RUN + o, n_valid);
                if (vb) gate_append(list, count, (t + NT) * RUN + o, n_valid);
            }
        }
    }
    // [phase:2 gate: survivor list]
    // The list is complete: every survivor was appended where it was found.  Only the ragged last tile of a channel has
    // anything left to do -- the dense path of phase 3 reads the bitmap itself, so bits at or beyond n_valid leave it.
    if (n_valid < (uint32_t)(2 * NT * RUN)) gate_mask_tail<RUN, NT>(candA, candB, tid, n_valid); // (wave-uniform)
}

// [phase:end]
// Cache policy of the streaming IQ loads: 2 = nt (read once, do not keep): measured 3 % faster than the
// default policy on the 1 GiB buffer (0.233 vs 0.241 ms).
#ifndef ADSB_LOAD_AUX
#define ADSB_LOAD_AUX 2
#endif
// [phase:1 magnitude (loads, stores: helpers)]
// Phase-1 geometry: one 16-byte load = 8 i8 samples or 4 i16 samples per lane; kIters sweeps of the workgroup cover
// the tile + halo (17 for both sample types at the default tile lengths).
template <int ST> struct P1 {
    static constexpr int kSPL = ST == ADSB_SAMPLE_I8 ? 8 : 4;
    static constexpr int kIters = (TileCfg<ST>::kMagT + kThreads * kSPL - 1) / (kThreads * kSPL);
};

// All of a tile's loads are issued at once (nothing is waited for here): 17 x 16 bytes per lane = the whole tile
// in flight.  `live == false` (there is no next tile) clips the descriptor to zero records: the loads return zeros
// without touching memory.  The last sweep only covers the halo: whole waves past it skip it (scalar branch).
template <int ST>
__device__ __forceinline__ void issue_tile_loads(const DemodArgs &p, const TilePos &tp, bool live, uint32_t tid,
                                                 u32x4 (&raw)[P1<ST>::kIters])
{
    constexpr int BPS = (ST == ADSB_SAMPLE_I8) ? 2 : 4;
    __amdgpu_buffer_rsrc_t rsrc = tile_rsrc<BPS, TileCfg<ST>::kMagT>(p, tp, live);
    const uint32_t wave_s0 = __builtin_amdgcn_readfirstlane(tid & ~63u) * P1<ST>::kSPL;
#pragma unroll
    for (int it = 0; it < P1<ST>::kIters; ++it)
        if ((uint32_t)it * (kThreads * P1<ST>::kSPL) + wave_s0 < (uint32_t)TileCfg<ST>::kMagT)
            // (the sweep's constant goes into the SGPR offset -- no per-load VALU address; gfx950 counts it in the
            // descriptor's bounds check: tools/ubench/soffset_probe.hip)
            raw[it] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, tid * 16, (uint32_t)it * (kThreads * 16), ADSB_LOAD_AUX);
}

// raw IQ -> magnitudes in LDS (u8 for i8 input, u16 for i16).  Returns (wave-uniform, CS16 only) whether this wave saw
// a magnitude that is not an ordered f16 bit pattern (>= 0x7C00 = 31744): the gate then takes its integer form.
template <int ST, int MAGMODE>
__device__ __forceinline__ bool magnitudes_to_lds(const u32x4 (&raw)[P1<ST>::kIters], typename MagT<ST>::type *mag, uint32_t tid)
{
    uint32_t mx = 0;
    const uint32_t wave_s0 = __builtin_amdgcn_readfirstlane(tid & ~63u) * P1<ST>::kSPL;
#pragma unroll
    for (int it = 0; it < P1<ST>::kIters; ++it) {
        if ((uint32_t)it * (kThreads * P1<ST>::kSPL) + wave_s0 < (uint32_t)TileCfg<ST>::kMagT) {
            const uint32_t s = (uint32_t)it * (kThreads * P1<ST>::kSPL) + tid * P1<ST>::kSPL;
            uint32_t lo, hi;
            if (ST == ADSB_SAMPLE_I8) mags8_i8<MAGMODE>(raw[it], lo, hi);
            else {
                mags4_i16(raw[it], lo, hi);
                mx = pkmax(mx, pkmax(lo, hi)); // (samples past the channel end read as zero)
            }
            if (s < (uint32_t)TileCfg<ST>::kMagT) *reinterpret_cast<uint2 *>(mag + s) = make_uint2(lo, hi);
        }
    }
    return ST == ADSB_SAMPLE_I16 && __builtin_amdgcn_ballot_w64(((mx & 0xFFFFu) >= 0x7C00u) || ((mx >> 16) >= 0x7C00u)) != 0;
}

// [phase:1 magnitude (loads, stores)]
// The tile prologue of every scan, between the issue of a tile's loads and their first use: the launch's first workgroup
// clears the result header's flags, every workgroup its two LDS counters.
__device__ __forceinline__ void clear_launch_flags(const DemodArgs &p, const bool first, const uint32_t tid)
{
    if (tid == 0 && first) {
        p.hdr->retry = 0;
        if (p.count_groups) { // first pass of a launch: the finishing kernel ORs this launch's flags in
            p.hdr->flags = 0;
            if (p.hdr_pub) p.hdr_pub[2] = 0;
        }
    }
}
__device__ __forceinline__ void tile_prologue(const DemodArgs &p, const bool first, uint32_t *misc, const uint32_t tid)
{
    clear_launch_flags(p, first, tid);
    if (tid == 0) {
        misc[8] = 0;  // valid-frame counter (tiles without slots only)
        misc[12] = 0; // survivor counter
    }
}

// [phase:3 hand-over: slots, offsets, sliced bytes]
// ---- phase 3 of every scan: the survivor hand-over -------------------------------------------------------------------
// Every survivor gets a frame slot, its absolute offset and its 14 sliced bytes (the image is here, in
// LDS).  CRC-24, repair, ordering inside the tile and the valid-frame count are finish_order's work, one
// LANE per survivor instead of sixteen.  (With the whole decode in this kernel a tile's 33 KB of LDS were
// held through a latency-bound epilogue: 19 % of the kernel time for 13 % of its instructions.)

// One record by its 16-lane group, one lane per frame byte: offset + 14 raw bytes (no CRC verdict yet).
__device__ __forceinline__ void put_record(adsb_frame *slot, const uint64_t o64, const uint32_t byte, const uint32_t l)
{
    unsigned char *rec = reinterpret_cast<unsigned char *>(slot);
    if (l < 14) rec[8 + l] = (unsigned char)byte;
    else reinterpret_cast<uint32_t *>(rec)[l - 14] = l == 14 ? (uint32_t)o64 : (uint32_t)(o64 >> 32);
}

// Seg::valid is written by the decode kernel, except for a tile that lost its slots (counted in place)
__device__ __forceinline__ void write_seg(const DemodArgs &p, const uint32_t tile, const uint32_t base_slot, const uint32_t cand,
                                          const uint32_t valid)
{
    Seg e;
    e.base = base_slot;
    e.cand = cand;
    e.valid = valid;
    e.decoded = base_slot == kNoBase ? 1u : 0u;
    p.seg[tile] = e; // (finish_order reads it)
}

// The hand-over of a tile of TILE offsets whose gate left `total` survivors: their bitmap in `cand` (BITS offsets per
// word) and, when there are at most kSparseCap, their offsets, unordered, in `list`.  Call it behind the barrier that
// ends the gate.  `total` = kCountBitmap: there is no list and no count, only the bitmap (the sieve scan's workgroup path).
//   slicer(have, off, l, dropped), called by all lanes of a 16-lane group (l = tid & 15: the lane's place in it; `have` =
//     the group has a survivor, list entry `off`), returns this lane's frame byte -- l < 14: byte l, lanes 14 / 15: any --
//     and sets `dropped` when the samples themselves reject the survivor after all (the code and sieve scans; the record
//     then carries an all-ones offset, which finish_order skips).
//   recheck(list, n), called by the whole workgroup for every chunk of n list entries drawn from the bitmap, before they
//     are sliced (the sieve scan runs its exact gate there and marks entries; it brings its own barrier).
// lane, wave = tid & 63, tid >> 6, which every caller holds already (derived again in here, the CS16 kernel's instructions
// come out in another order).  Writes the tile's Seg: ahead of the slicing when the survivors fit the tile's own slots (nothing in
// this launch reads it; finish_order is a later one), after it otherwise.  Uses misc[0 .. 3], misc[8] (valid frames of a tile without slots), misc[9].
constexpr uint32_t kCountBitmap = 0xFFFFFFFFu;
struct NoRecheck {
    __device__ __forceinline__ void operator()(uint16_t *, uint32_t) const {}
};
template <int TILE, int BITS, class SLICER, class RECHECK = NoRecheck>
__device__ __forceinline__ void hand_over(const DemodArgs &p, const uint32_t tile, const uint64_t sample0, uint32_t total,
                                          const uint32_t *cand, uint16_t *list, uint32_t *misc, const uint32_t tid,
                                          const uint32_t lane, uint32_t wave, SLICER slicer, RECHECK recheck = RECHECK())
{
    // `total` comes out of LDS and `wave` out of tid: both are wave-uniform, which hipcc cannot know.  As scalars, every
    // test on them below is a scalar branch, and a wave without a survivor to slice -- in the normal tile, waves 2 and 3
    // -- leaves on the first of them with no set-up behind it.
    total = __builtin_amdgcn_readfirstlane(total);
    wave = __builtin_amdgcn_readfirstlane(wave);
    const uint64_t abs0 = sample0 + p.offset_base; // absolute offset of this tile's offset 0
    // 16-lane groups slice one survivor each, one lane per frame byte, and store offset + 14 raw bytes
    // into the survivor's slot: 16 survivors per workgroup round
    const uint32_t g = tid >> 4, l = tid & 15;
    auto slice_round = [&](uint32_t slot0, uint32_t ncl) {
        for (uint32_t r = 0; r + 4 * wave < ncl; r += kThreads / 16) { // (later waves: none of their four groups has a survivor)
            const uint32_t ci = r + g;
            const bool have = ci < ncl; // uniform within the 16-lane group
            const uint32_t off = have ? list[ci] : 0u;
            bool dropped;
            const uint32_t byte = slicer(have, off, l, dropped);
            if (have) put_record(p.slots + (size_t)slot0 + ci, dropped ? ~0ull : abs0 + off, byte, l);
        }
    };

    // Frame slots: the tile's own fixed region when the survivors fit (no atomics), otherwise one allocation from the
    // shared pool.  In the usual case (a handful of survivors) every thread knows the base without asking tid 0, and the
    // list is complete since the barrier that ended the gate: no further barrier.
    if (total <= kQuota) {
        if (tid == 0) write_seg(p, tile, tile * kQuota, total, misc[8]);
        slice_round(tile * kQuota, total); // unordered list (finish_order ranks it): survivor j -> slot j
        return;
    }

    const bool dense = total > (uint32_t)kSparseCap;
    u32x4 cw = {0, 0, 0, 0};
    uint32_t cnt = 0, my_first = 0;
    if (dense) {
        // dense fallback: ordered compaction of the bitmap by workgroup-wide prefix sums
        // bitmap: offset BITS w + b of the tile is bit b of word w; words 4*tid .. 4*tid+3 per thread
        if (4 * tid < (uint32_t)(TILE / BITS)) cw = reinterpret_cast<const u32x4 *>(cand)[tid];
        cnt = __builtin_popcount(cw.x) + __builtin_popcount(cw.y) + __builtin_popcount(cw.z) +
              __builtin_popcount(cw.w);
        uint32_t incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            uint32_t t = __shfl_up(incl, d, 64);
            if ((int)lane >= d) incl += t;
        }
        if (lane == 63) misc[wave] = incl;
        __syncthreads();
        uint32_t wbase = 0;
        total = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            uint32_t t = misc[w];
            wbase += (w < (int)wave) ? t : 0u;
            total += t;
        }
        my_first = wbase + incl - cnt; // index of this thread's first candidate
        total = __builtin_amdgcn_readfirstlane(total);
    }

    // more than the tile's quota, or drawn from the bitmap: one allocation from the shared pool
    if (tid == 0) {
        const unsigned long long b64 = atomicAdd(&p.hdr->alloc, (unsigned long long)total);
        // (pool_off: test knob, adsb_debug_pool_limit -- every tile over its quota loses its slots)
        misc[9] = (!p.pool_off && b64 + total <= (unsigned long long)p.cap_slots) ? p.pool_first + (uint32_t)b64 : kNoBase;
    }
    __syncthreads();
    const uint32_t base_slot = misc[9];
    for (uint32_t chunk = 0; chunk < total; chunk += kListCap) {
        if (dense && cnt) {
            uint32_t idx = my_first;
            const uint32_t words[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t bits = words[k];
                while (bits) {
                    const uint32_t b = __builtin_ctz(bits);
                    bits &= bits - 1;
                    if (idx >= chunk && idx < chunk + kListCap)
                        list[idx - chunk] = (uint16_t)((4 * tid + k) * BITS + b);
                    ++idx;
                }
            }
        }
        __syncthreads();
        const uint32_t ncl = (total - chunk) < (uint32_t)kListCap ? (total - chunk) : (uint32_t)kListCap;
        if (dense) recheck(list, ncl);
        if (base_slot != kNoBase) {
            slice_round(base_slot + chunk, ncl); // (ordered when dense; 33..64 survivors: unordered like the simple case)
        } else {
            // The slot store is full (pathological input: SURVEY F8).  The host re-plans from exact counts,
            // so this tile's survivors are decoded HERE, from the image in LDS, only to be counted.
            for (uint32_t r = 0; r + 4 * wave < ncl; r += kThreads / 16) { // (later waves: none of their four groups has a candidate)
                const uint32_t ci = r + g;
                const bool have = ci < ncl; // uniform within the 16-lane group
                const uint32_t off = have ? list[ci] : 0u;
                bool dropped;
                const uint32_t byte = slicer(have, off, l, dropped);
                const bool valid = count_candidate(have && !dropped, byte, l, lane);
                if (valid && l == 0) atomicAdd(&misc[8], 1u);
            }
        }
        __syncthreads();
    }
    if (tid == 0) write_seg(p, tile, base_slot, total, misc[8]);
}

// [phase:end]
// demod_tiles: one workgroup = one tile; the hardware dispatcher starts the next tile as soon as one retires, which
// staggers the phases of a CU's co-resident workgroups.  Per tile:
//   phase 1  the tile's raw IQ (16-byte loads, all in flight at once) becomes the LDS image: floor(sqrt)
//            magnitudes (u8 / u16);                                                                         ... barrier
//   phase 2  preamble + DF17 gate over the tile's offsets (gate_phase);                                     ... barrier
//   phase 3  every survivor gets a frame slot, its offset and its 14 sliced bytes; CRC-24, repair and ordering are
//            finish_order's (below).
// Measured alternatives: persistent workgroups drawing tiles from per-XCD ticket counters with
// the next tile's loads issued before phase 3 run the same tile in ~10 % more VALU instructions (loop-carried
// registers, SGPR spills) and come out 7 % slower; several tiles per workgroup with the next tile's loads in flight
// need 147 VGPRs (3 waves per SIMD): 0.25-0.27 ms against 0.182.  The instruction count is what bounds this kernel.
// Waves per SIMD the register allocation is held to = workgroups per CU the LDS image allows (4 waves per workgroup):
// 8 for the i8 root scan (u8 magnitudes: 19 KB), ADSB_SCAN_WAVES for the 16-bit images (CS16; the nsq scan, ab/nsq.inc).
#ifndef ADSB_SCAN_WAVES
#define ADSB_SCAN_WAVES 4
#endif
// The tile body: everything one workgroup does for one tile (`first` = it is the launch's first workgroup: it clears
// the result header's flags).  smem: Lds<ST>::kTotal bytes, 16-byte aligned.
template <int ST, int MAGMODE>
__device__ __forceinline__ void scan_tile(const DemodArgs &p, const uint32_t tile, const bool first, unsigned char *smem)
{
    typedef Lds<ST> L;
    typedef TileCfg<ST> TC; // tile length of this sample type
    typedef typename L::mag_t mag_t;
    static_assert(kThreads / 64 <= 4, "misc[4 + wave] must stay below misc[8]");

    mag_t *mag = reinterpret_cast<mag_t *>(smem);
    uint32_t *cand = reinterpret_cast<uint32_t *>(smem + L::kOffCand);
    uint16_t *list = reinterpret_cast<uint16_t *>(smem + L::kOffList);
    uint32_t *misc = reinterpret_cast<uint32_t *>(smem + L::kOffMisc);

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63, wave = tid >> 6;

    if (MAGMODE == 1) __builtin_amdgcn_s_setreg((1 | (0 << 6) | ((2 - 1) << 11)), 3);
#if ADSB_TILE_STAMPS
    unsigned long long ts_prev = 0;
    uint32_t ts_seg[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    ts_seg[7] = (uint32_t)__builtin_amdgcn_s_memrealtime();
    TSTAMP(-1);
    ts_seg[8] = (uint32_t)ts_prev; // s_memtime next to the s_memrealtime above: the shader clock under this load
#endif
    {
        const TilePos tp = tile_pos<TC::kTileT>(p, tile);
        const uint64_t sample0 = tp.sample0;
        const uint32_t n_valid = tp.n_valid;
        // [phase:1 magnitude (loads, stores)]
        // ---- phase 1, first half: the loads go out before anything else --------------------------------------------
        u32x4 raw[P1<ST>::kIters];
        issue_tile_loads<ST>(p, tp, true, tid, raw);
        TSTAMP(0); // prologue, loads issued
        tile_prologue(p, first, misc, tid);
#if ADSB_TILE_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // (diagnostic build only) the whole wait for the loads ...
        TSTAMP(6);                                       // ... as its own segment
#endif
        // ---- phase 1, second half: raw IQ -> the LDS image ---------------------------------------------------
        const bool wave_big = magnitudes_to_lds<ST, MAGMODE>(raw, mag, tid);
        if (ST == ADSB_SAMPLE_I16 && lane == 0) misc[4 + wave] = wave_big ? 1u : 0u; // (every wave writes its own word)
        TSTAMP(1); // phase 1 arithmetic
        __syncthreads();
        TSTAMP(2); // barrier

        // [phase:2 gate: call]
        // ---- phase 2: preamble + DF17 gate, two runs per lane, packed u16x2 --------------------
        if constexpr (ST == ADSB_SAMPLE_I16) {
            // the 3-input f16 gate whenever every value of the tile is an ordered f16 pattern (any signal below 2/3 of
            // full scale); the integer gate otherwise
            uint32_t any_big = 0;
#pragma unroll
            for (int w = 0; w < kThreads / 64; ++w) any_big |= misc[4 + w];
            const bool big = any_big != 0; // (workgroup-uniform)
            if (!big) gate_phase<ST, TC::kRunT, kThreads, true>(mag, cand, list, &misc[12], tid, n_valid);
            else gate_phase<ST, TC::kRunT, kThreads, false>(mag, cand, list, &misc[12], tid, n_valid);
        } else {
            gate_phase<ST, TC::kRunT, kThreads>(mag, cand, list, &misc[12], tid, n_valid);
        }
        TSTAMP(3); // phase 2
        __syncthreads();
        TSTAMP(4); // barrier

        // [phase:3 hand-over: slots, offsets, sliced bytes]
        // ---- phase 3: PPM slice of the gate survivors; the CRC stage is a kernel of its own --------------------
        constexpr int kBitsPerWord = TC::kRunT < 32 ? TC::kRunT : 32; // offsets per survivor-bitmap word (gate_phase)
        hand_over<TC::kTileT, kBitsPerWord>(p, tile, sample0, misc[12], cand, list, misc, tid, lane, wave,
                                            [=](const bool, const uint32_t off, const uint32_t l, bool &dropped) {
                                                dropped = false; // (the magnitudes are exact: the gate's verdict stands)
                                                return slice_byte<ST>(mag, off, l < 14 ? l : 13);
                                            });
        TSTAMP(5); // phase 3
#if ADSB_TILE_STAMPS
        if ((tid & 63u) == 0 && (wave == 0 || wave == 3)) {
            uint32_t *dst = reinterpret_cast<uint32_t *>(p.stamps) + (size_t)tile * 16 + (wave ? 8 : 0);
#pragma unroll
            for (int k = 0; k < 8; ++k) dst[k] = ts_seg[k];
            if (wave) dst[6] = ts_seg[8]; // wave 3's load wait is wave 0's: its slot carries the s_memtime stamp
        }
#endif
    }
    // [phase:end]
    if (MAGMODE == 1) __builtin_amdgcn_s_setreg((1 | (0 << 6) | ((2 - 1) << 11)), 0);
}

// Which tile a workgroup takes.  The dispatcher deals workgroups to the eight XCDs round-robin (workgroup b runs on XCD b mod 8:
// tools/ubench/xcc_probe.hip reads HW_REG_XCC_ID in every workgroup, profiles/r04_xcc_probe.txt)
// and each XCD has its own L2: with tile = b, a tile's 240-sample halo -- the first samples of the NEXT tile -- is fetched by two
// different XCDs, i.e. twice from HBM (FETCH_SIZE = 1.016 x the buffer for i8, 1.031 x for CS16: exactly the halos).  With the
// launch's tiles cut into eight contiguous ranges, XCD x walking range x in order, neighbouring tiles run on the same XCD at about
// the same time and the halo is an L2 hit.  (n = 8 q + r tiles: XCD x owns q + (x < r) of them, starting at x q + min(x, r); b =
// 8 j + x < n picks the j-th.)
#ifndef ADSB_XCD_MAP
#define ADSB_XCD_MAP 1
#endif
__device__ __forceinline__ uint32_t tile_of_workgroup(uint32_t b, uint32_t n)
{
#if ADSB_XCD_MAP
    const uint32_t q = n >> 3, r = n & 7u, x = b & 7u, j = b >> 3;
    return x * q + (x < r ? x : r) + j;
#else
    (void)n;
    return b;
#endif
}

template <int ST, int MAGMODE>
__global__ __launch_bounds__(kThreads, ST == ADSB_SAMPLE_I8 ? 8 : ADSB_SCAN_WAVES) void demod_tiles(DemodArgs p)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[Lds<ST>::kTotal];
    scan_tile<ST, MAGMODE>(p, p.tile_first + tile_of_workgroup(blockIdx.x, p.tile_count), blockIdx.x == 0, smem);
}

// ---- CRC-24 + single-bit repair of the sliced survivors (demod.rs:71-81; crc.rs:10-65) --------------------------
// Byte-wise table of the Mode-S CRC-24 (generator 0x1FFF409, MSB first, init 0, no final XOR: crc.rs:10-40):
// kCrcTab[v] = (v * x^24) mod G.  crc' = (crc << 8) ^ kCrcTab[(crc >> 16) ^ byte] over the 11 data bytes.
struct CrcTable {
    uint32_t v[256];
};
constexpr CrcTable make_crc_table()
{
    CrcTable t{};
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t r = i << 16;
        for (int k = 0; k < 8; ++k) {
            r <<= 1;
            if (r & 0x1000000u) r ^= 0x1FFF409u;
        }
        t.v[i] = r & 0xFFFFFFu;
    }
    return t;
}
__constant__ CrcTable kCrcTab = make_crc_table();
// The 88 data-bit syndromes sorted, (syndrome << 7) | bit index, padded to 128 entries: the single-bit repair of
// crc.rs:49-65 (at most one of the 88 distinct non-zero values matches) as a 7-step binary search.
struct SynSorted {
    uint32_t v[128];
};
constexpr SynSorted make_syn_sorted()
{
    SynSorted t{};
    SynTable sy = make_syn();
    for (int j = 0; j < 128; ++j) t.v[j] = j < 88 ? ((sy.v[j] << 7) | (uint32_t)j) : 0xFFFFFFFFu;
    for (int i = 1; i < 128; ++i) { // insertion sort (constant evaluation)
        uint32_t x = t.v[i];
        int k = i - 1;
        while (k >= 0 && t.v[k] > x) {
            t.v[k + 1] = t.v[k];
            --k;
        }
        t.v[k + 1] = x;
    }
    return t;
}
__constant__ SynSorted kSynSorted = make_syn_sorted();

// finish_order: the second (and last) kernel of a launch.  The scan kernel (demod_tiles) left, per tile, `Seg{base,
// cand}` and, in the slots base .. base+cand-1, every gate survivor's absolute offset and 14 sliced bytes (unordered when
// cand <= kSparseCap, ascending otherwise).  This kernel checks them (CRC-24 over the 11 data bytes, byte-wise with a
// 1 KB table in LDS; a non-zero syndrome is looked up among the 88 data-bit syndromes and that bit flipped, crc.rs:49-65:
// a flip in the CRC field itself never matches) AND puts the valid frames into the final list in ascending (channel,
// offset) order -- the order the reference's mpsc channel delivers them in (adsb.rs:98-111).  Rounds 1-2 did this in two
// kernels (finish_candidates + gather_tiles: 16.5 + 5.9 us at 32 768 tiles, plus a dispatch gap); fused, every record is
// read once, finished in registers and written once, to its final place:
//   * one workgroup (4 waves) takes 32 consecutive tiles; a wave takes 4 tiles per pass, 16 lanes each, ONE LANE per
//     survivor (a tile has ~8 survivors; tiles with more than 16 take the whole wave afterwards);
//   * the lane's place inside its tile = its rank by offset among the tile's valid frames (15 DPP row rotations);
//   * the tile's place in the list = valid frames in all earlier tiles.  Counts are reduced per workgroup; every
//     workgroup publishes its aggregate in one 8-byte word {value | flag | epoch of the launch} (never cleared: a word
//     of another epoch reads as "not there yet"), the last workgroup of every 64 also publishes the sum of its 64, and
//     a workgroup's start is the sum of the (at most 63) aggregates before it in its own 64 plus the sums of all earlier
//     64s: two dependent round trips of wave-wide loads, whatever the grid size; up to 1024 workgroups (1 GiB of i8 IQ)
//     every workgroup simply sums all aggregates before it, one round trip (a chained look-back degenerates here:
//     all workgroups reach it at the same moment, and the last one would walk N/64 windows one after the other; a
//     ticket counter for arrival order costs 12 us by itself at 88 tickets per microsecond on one address);
//   * a workgroup only ever waits for workgroups with a LOWER block index, and the lowest unfinished block is always
//     resident (each XCD's dispatcher walks its share of the grid in order), so the waits end; a lane that still
//     finds nothing after ~0.1 s gives up and reports it (Header::retry bit 2 -> ADSB_E_STATE on the host) instead of
//     hanging the device;
//   * the last workgroup knows the total: it writes the header and re-arms the pool.
// A re-run of lost tiles (slot-pool overflow, host-planned positions in `out_start`) uses the same kernel without the
// exchange.
constexpr int kFinTiles = 32;          // tiles per workgroup
constexpr int kFinThreads = 256;
constexpr int kFinFan = 64;            // workgroups per second-level sum
constexpr int kFinFlat = 1024;         // up to this many workgroups exchange their aggregates in one level
constexpr int kFinSumsPerRound = 64 * 8; // second-level sums a wave reads at a time: eight loads per lane
constexpr uint32_t kLbReady = 1u;      // exchange word: value[31:0] | flag[33:32] | epoch[63:34]
constexpr uint32_t kLbSpinLimit = 1u << 21; // polls (with s_sleep) before a lane gives up: ~0.1 s

// CRC-24 + single-bit repair of one record per lane (w = the record as loaded; straight-line code, no branches, so
// that the chains of a wave's four tiles interleave): returns whether the frame is valid; w comes back finished
// (repaired bit flipped, status and fixed_bit filled in).
__device__ __forceinline__ bool finish_record(uint32_t (&w)[6], const bool have, const uint32_t *crc_tab, const uint32_t *syn_sorted)
{
    // frame byte i is record byte 8 + i: dword 2 + (i >> 2), byte (i & 3)
    uint32_t crc = 0;
#pragma unroll
    for (int i = 0; i < 11; ++i) {
        const uint32_t b = (w[2 + (i >> 2)] >> (8 * (i & 3))) & 0xFFu;
        crc = ((crc << 8) ^ crc_tab[((crc >> 16) ^ b) & 0xFFu]) & 0xFFFFFFu;
    }
    const uint32_t rx = ((w[4] >> 24) << 16) | ((w[5] & 0xFFu) << 8) | ((w[5] >> 8) & 0xFFu); // frame bytes 11, 12, 13
    const uint32_t sm = crc ^ rx;
    uint32_t pos = 0; // binary search: first entry whose syndrome is >= sm
#pragma unroll
    for (int step = 64; step >= 1; step >>= 1)
        pos += ((syn_sorted[pos + step - 1] >> 7) < sm) ? (uint32_t)step : 0u;
    const uint32_t hit = syn_sorted[pos];
    const bool found = sm != 0 && (hit >> 7) == sm;
    const bool valid = have && (sm == 0 || found);
    const bool fix = valid && sm != 0;
    const uint32_t fixed = fix ? (hit & 0x7Fu) : 0xFFu;          // data bit 0..87, MSB first
    const uint32_t status = valid ? (sm == 0 ? 0u : 1u) : 0xFFu;
    const uint32_t bi = 8u + ((hit & 0x7Fu) >> 3);               // record byte of that bit
    const uint32_t flip = fix ? ((0x80u >> (hit & 7u)) << (8u * (bi & 3u))) : 0u;
    const uint32_t wi = bi >> 2;                                 // 2, 3 or 4
    w[2] ^= wi == 2 ? flip : 0u;
    w[3] ^= wi == 3 ? flip : 0u;
    w[4] ^= wi == 4 ? flip : 0u;
    w[5] = (w[5] & 0xFFFFu) | (status << 16) | (fixed << 24);
    return valid;
}


template <int N> __device__ __forceinline__ uint32_t row_ror(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x120 + N /* row_ror:N */, 0xF, 0xF, true);
}
// number of lanes of this lane's 16-lane row whose key is smaller than its own (keys of lanes that do not count are
// >= 0x10000, above every key that does)
__device__ __forceinline__ uint32_t row_rank(uint32_t key)
{
    uint32_t below = 0;
#define ADSB_RANK_STEP(N) below += row_ror<N>(key) < key ? 1u : 0u;
    ADSB_RANK_STEP(1) ADSB_RANK_STEP(2) ADSB_RANK_STEP(3) ADSB_RANK_STEP(4) ADSB_RANK_STEP(5)
    ADSB_RANK_STEP(6) ADSB_RANK_STEP(7) ADSB_RANK_STEP(8) ADSB_RANK_STEP(9) ADSB_RANK_STEP(10)
    ADSB_RANK_STEP(11) ADSB_RANK_STEP(12) ADSB_RANK_STEP(13) ADSB_RANK_STEP(14) ADSB_RANK_STEP(15)
#undef ADSB_RANK_STEP
    return below;
}

__device__ __forceinline__ void store_record(adsb_frame *dst, const uint32_t (&w)[6])
{
    uint2 *d = reinterpret_cast<uint2 *>(dst);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = make_uint2(w[2 * k], w[2 * k + 1]);
}
__device__ __forceinline__ void load_record(const adsb_frame *src, uint32_t (&w)[6])
{
    const uint2 *s2 = reinterpret_cast<const uint2 *>(src);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint2 v = s2[k];
        w[2 * k] = v.x;
        w[2 * k + 1] = v.y;
    }
}

// A tile with more than 16 survivors, by a whole wave: finished records go back to the tile's slots in offset order
// (ranked when they arrived unordered, i.e. cand <= kSparseCap; more arrive in order); returns its valid count.
__device__ __forceinline__ uint32_t finish_big_tile(const FinishArgs &a, const Seg &e, const uint32_t *crc_tab,
                                                    const uint32_t *syn_sorted, uint32_t lane)
{
    uint32_t n_good = 0;
    for (uint32_t chunk = 0; chunk < e.cand; chunk += 64) {
        const uint32_t nc = (e.cand - chunk) < 64u ? (e.cand - chunk) : 64u;
        uint32_t w[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0, 0};
        if (lane < nc) load_record(a.slots + (size_t)e.base + chunk + lane, w);
        // (offset all ones: a survivor of the code gate that the samples themselves rejected -- no record)
        const bool valid = finish_record(w, lane < nc && w[1] != 0xFFFFFFFFu, crc_tab, syn_sorted);
        uint32_t slot = lane;
        if (e.cand <= (uint32_t)kSparseCap) { // one chunk, unordered: rank by offset (wrap-safe: a tile spans < 2^15)
            // keys: offset relative to some record's (within 2^15 either way) for records; above them and distinct for rejected
            // ones, so that every lane gets a slot of its own
            const bool rec = lane < nc && w[1] != 0xFFFFFFFFu;
            const unsigned long long rm = __ballot(rec);
            const uint32_t ref = rm ? (uint32_t)__builtin_amdgcn_readlane((int)w[0], (int)__builtin_ctzll(rm)) : 0u;
            const int32_t mine = rec ? (int32_t)(w[0] - ref) : (int32_t)(0x40000000u + lane);
            uint32_t below = 0;
            for (uint32_t k = 0; k < nc; ++k) {
                const int32_t other = (int32_t)__builtin_amdgcn_readlane((int)mine, (int)k);
                below += other < mine ? 1u : 0u;
            }
            slot = below;
        }
        if (lane < nc) store_record(a.slots + (size_t)e.base + chunk + slot, w);
        n_good += (uint32_t)__builtin_popcountll(__ballot(valid));
    }
    return n_good;
}

constexpr int kFinLdsWords = 256 + 128 + 2 * kFinTiles; // tables, per-tile counts, per-tile positions
// What workgroup `blk` of `n_blk` does (lds: kFinLdsWords words).
// PUB_ATOMIC: the caller-owned header copy's flags word is updated with 64-bit atomic ORs (device memory: finish_order).  The
// small-buffer kernel, whose copy lives in pinned HOST memory, passes false and publishes the flags itself with one plain
// store at the end (atomics over PCIe are a platform option, not a given).
template <bool PUB_ATOMIC = true>
__device__ __forceinline__ void finish_block(const FinishArgs &a, const uint32_t blk, const uint32_t n_blk, uint32_t *lds)
{
    uint32_t *crc_tab = lds, *syn_sorted = lds + 256;
    uint32_t *counts = lds + 384;            // valid frames per tile of this workgroup
    uint32_t *tpos = lds + 384 + kFinTiles;  // position of each tile's first frame in the final list
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, sub = lane & 15;
    const uint32_t tile0 = a.tile_first + blk * kFinTiles, t_end = a.tile_first + a.tile_count;

    // ---- this wave's 8 tiles, 4 per pass: one lane per survivor ------------------------------------------------------
    // One memory round trip for everything the lane needs: the tile's Seg AND, without waiting for it, the record at
    // the place a small tile's survivor `sub` is known to be (a tile with at most kQuota survivors keeps them in its
    // own fixed slots, tile * kQuota + i: demod_tiles), next to the tables' words.
    Seg e[2];
    uint32_t w[2][6], rank[2];
    bool valid[2], small_[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const uint32_t idx = wave * 8 + p * 4 + g, tile = tile0 + idx;
        e[p].base = kNoBase; e[p].cand = 0; e[p].valid = 0; e[p].decoded = 1;
        w[p][0] = w[p][1] = 0xFFFFFFFFu;
        w[p][2] = w[p][3] = w[p][4] = w[p][5] = 0;
        if (tile < t_end) {
            e[p] = a.seg[tile];
            load_record(a.slots + (size_t)tile * kQuota + sub, w[p]);
        }
    }
    for (uint32_t i = tid; i < 256 + 128; i += kFinThreads) {
        if (i < 256) crc_tab[i] = kCrcTab.v[i];
        else syn_sorted[i - 256] = kSynSorted.v[i - 256];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const bool live = e[p].cand != 0 && e[p].base != kNoBase && !e[p].decoded;
        small_[p] = live && e[p].cand <= 16u; // (then base == tile * kQuota: what was loaded above is its record)
        if (!(small_[p] && sub < e[p].cand)) {
            w[p][0] = w[p][1] = 0xFFFFFFFFu;
            w[p][2] = w[p][3] = w[p][4] = w[p][5] = 0;
        }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const uint32_t idx = wave * 8 + p * 4 + g;
        // (offset all ones: a survivor of the code gate that the samples themselves rejected -- no record)
        valid[p] = finish_record(w[p], small_[p] && sub < e[p].cand && w[p][1] != 0xFFFFFFFFu, crc_tab, syn_sorted);
        // place inside the tile: rank by offset among the valid frames of the 16-lane row.  A tile's offsets lie within
        // 2^15 of each other: relative to the row's first survivor they fit 16 bits (wrap-safe); bit 16 = does not count.
        // (relative to the row's first RECORD: a rejected survivor's all-ones offset is no reference)
        const uint32_t recs = (uint32_t)(__ballot(w[p][1] != 0xFFFFFFFFu) >> (16u * g)) & 0xFFFFu;
        const uint32_t ref = (uint32_t)__shfl((int)w[p][0], (int)((lane & 48u) + (recs ? (uint32_t)__builtin_ctz(recs) : 0u)), 64);
        const uint32_t key = valid[p] ? ((w[p][0] - ref + 0x8000u) & 0xFFFFu) : 0x10000u;
        rank[p] = row_rank(key);
        const uint32_t cnt = (uint32_t)__builtin_popcount((uint32_t)(__ballot(valid[p]) >> (16u * g)) & 0xFFFFu);
        if (sub == 0) counts[idx] = small_[p] ? cnt : (e[p].decoded ? e[p].valid : 0u); // (a tile the scan had to count itself keeps its count)
    }
    // tiles with more than 16 survivors (coarse or constant input): the whole wave, one tile after the other.  Which
    // ones: a 2 x 4-bit mask from the Seg entries the rows already hold (no further loads on the usual path)
    uint32_t big_mask = 0;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const bool big = e[p].cand > 16u && e[p].base != kNoBase && !e[p].decoded;
        const unsigned long long m = __ballot(big && sub == 0); // bits 0, 16, 32, 48: rows 0..3
        big_mask |= (uint32_t)(((m >> 0) & 1u) | ((m >> 15) & 2u) | ((m >> 30) & 4u) | ((m >> 45) & 8u)) << (4 * p);
    }
    for (uint32_t left = big_mask; left; left &= left - 1) { // (wave-uniform)
        const uint32_t i = (uint32_t)__builtin_ctz(left), idx = wave * 8 + i;
        const Seg eb = a.seg[tile0 + idx];
        const uint32_t n_good = finish_big_tile(a, eb, crc_tab, syn_sorted, lane);
        if (lane == 0) counts[idx] = n_good;
    }
    __syncthreads();

    // ---- where this workgroup's frames start: prefix inside the workgroup + look-back over the earlier ones ----------
    if (wave == 0) {
        const uint32_t c = lane < (uint32_t)kFinTiles ? counts[lane] : 0u;
        uint32_t incl = c;
#pragma unroll
        for (int d = 1; d < kFinTiles; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d, 64);
            if ((int)lane >= d) incl += t;
        }
        const uint32_t total = __shfl(incl, kFinTiles - 1, 64);
        unsigned long long before = 0; // valid frames in all earlier workgroups
        if (a.out_start == nullptr) {
            const unsigned long long tag = ((unsigned long long)a.epoch << 34) | ((unsigned long long)kLbReady << 32);
            uint64_t *lb_a = a.lb, *lb_s = a.lb + a.lb_groups_at; // one word per workgroup | one per 64 workgroups
            if (lane == 0 && blk != a.stall_blk) __hip_atomic_store(lb_a + blk, tag | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t grp = blk / kFinFan, r = blk % kFinFan;
            bool failed = false;
            auto wave_sum = [&](unsigned long long x) {
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    const uint32_t lo = __shfl_xor((uint32_t)x, d, 64), hi32 = __shfl_xor((uint32_t)(x >> 32), d, 64);
                    x += ((unsigned long long)hi32 << 32) | lo;
                }
                return x;
            };
            if (n_blk <= (uint32_t)kFinFlat) {
                // small grids (up to 1024 workgroups = 1 GiB of i8 IQ): one level -- every aggregate before this one, 16
                // independent loads per lane in flight at once, re-read until all carry the tag: ONE exchange round trip
                unsigned long long acc;
                uint32_t spins = 0;
                bool ok;
                do {
                    unsigned long long v[kFinFlat / 64];
#pragma unroll
                    for (int u = 0; u < kFinFlat / 64; ++u) {
                        const uint32_t k = (uint32_t)u * 64u + lane;
                        v[u] = k < blk ? __hip_atomic_load(lb_a + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : tag;
                    }
                    acc = 0;
                    ok = true;
#pragma unroll
                    for (int u = 0; u < kFinFlat / 64; ++u) {
                        ok = ok && (v[u] >> 32) == (tag >> 32);
                        acc += v[u] & 0xFFFFFFFFull;
                    }
                    if (!__all(ok)) {
                        __builtin_amdgcn_s_sleep(2);
                        if (++spins > kLbSpinLimit) { failed = true; ok = true; acc = 0; }
                    }
                } while (!__all(ok));
                before = wave_sum(acc);
            } else {
                // two levels: the aggregates before this one inside its 64 (one per lane) and the sums of the earlier 64s
                // (lane l takes l, l + 64, ...; published by workgroups with lower indices than this one).  Both sets of
                // loads are in flight together and re-read until they carry the tag: one round trip when the others are
                // ahead, as they mostly are -- not one per level and per 64 earlier sums.  The last of a 64 publishes its
                // 64's sum as soon as its own in-group words are complete (it does not wait for the earlier 64s: no chain).
                unsigned long long in_grp = 0, earlier = 0;
                bool in_done = false, e_done = grp == 0;
                uint32_t spins = 0;
                do {
                    unsigned long long vi = tag, e_acc = 0;
                    bool e_ok = true;
                    if (!in_done && lane < r) vi = __hip_atomic_load(lb_a + (size_t)grp * kFinFan + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (!e_done) {
                        for (uint32_t k0 = 0; k0 < grp; k0 += (uint32_t)kFinSumsPerRound) { // (wave-uniform trip count; eight loads per lane at a time)
                            unsigned long long v[kFinSumsPerRound / 64];
#pragma unroll
                            for (int u = 0; u < kFinSumsPerRound / 64; ++u) {
                                const uint32_t k = k0 + (uint32_t)u * 64u + lane;
                                v[u] = k < grp ? __hip_atomic_load(lb_s + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : tag;
                            }
#pragma unroll
                            for (int u = 0; u < kFinSumsPerRound / 64; ++u) {
                                e_ok = e_ok && (v[u] >> 32) == (tag >> 32);
                                e_acc += v[u] & 0xFFFFFFFFull;
                            }
                        }
                    }
                    if (!in_done && __all((vi >> 32) == (tag >> 32))) {
                        in_grp = wave_sum(vi & 0xFFFFFFFFull);
                        in_done = true;
                        if (r == kFinFan - 1 && lane == 0) { // the last of its 64 publishes their sum (a 64's frames fit 32 bits)
                            const unsigned long long sum64 = in_grp + total;
                            __hip_atomic_store(lb_s + grp, tag | (sum64 > 0xFFFFFFFFull ? 0xFFFFFFFFull : sum64), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
                    if (!e_done && __all(e_ok)) {
                        earlier = wave_sum(e_acc);
                        e_done = true;
                    }
                    if (!(in_done && e_done)) {
                        __builtin_amdgcn_s_sleep(2);
                        if (++spins > kLbSpinLimit) { failed = true; in_done = e_done = true; in_grp = earlier = 0; }
                    }
                } while (!(in_done && e_done));
                before = in_grp + earlier;
            }
            if (__any(failed) && lane == 0) { // gave up waiting: the host returns ADSB_E_STATE; device-side consumers see a list with holes
                atomicOr(&a.hdr->retry, 4u);
                atomicOr(&a.hdr->flags, ADSB_FLAG_INCOMPLETE);
                if (PUB_ATOMIC && a.hdr_pub) atomicOr(reinterpret_cast<unsigned long long *>(a.hdr_pub + 2), (unsigned long long)ADSB_FLAG_INCOMPLETE);
            }
            if (blk == n_blk - 1 && lane == 0) { // the last workgroup: the whole launch's total is known here
                const unsigned long long tot = before + total, n_out = tot < a.max_out ? tot : a.max_out;
                a.hdr->total_found = tot;
                a.hdr->n_out = n_out;
                // flags were cleared by the scan kernel; bits are OR-ed in (another workgroup may add INCOMPLETE)
                if (tot > a.max_out) atomicOr(&a.hdr->flags, ADSB_FLAG_TRUNCATED);
                a.hdr->alloc = 0; // pool allocator: ready for the next launch
                if (a.hdr_pub) {
                    a.hdr_pub[0] = n_out;
                    a.hdr_pub[1] = tot;
                    if (PUB_ATOMIC && tot > a.max_out) atomicOr(reinterpret_cast<unsigned long long *>(a.hdr_pub + 2), (unsigned long long)ADSB_FLAG_TRUNCATED);
                    a.hdr_pub[3] = 0;
                }
                if (a.chan_prefix) a.chan_prefix[a.n_channels] = tot;
            }
        }
        if (lane < (uint32_t)kFinTiles) {
            const uint32_t tile = tile0 + lane;
            unsigned long long pos = before + (incl - c);
            if (a.out_start) pos = tile < t_end ? a.out_start[tile] : 0xFFFFFFFFu;
            const uint32_t p32 = pos > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)pos;
            tpos[lane] = p32;
            if (tile < t_end) {
                // frames before each channel's first tile (adsb_fetch turns them into per-channel counts)
                if (a.chan_prefix && tile % a.tiles_per_channel == 0) a.chan_prefix[tile / a.tiles_per_channel] = pos;
            }
        }
    }
    __syncthreads();

    // ---- every frame to its place -------------------------------------------------------------------------------------
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const uint32_t idx = wave * 8 + p * 4 + g, tile = tile0 + idx;
        const uint32_t dst = tpos[idx] + rank[p];
        if (valid[p] && dst < a.max_out && tpos[idx] != 0xFFFFFFFFu) store_record(a.out + dst, w[p]);
        if (sub == 0 && tile < t_end) {
            if (small_[p]) a.seg[tile].valid = counts[idx];
            // a tile that lost its slots (the pool was full) but whose frames are wanted: the host re-plans
            if (e[p].base == kNoBase && e[p].cand != 0 && counts[idx] != 0 && tpos[idx] < a.max_out && a.out_start == nullptr) {
                atomicOr(&a.hdr->retry, 1u);
                atomicOr(&a.hdr->flags, ADSB_FLAG_INCOMPLETE); // visible to device-side consumers: the list has holes
                if (PUB_ATOMIC && a.hdr_pub) atomicOr(reinterpret_cast<unsigned long long *>(a.hdr_pub + 2), (unsigned long long)ADSB_FLAG_INCOMPLETE);
            }
        }
    }
    for (uint32_t left = big_mask; left; left &= left - 1) { // the big tiles' valid frames, from their slots (offset order), by the whole wave
        const uint32_t i = (uint32_t)__builtin_ctz(left), idx = wave * 8 + i, tile = tile0 + idx;
        const Seg eb = a.seg[tile];
        if (lane == 0) a.seg[tile].valid = counts[idx];
        uint32_t pos = tpos[idx];
        if (pos >= a.max_out) continue;
        for (uint32_t i0 = 0; i0 < eb.cand; i0 += 64) {
            const uint32_t k = i0 + lane;
            uint32_t x[6] = {0, 0, 0, 0, 0, 0xFF0000u};
            if (k < eb.cand) load_record(a.slots + (size_t)eb.base + k, x);
            const bool ok = k < eb.cand && ((x[5] >> 16) & 0xFFu) != 0xFFu;
            const unsigned long long m = __ballot(ok);
            const uint32_t dst = pos + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
            if (ok && dst < a.max_out) store_record(a.out + dst, x);
            pos += (uint32_t)__builtin_popcountll(m);
        }
    }
}

__global__ __launch_bounds__(kFinThreads) void finish_order(FinishArgs a)
{
    __shared__ uint32_t lds[kFinLdsWords];
    finish_block<true>(a, blockIdx.x, gridDim.x, lds);
}

void finish_geometry(uint32_t *tiles_per_workgroup, uint32_t *fan, uint32_t *flat, uint32_t *sums_per_round)
{
    if (tiles_per_workgroup) *tiles_per_workgroup = kFinTiles;
    if (fan) *fan = kFinFan;
    if (flat) *flat = kFinFlat;
    if (sums_per_round) *sums_per_round = kFinSumsPerRound;
}

hipError_t launch_finish(hipStream_t s, const FinishArgs &a, hipEvent_t e0, hipEvent_t e1)
{
    const uint32_t blocks = (a.tile_count + kFinTiles - 1) / kFinTiles;
    if (blocks == 0) return hipSuccess;
    hipExtLaunchKernelGGL(finish_order, dim3(blocks), dim3(kFinThreads), 0, s, e0, e1, 0, a);
    return hipGetLastError();
}

// ---- the laboratory scans (A/B: bit-exact, none faster) -------------------------------------------------------------
// Each file holds one scan: image layout, loads, gate, slicer, scan_tile_*, its kernel (-DADSB_AB_KERNELS=1 only) and its
// private knobs.  (The device bodies and the two probe kernels the C ABI exposes in every build are always compiled.)
#include "ab/nsq.inc"
#include "ab/reg.inc"
#include "ab/code.inc"
#include "ab/sieve.inc"

// ---- small buffers: scan + finish in ONE dispatch, results straight into host memory --------------------------------------
// A buffer of at most kFinTiles tiles (the reference's own buffers: 20 000 samples = 2 tiles, adsb.rs:77-79; an SDR's MTU-
// sized reads, adsb.rs:59-64) is not worth three host calls per kernel and a copy each way: one workgroup per tile runs the
// tile body, the workgroup that finishes LAST (a counter in device memory; agent-scope release / acquire around it) runs
// the finishing block over all tiles, writes header and frames through the caller's pointer -- pinned host memory the
// device can write -- and then, behind a system-scope fence, a sequence number the host polls.  The samples are read
// from pinned host memory the same way.  Per buffer the host makes ONE call (the launch).
static_assert(kFinThreads == kThreads, "the small-buffer kernel runs both bodies in one workgroup shape");
template <int ST, int MAGMODE, int SCAN>
__global__ __launch_bounds__(kThreads, 4) void demod_small(DemodArgs p, FinishArgs f, SmallArgs sm)
{
    constexpr int kScanBytes = SCAN == kScanSieve ? SieveLds::kTotal : SCAN == kScanReg ? RegLds::kTotal : SCAN == kScanCode ? CodeLds::kTotal : SCAN == kScanNsq ? NsqLds::kTotal : Lds<ST>::kTotal, kFinBytes = kFinLdsWords * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem[kScanBytes > kFinBytes ? kScanBytes : kFinBytes];
    __shared__ uint32_t last_flag;
    if constexpr (SCAN == kScanSieve) scan_tile_sieve(p, p.tile_first + blockIdx.x, blockIdx.x == 0, smem);
    else if constexpr (SCAN == kScanReg) scan_tile_reg(p, p.tile_first + blockIdx.x, blockIdx.x == 0, smem);
    else if constexpr (SCAN == kScanCode) scan_tile_code(p, p.tile_first + blockIdx.x, blockIdx.x == 0, smem);
    else if constexpr (SCAN == kScanNsq) scan_tile_nsq(p, p.tile_first + blockIdx.x, blockIdx.x == 0, smem);
    else scan_tile<ST, MAGMODE>(p, p.tile_first + blockIdx.x, blockIdx.x == 0, smem);
    // hand-off to whichever workgroup arrives last (cdna_hip_programming.md Guideline 16: every storing wave drains its
    // stores, the workgroup's barrier, one lane's agent-scope release, then the counter; the reader acquires)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t prev = __hip_atomic_fetch_add(sm.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_flag = prev == gridDim.x - 1 ? 1u : 0u;
        if (last_flag) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!last_flag) return;
    finish_block<false>(f, 0, 1, reinterpret_cast<uint32_t *>(smem));
    // everything is written (list and header, through f.out / f.hdr_pub): tell the host
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        // the flags this workgroup's lanes OR-ed into the device header, to the host copy by ONE plain store
        if (f.hdr_pub) f.hdr_pub[2] = (uint64_t)__hip_atomic_load(&f.hdr->flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *sm.done = 0; // re-armed for the next launch on this result set
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");      // system scope: the host reads what this kernel wrote
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(sm.seq_host, sm.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

hipError_t launch_small(hipStream_t s, int sample_type, int mag_mode, int scan, const DemodArgs &p, const FinishArgs &f,
                        const SmallArgs &sm)
{
    if (p.tile_count == 0 || p.tile_count > (uint32_t)kFinTiles) return hipErrorInvalidValue;
    dim3 grid(p.tile_count), block(kThreads);
    if (sample_type == ADSB_SAMPLE_I16) hipLaunchKernelGGL((demod_small<ADSB_SAMPLE_I16, 0, kScanRoot>), grid, block, 0, s, p, f, sm);
#if ADSB_AB_KERNELS
    else if (scan == kScanSieve) hipLaunchKernelGGL((demod_small<ADSB_SAMPLE_I8, 0, kScanSieve>), grid, block, 0, s, p, f, sm);
    else if (scan == kScanNsq) hipLaunchKernelGGL((demod_small<ADSB_SAMPLE_I8, 0, kScanNsq>), grid, block, 0, s, p, f, sm);
    else if (scan == kScanReg) hipLaunchKernelGGL((demod_small<ADSB_SAMPLE_I8, 0, kScanReg>), grid, block, 0, s, p, f, sm);
    else if (scan == kScanCode) hipLaunchKernelGGL((demod_small<ADSB_SAMPLE_I8, 0, kScanCode>), grid, block, 0, s, p, f, sm);
#else
    else if (scan != kScanRoot) return hipErrorInvalidValue; // (the A/B kernels are not in this build)
#endif
    else if (mag_mode == 0) hipLaunchKernelGGL((demod_small<ADSB_SAMPLE_I8, 0, kScanRoot>), grid, block, 0, s, p, f, sm);
    else if (mag_mode == 1) hipLaunchKernelGGL((demod_small<ADSB_SAMPLE_I8, 1, kScanRoot>), grid, block, 0, s, p, f, sm);
    else hipLaunchKernelGGL((demod_small<ADSB_SAMPLE_I8, 2, kScanRoot>), grid, block, 0, s, p, f, sm);
    return hipGetLastError();
}

// No tiles at all (a 240-sample buffer: adsb.rs:98 iterates 0..0), or a measurement launch without the finishing
// kernel: the header of an empty list.
__global__ void empty_result_kernel(Header *hdr, uint64_t *hdr_pub, uint64_t *chan_prefix, uint32_t n_channels)
{
    if (threadIdx.x == 0) {
        hdr->n_out = 0;
        hdr->total_found = 0;
        hdr->flags = 0;
        hdr->retry = 0;
        hdr->alloc = 0;
        if (hdr_pub) { hdr_pub[0] = 0; hdr_pub[1] = 0; hdr_pub[2] = 0; hdr_pub[3] = 0; }
    }
    if (chan_prefix)
        for (uint32_t k = threadIdx.x; k <= n_channels; k += blockDim.x) chan_prefix[k] = 0;
}
hipError_t launch_empty_result(hipStream_t s, Header *hdr, uint64_t *hdr_pub, uint64_t *chan_prefix, uint32_t n_channels,
                               hipEvent_t e0, hipEvent_t e1)
{
    hipExtLaunchKernelGGL(empty_result_kernel, dim3(1), dim3(64), 0, s, e0, e1, 0, hdr, hdr_pub, chan_prefix, n_channels);
    return hipGetLastError();
}

template <int ST>
static hipError_t launch_demod_st(hipStream_t s, int mag_mode, const DemodArgs &a, uint32_t grid_x,
                                  hipEvent_t e0, hipEvent_t e1)
{
    dim3 grid(grid_x), block(kThreads);
    if (ST == ADSB_SAMPLE_I16) mag_mode = 0; // the CS16 magnitude chain does not depend on the converter's rounding
    switch (mag_mode) {
    case 0: hipExtLaunchKernelGGL((demod_tiles<ST, 0>), grid, block, 0, s, e0, e1, 0, a); break;
    case 1: hipExtLaunchKernelGGL((demod_tiles<ST, ST == ADSB_SAMPLE_I8 ? 1 : 0>), grid, block, 0, s, e0, e1, 0, a); break;
    default: hipExtLaunchKernelGGL((demod_tiles<ST, ST == ADSB_SAMPLE_I8 ? 2 : 0>), grid, block, 0, s, e0, e1, 0, a); break;
    }
    return hipGetLastError();
}

bool tile_stamps_built() { return ADSB_TILE_STAMPS != 0; }

hipError_t launch_demod(hipStream_t s, int sample_type, int mag_mode, int scan, const DemodArgs &a,
                        hipEvent_t e0, hipEvent_t e1)
{
    if (a.tile_count == 0) return hipSuccess;
#if ADSB_AB_KERNELS
    if (sample_type == ADSB_SAMPLE_I8 && scan == kScanSieve) {
        uint32_t grid = a.tile_count;
        if (kSievePersistent) { // (A/B) four workgroups per CU, each loops over its share of the tiles
            static int sieve_slots = 0;
            if (sieve_slots == 0) {
                int dev = 0, cus = 0;
                if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
                sieve_slots = cus * 4;
            }
            if (grid > (uint32_t)sieve_slots) grid = (uint32_t)sieve_slots;
        }
        hipExtLaunchKernelGGL(demod_tiles_sieve, dim3(grid), dim3(kThreads), 0, s, e0, e1, 0, a);
        return hipGetLastError();
    }
    if (sample_type == ADSB_SAMPLE_I8 && scan == kScanNsq) {
        hipExtLaunchKernelGGL(demod_tiles_nsq, dim3(a.tile_count), dim3(kThreads), 0, s, e0, e1, 0, a);
        return hipGetLastError();
    }
    if (sample_type == ADSB_SAMPLE_I8 && scan == kScanReg) {
        hipExtLaunchKernelGGL(demod_tiles_reg, dim3(a.tile_count), dim3(kThreads), 0, s, e0, e1, 0, a);
        return hipGetLastError();
    }
    if (sample_type == ADSB_SAMPLE_I8 && scan == kScanCode) {
        hipExtLaunchKernelGGL(demod_tiles_code, dim3(a.tile_count), dim3(kThreads), 0, s, e0, e1, 0, a);
        return hipGetLastError();
    }
#else
    if (sample_type == ADSB_SAMPLE_I8 && scan != kScanRoot) return hipErrorInvalidValue; // (the A/B kernels are not in this build)
#endif
    if (sample_type == ADSB_SAMPLE_I8) return launch_demod_st<ADSB_SAMPLE_I8>(s, mag_mode, a, a.tile_count, e0, e1);
    return launch_demod_st<ADSB_SAMPLE_I16>(s, 0, a, a.tile_count, e0, e1);
}

// ---- field decode (what AdsbPacket::new computes, src/adsb/packet.rs:25-49) -----------------------
// One thread per frame; 32-byte records.  Integer bit-field work, bound by the 24 + 32 bytes moved
// per frame (a few MB per launch): a latency-bound epilogue, not a hot kernel.
__constant__ char kIcaoCharset[65] = "#ABCDEFGHIJKLMNOPQRSTUVWXYZ#####_###############0123456789######"; // msgs.rs:172-177

__global__ __launch_bounds__(256) void decode_fields_kernel(const adsb_frame *frames, const Header *hdr,
                                                           uint32_t cap, adsb_packet_fields *out)
{
    const uint64_t n64 = hdr ? hdr->n_out : cap;
    const uint32_t n = n64 < cap ? (uint32_t)n64 : cap;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(frames + i); // bytes[] start at byte 8
    uint8_t b[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t v = w[2 + k];
        b[4 * k] = v & 0xFF; b[4 * k + 1] = (v >> 8) & 0xFF; b[4 * k + 2] = (v >> 16) & 0xFF; b[4 * k + 3] = v >> 24;
    }
    adsb_packet_fields f;
    f.icao = ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
    f.downlink_format = b[0] >> 3;
    f.capability = b[0] & 5;          // sic: the reference masks with 5 (packet.rs:27)
    f.msg_type = b[4] >> 3;
    f.altitude = 0; f.cpr_latitude = 0; f.cpr_longitude = 0;
    f.surveillance_status = 0; f.nic_supplement = 0; f.cpr_time = 0; f.cpr_odd = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) f.callsign[k] = 0;
    const uint8_t *m = b + 4;         // the 7-byte ME field, packet[4..11]
    if (f.msg_type >= 1 && f.msg_type <= 4) {           // msgs.rs:210-212
        f.msg_kind = 0;
        unsigned long long bits = 0;
#pragma unroll
        for (int k = 1; k < 7; ++k) bits = (bits << 8) | m[k];
#pragma unroll
        for (int c = 0; c < 8; ++c) f.callsign[c] = kIcaoCharset[(bits >> (42 - 6 * c)) & 0x3F];
    } else if (f.msg_type >= 9 && f.msg_type <= 18) {   // msgs.rs:122-124
        f.msg_kind = 1;
        const int code = ((int)(m[1] >> 1) << 4) | (m[2] >> 4);
        f.altitude = code * ((m[1] & 1) ? 25 : 100) - 1000;
        f.surveillance_status = (m[0] >> 1) & 3;
        f.nic_supplement = m[0] & 1;
        f.cpr_time = (m[2] >> 3) & 1;
        f.cpr_odd = (m[2] >> 2) & 1;
        f.cpr_latitude = ((uint32_t)(m[2] & 3) << 15) | ((uint32_t)m[3] << 7) | (m[4] >> 1);
        f.cpr_longitude = ((uint32_t)(m[4] & 1) << 16) | ((uint32_t)m[5] << 8) | m[6];
    } else {
        f.msg_kind = 2;
    }
    out[i] = f;
}

hipError_t launch_decode_fields(hipStream_t s, const adsb_frame *frames, const Header *hdr, uint32_t cap,
                                adsb_packet_fields *out)
{
    if (cap == 0) return hipSuccess;
    hipLaunchKernelGGL(decode_fields_kernel, dim3((cap + 255) / 256), dim3(256), 0, s, frames, hdr, cap, out);
    return hipGetLastError();
}

// ---- test / measurement kernels -----------------------------------------------------------------
template <int ST, int MAGMODE>
__global__ void magnitudes_kernel(const void *iq, size_t n, uint16_t *out)
{
    if (MAGMODE == 1) __builtin_amdgcn_s_setreg((1 | (0 << 6) | ((2 - 1) << 11)), 3);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    if (ST == ADSB_SAMPLE_I8) {
        // 8 samples per thread-step through the same code path as the tile kernel
        const size_t groups = (n + 7) / 8;
        for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
            u32x4 v = {0, 0, 0, 0};
            const uint16_t *src = reinterpret_cast<const uint16_t *>(iq) + g * 8;
            uint16_t tmp[8];
            for (int k = 0; k < 8; ++k) tmp[k] = (g * 8 + k < n) ? src[k] : (uint16_t)0;
            v.x = tmp[0] | ((uint32_t)tmp[1] << 16);
            v.y = tmp[2] | ((uint32_t)tmp[3] << 16);
            v.z = tmp[4] | ((uint32_t)tmp[5] << 16);
            v.w = tmp[6] | ((uint32_t)tmp[7] << 16);
            uint32_t lo, hi;
            mags8_i8<MAGMODE>(v, lo, hi);
            for (int k = 0; k < 8; ++k)
                if (g * 8 + k < n) out[g * 8 + k] = (uint16_t)(((k < 4 ? lo : hi) >> (8 * (k & 3))) & 0xFFu);
        }
    } else {
        // 4 samples per thread-step through the same code path as the tile kernel
        const size_t groups = (n + 3) / 4;
        for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(iq) + g * 4;
            uint32_t tmp[4];
            for (int k = 0; k < 4; ++k) tmp[k] = (g * 4 + k < n) ? src[k] : 0u;
            u32x4 v = {tmp[0], tmp[1], tmp[2], tmp[3]};
            uint32_t lo, hi;
            mags4_i16(v, lo, hi);
            for (int k = 0; k < 4; ++k)
                if (g * 4 + k < n) out[g * 4 + k] = (uint16_t)((k < 2 ? lo : hi) >> (16 * (k & 1)));
        }
    }
    if (MAGMODE == 1) __builtin_amdgcn_s_setreg((1 | (0 << 6) | ((2 - 1) << 11)), 0);
}

hipError_t launch_magnitudes(hipStream_t s, int sample_type, int mag_mode, const void *iq, size_t n,
                             uint16_t *out)
{
    if (n == 0) return hipSuccess;
    dim3 grid(1024), block(256);
    if (sample_type == ADSB_SAMPLE_I16) {
        hipLaunchKernelGGL((magnitudes_kernel<ADSB_SAMPLE_I16, 0>), grid, block, 0, s, iq, n, out);
    } else if (mag_mode == 0) {
        hipLaunchKernelGGL((magnitudes_kernel<ADSB_SAMPLE_I8, 0>), grid, block, 0, s, iq, n, out);
    } else if (mag_mode == 1) {
        hipLaunchKernelGGL((magnitudes_kernel<ADSB_SAMPLE_I8, 1>), grid, block, 0, s, iq, n, out);
    } else {
        hipLaunchKernelGGL((magnitudes_kernel<ADSB_SAMPLE_I8, 2>), grid, block, 0, s, iq, n, out);
    }
    return hipGetLastError();
}

// Pure streaming read: LOADS loads of 16 bytes per lane, all in flight before the first use, `nt` policy, one workgroup per
// LOADS x 4 KB; the values are only XOR-ed.  What this box's HBM delivers to a kernel that does nothing else with the bytes.  No
// single shape is the fastest on every box and size (tools/ubench/read_shapes.hip, profiles/r04_read_shapes.txt: 6.8-7.1 TB/s
// at 1 GiB, 7.0-7.2 at 16 GiB; the 16-load shape in plain workgroup order, the only one until round 4, is the slowest at 1 GiB
// by 3-4 %), so adsb_time_read_ceiling times three -- shape 0: 4 loads, 1: 8 loads, 2: 16 loads with the chunks dealt to
// workgroups in eight contiguous ranges like the scan's tiles -- and reports the fastest.
template <int LOADS, bool XCD>
__global__ __launch_bounds__(256) void read_only_kernel(const u32x4 *buf, size_t n16, uint32_t n_wg, uint32_t *sink)
{
    const uint32_t b = XCD ? tile_of_workgroup(blockIdx.x, n_wg) : blockIdx.x;
    const size_t base = (size_t)b * (256 * LOADS) + threadIdx.x;
    u32x4 v[LOADS];
#pragma unroll
    for (int k = 0; k < LOADS; ++k) {
        const size_t i = base + (size_t)k * 256;
        v[k] = i < n16 ? __builtin_nontemporal_load(buf + i) : u32x4{0u, 0u, 0u, 0u};
    }
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < LOADS; ++k) acc ^= v[k].x ^ v[k].y ^ v[k].z ^ v[k].w;
    if (acc == 0x9E3779B9u) *sink = acc; // practically never: keeps the loads alive
}

hipError_t launch_read_only(hipStream_t s, const void *buf, size_t bytes, uint32_t *sink, int shape)
{
    const size_t n16 = bytes / 16;
    if (n16 == 0) return hipSuccess;
    const int loads = shape == 0 ? 4 : shape == 1 ? 8 : 16;
    const size_t per_wg = (size_t)256 * loads;
    const uint32_t n_wg = (uint32_t)((n16 + per_wg - 1) / per_wg);
    const u32x4 *b = reinterpret_cast<const u32x4 *>(buf);
    if (shape == 0) hipLaunchKernelGGL((read_only_kernel<4, false>), dim3(n_wg), dim3(256), 0, s, b, n16, n_wg, sink);
    else if (shape == 1) hipLaunchKernelGGL((read_only_kernel<8, false>), dim3(n_wg), dim3(256), 0, s, b, n16, n_wg, sink);
    else if (shape == 2) hipLaunchKernelGGL((read_only_kernel<16, true>), dim3(n_wg), dim3(256), 0, s, b, n16, n_wg, sink);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// Synthetic source: one thread per sample (untimed; clarity over speed).
constexpr uint32_t kSynthBlocks = 256 * 16, kSynthThreads = 256; // the whole grid; longer ranges go round the loop

uint32_t synth_geometry() { return kSynthBlocks * kSynthThreads; }

template <int ST>
__global__ void synth_kernel(adsb_synth_cfg cfg, uint32_t channel, uint64_t first, size_t n, void *iq)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
        const uint64_t k = first + j;
        const uint64_t slot = k / cfg.slot_len;
        int vi, vq;
        adsb_synth::noise_iq(cfg, channel, k, vi, vq);
        // only samples inside a frame's 240-sample span need the slot's frame
        adsb_synth::Slot s;
        adsb_synth::slot_params(cfg, channel, slot, s);
        if (s.present) {
            const uint64_t start = slot * (uint64_t)cfg.slot_len + s.jitter;
            if (k >= start && k < start + 240 && adsb_synth::pulse_at(s.sent, (uint32_t)(k - start))) {
                vi += s.amp_i;
                vq += s.amp_q;
            }
        }
        if (ST == ADSB_SAMPLE_I8) {
            reinterpret_cast<int8_t *>(iq)[2 * j] = (int8_t)adsb_synth::clip8(vi);
            reinterpret_cast<int8_t *>(iq)[2 * j + 1] = (int8_t)adsb_synth::clip8(vq);
        } else {
            int wi = vi << cfg.amp_shift, wq = vq << cfg.amp_shift;
            wi = wi < -32768 ? -32768 : (wi > 32767 ? 32767 : wi);
            wq = wq < -32768 ? -32768 : (wq > 32767 ? 32767 : wq);
            reinterpret_cast<int16_t *>(iq)[2 * j] = (int16_t)wi;
            reinterpret_cast<int16_t *>(iq)[2 * j + 1] = (int16_t)wq;
        }
    }
}

hipError_t launch_synth(hipStream_t s, const adsb_synth_cfg &cfg, int sample_type, uint32_t channel,
                        uint64_t first, size_t n, void *iq)
{
    if (n == 0) return hipSuccess;
    dim3 grid(kSynthBlocks), block(kSynthThreads);
    if (sample_type == ADSB_SAMPLE_I8)
        hipLaunchKernelGGL((synth_kernel<ADSB_SAMPLE_I8>), grid, block, 0, s, cfg, channel, first, n, iq);
    else
        hipLaunchKernelGGL((synth_kernel<ADSB_SAMPLE_I16>), grid, block, 0, s, cfg, channel, first, n, iq);
    return hipGetLastError();
}

} // namespace adsbk
