// ab/sieve.inc -- the SIEVE scan (i8, kScanSieve); included by adsb_kernels.hip inside namespace adsbk.
//
// The root scan is bound by VALU issue (DESIGN.md section 5): 5.5 issue slots per sample for floor(sqrt(I^2+Q^2)), 4.8 for the
// sliding 16 + 10 tap ordering test, on an LDS image it has to transpose.  The sieve replaces both by ONE BIT PAIR per sample:
//   * a NECESSARY condition of the gate (demod.rs:17-57) that needs only neighbouring samples: every high/low pair of the
//     preamble and of the DF17 pattern that sits on adjacent samples -- 14 of them:
//         m[i+d] >= m[i+d+1]  for d in {0, 2, 7, 9, 16, 19, 21, 24}      ("G" taps)
//         m[i+d] <= m[i+d+1]  for d in {1, 6, 8, 18, 20, 22}             ("L" taps)
//     Noise passes all fourteen about once in 400 offsets (the taps are correlated: up-down runs are likelier than 2^-14).
//   * no root: with n = I^2+Q^2, floor(sqrt(a)) >= floor(sqrt(b)) implies b <= a + 2 sqrt(a) <= U(a) = a + a/8 + 8 (the
//     tangent of 2 sqrt at a = 64; a SUPERSET test -- exact floor(sqrt) decides the candidates afterwards).  Per sample: a mask,
//     one v_dot4_i32_i8 accumulating onto 0x4B000000 (the result IS the float 2^23 + n), half a v_pk_fma_f32 for 2^23 + U(n),
//     and two compares with the next sample: G[j] = (U(n[j]) >= n[j+1]), L[j] = (U(n[j+1]) >= n[j]).
//   * all of that happens in the registers the coalesced 16-byte loads fill: a lane holds 8 consecutive samples (+ the ninth,
//     its neighbour's first: one DPP move), shifts its 8 G bits and 8 L bits into two bytes (v_cmp + v_addc each: no
//     v_cndmask) and stores them: the tile's two BIT STREAMS in LDS, 4 KB for 16384 samples where the root scan parks 16 KB of
//     magnitudes.  No transposition of samples, no halo recomputation, no scalar-ALU work.
//   * the fourteen taps of an offset are then bit i + d of those streams: a lane takes 64 offsets at once as 64-bit words --
//     shifts and ANDs, ~40 VALU instructions per 64 x 64 offsets of a wave.
//   * the candidates (about 40 per tile on the synthetic stream: 8 frames + chance passes) are decided from the samples
//     themselves -- the raw IQ bytes, parked in LDS as they arrive (ds_write_b128 of the load registers: no VALU): the gate
//     exactly by one LANE per candidate (floor(sqrt) is monotone, so min / max are taken on n and two roots decide), the 112
//     PPM bits of the survivors by 16-lane groups with one root per pair (floor(sqrt(x)) > floor(sqrt(y)) iff r(x)^2 > y).
//     (Re-reading them from global memory instead -- ADSB_SV_IMG=0: 6.6 KB of LDS, eight workgroups per CU -- costs two dependent
//     round trips per tile: 0.229 ms against 0.200.)  Survivors go to the tile's frame slots exactly as the root scan leaves
//     them: Seg, slots and finish_order are shared, and so is the survivor hand-over (hand_over, adsb_kernels.hip) on the
//     path that coarse or constant input takes.
// Geometry: the root scan's (kTile = 16384 offsets, kThreads = 256); 39 KB of LDS per workgroup: four workgroups per CU.
// Measured (profiles/r04_ab_sieve.txt): loads + image + relation bits alone 0.154 ms (the read ceiling), + taps 0.170, complete
// 0.200 ms (root scan: 0.190): bit-exact, not faster -- an A/B kernel (-DADSB_AB_KERNELS=1).

// ADSB_SV_IMG = 1: the raw IQ image in LDS (39 KB per workgroup: four per CU), each wave decides its own candidates from it.
// ADSB_SV_IMG = 0 (A/B): no image (6.6 KB: eight workgroups per CU); the candidates' samples are re-read through the tile's
// descriptor (default cache policy: they were loaded a few microseconds ago), the tile's candidates pooled between barriers.
#ifndef ADSB_SV_IMG
#define ADSB_SV_IMG 1
#endif
#ifndef ADSB_SV_WAVES
#define ADSB_SV_WAVES (!ADSB_SV_IMG ? 8 : ADSB_SV_SWEEPS >= 8 ? 4 : 5) // waves per SIMD the register allocation is held to (= workgroups per CU)
#endif
#ifndef ADSB_SV_POOLED
#define ADSB_SV_POOLED (ADSB_SV_IMG ? 0 : 1) // the candidates' tail: 0 = wave by wave, 1 = the tile's candidates pooled between two barriers
#endif
#ifndef ADSB_SV_AUX
#define ADSB_SV_AUX (ADSB_SV_IMG ? ADSB_LOAD_AUX : 0) // cache policy of the streaming loads
#endif
constexpr int kSvSweeps = ADSB_SV_SWEEPS;                    // sweeps of 16-byte loads that cover the tile ...
constexpr int kSvTile = kSieveTile;                          // ... of kSvSweeps x 2048 offsets (adsb_kernels.h)
constexpr int kSvMag = kSvTile + kHalo;                      // samples a tile reads
constexpr int kSvOpl = kSvTile / kThreads;                   // offsets a lane takes in phase 2 (64 or 48)
constexpr int kSvHaloLanes = kHalo / 8;                      // ... and 32 lanes of one more sweep its 256 samples of halo (the
                                                             // sieve needs 25 of them, a survivor's PPM slice 239)
constexpr int kSvStreamBytes = ((kSvTile + 64) / 8 + 15) & ~15; // one bit stream: tile + 64 bits of halo, in whole 16 bytes
static_assert(kSvOpl % 16 == 0 && kSvOpl >= 32 && kSvOpl <= 64 && kSvHaloLanes <= 64 && kHalo % 8 == 0, "sieve scan geometry");
struct SieveLds {
    static constexpr int kOffImg = 0;                                // the raw IQ of tile + halo, 2 bytes per sample, linear
    static constexpr int kOffG = ADSB_SV_IMG ? kSvMag * 2 : 0;
    static constexpr int kOffL = kOffG + kSvStreamBytes;
    static constexpr int kOffCand = kOffL + kSvStreamBytes;          // candidate bitmap: word w = offsets 32 w .. 32 w + 31
    static constexpr int kOffList = kOffCand + kSvTile / 8;            // 1 KB: per wave 64 x u16 candidates + 64 x u16 survivors (the
                                                                     // usual path), or kListCap x u16 entries (the workgroup path)
    static constexpr int kOffMisc = kOffList + 1024;                 // 16 x u32
    static constexpr int kTotal = kOffMisc + 64;
};
static_assert(kThreads >= kListCap && kListCap * 2 <= 1024 && (kThreads / 64) * 64 * 4 <= 1024, "one lane per listed candidate");
static_assert(SieveLds::kTotal <= 163840 / ADSB_SV_WAVES, "ADSB_SV_WAVES workgroups per CU");

#ifndef ADSB_SV_ABL
#define ADSB_SV_ABL 0 // measurement only (no frames): 1 = loads + bit streams only, 2 = + sieve (candidates counted, not decided)
#endif

// [phase:1 sieve: nine samples -> two bytes of relation bits]
// v = the lane's 8 samples, x8 = the dword behind them (sample 8 in its low half).  Returns G byte | L byte << 8, bit k of a byte
// = relation k (sample k against sample k + 1).
// (asm: for the dot builtin hipcc picks VOP2 v_dot4c, which needs a v_mov per call; gfx950 wants 3 wait states between a DOT and
// a different VALU reading its result, and 2 between a VALU writing an SGPR and a VALU reading it; hipcc pads nothing around asm:
// the dot block ends in s_nop 2, and all eight compares of a block come before the first v_addc)
__device__ __forceinline__ uint32_t sv_relation_bytes(const u32x4 v, const uint32_t x8, const int acc, const f32x2 mul, const f32x2 add,
                                                      uint32_t &g, uint32_t &l)
{
    const uint32_t a0 = v.x & 0xFFFFu, a1 = v.x & 0xFFFF0000u, a2 = v.y & 0xFFFFu, a3 = v.y & 0xFFFF0000u,
                   a4 = v.z & 0xFFFFu, a5 = v.z & 0xFFFF0000u, a6 = v.w & 0xFFFFu, a7 = v.w & 0xFFFF0000u, a8 = x8 & 0xFFFFu;
    uint32_t f[9];
    asm("v_dot4_i32_i8 %0, %9, %14, %23\n\t"
        "v_dot4_i32_i8 %1, %9, %15, %23\n\t"
        "v_dot4_i32_i8 %2, %10, %16, %23\n\t"
        "v_dot4_i32_i8 %3, %10, %17, %23\n\t"
        "v_dot4_i32_i8 %4, %11, %18, %23\n\t"
        "v_dot4_i32_i8 %5, %11, %19, %23\n\t"
        "v_dot4_i32_i8 %6, %12, %20, %23\n\t"
        "v_dot4_i32_i8 %7, %12, %21, %23\n\t"
        "v_dot4_i32_i8 %8, %13, %22, %23\n\t"
        "s_nop 2"
        : "=&v"(f[0]), "=&v"(f[1]), "=&v"(f[2]), "=&v"(f[3]), "=&v"(f[4]), "=&v"(f[5]), "=&v"(f[6]), "=&v"(f[7]), "=&v"(f[8])
        : "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w), "v"(x8), "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(a4), "v"(a5), "v"(a6),
          "v"(a7), "v"(a8), "s"(acc));
    // 2^23 + 9 + 1.125 n, rounded to an integer: >= 2^23 + n + n/8 + 8.5 > 2^23 + n + 2 sqrt(n).  Both patterns are positive
    // floats of one binade: their integer order is their numeric order.
    uint32_t u[9];
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        f32x2 t = {__builtin_bit_cast(float, f[k]), __builtin_bit_cast(float, f[k + 1])};
        t = __builtin_elementwise_fma(t, mul, add);
        const float t0 = t.x, t1 = t.y; // (through scalars: __builtin_bit_cast of a vector ELEMENT reads element 0 here)
        u[k] = __builtin_bit_cast(uint32_t, t0);
        u[k + 1] = __builtin_bit_cast(uint32_t, t1);
    }
    u[8] = __builtin_bit_cast(uint32_t, __builtin_fmaf(__builtin_bit_cast(float, f[8]), mul.x, add.x));
    // bit k of G: u[k] >= f[k+1]; of L: u[k+1] >= f[k].  k = 7 first: byte = byte + byte + carry-in per relation.
    // (g, l: the shift registers, carried from call to call -- only their low eight bits are used, so they are never cleared)
    uint64_t m0, m1, m2, m3, m4, m5, m6, m7;
#define SV_SHIFT_IN                                                                                                 \
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %8\n\t"                                                                 \
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %7\n\t"                                                                 \
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %6\n\t"                                                                 \
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %5\n\t"                                                                 \
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %4\n\t"                                                                 \
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %3\n\t"                                                                 \
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %2\n\t"                                                                 \
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %1"
    asm("v_cmp_ge_u32_e64 %1, %9, %18\n\t"
        "v_cmp_ge_u32_e64 %2, %10, %19\n\t"
        "v_cmp_ge_u32_e64 %3, %11, %20\n\t"
        "v_cmp_ge_u32_e64 %4, %12, %21\n\t"
        "v_cmp_ge_u32_e64 %5, %13, %22\n\t"
        "v_cmp_ge_u32_e64 %6, %14, %23\n\t"
        "v_cmp_ge_u32_e64 %7, %15, %24\n\t"
        "v_cmp_ge_u32_e64 %8, %16, %25\n\t" SV_SHIFT_IN
        : "+v"(g), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3), "=&s"(m4), "=&s"(m5), "=&s"(m6), "=&s"(m7)
        : "v"(u[0]), "v"(u[1]), "v"(u[2]), "v"(u[3]), "v"(u[4]), "v"(u[5]), "v"(u[6]), "v"(u[7]), "v"(u[8]),
          "v"(f[1]), "v"(f[2]), "v"(f[3]), "v"(f[4]), "v"(f[5]), "v"(f[6]), "v"(f[7]), "v"(f[8])
        : "vcc");
    asm("v_cmp_ge_u32_e64 %1, %10, %18\n\t"
        "v_cmp_ge_u32_e64 %2, %11, %19\n\t"
        "v_cmp_ge_u32_e64 %3, %12, %20\n\t"
        "v_cmp_ge_u32_e64 %4, %13, %21\n\t"
        "v_cmp_ge_u32_e64 %5, %14, %22\n\t"
        "v_cmp_ge_u32_e64 %6, %15, %23\n\t"
        "v_cmp_ge_u32_e64 %7, %16, %24\n\t"
        "v_cmp_ge_u32_e64 %8, %17, %25\n\t" SV_SHIFT_IN
        : "+v"(l), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3), "=&s"(m4), "=&s"(m5), "=&s"(m6), "=&s"(m7)
        : "v"(u[0]), "v"(u[1]), "v"(u[2]), "v"(u[3]), "v"(u[4]), "v"(u[5]), "v"(u[6]), "v"(u[7]), "v"(u[8]),
          "v"(f[0]), "v"(f[1]), "v"(f[2]), "v"(f[3]), "v"(f[4]), "v"(f[5]), "v"(f[6]), "v"(f[7])
        : "vcc");
#undef SV_SHIFT_IN
    return (g & 0xFFu) | (l << 8);
}

// [phase:2 sieve: the fourteen taps on 64-bit words]
// G, L: bits 0 .. 95 of the two streams from this lane's first offset on.  With
//   Y[j] = L[j] & G[j+1]      A[j] = G[j] & Y[j+1]      Z[j] = Y[j] & Y[j+2]
//   P[i] = A[i] & Z[i+6] & G[i+16] & Z[i+18] & L[i+22] & G[i+24]      (taps G 0 2 7 9 16 19 21 24, L 1 6 8 18 20 22)
// returns P for the lane's 64 offsets.
__device__ __forceinline__ void sv_taps(const uint32_t (&G)[3], const uint32_t (&L)[3], uint32_t &p0, uint32_t &p1)
{
    auto sh = [](const uint32_t (&a)[3], int k, int d) { // word k of a >> d (0 < d < 32)
        return __builtin_amdgcn_alignbit(k + 1 < 3 ? a[k + 1] : 0u, a[k], (uint32_t)d);
    };
    uint32_t Y[3], Z[3], A[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) Y[k] = L[k] & sh(G, k, 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) Z[k] = Y[k] & sh(Y, k, 2);
#pragma unroll
    for (int k = 0; k < 2; ++k) A[k] = G[k] & sh(Y, k, 1);
    p0 = A[0] & sh(Z, 0, 6) & sh(G, 0, 16) & sh(Z, 0, 18) & sh(L, 0, 22) & sh(G, 0, 24);
    p1 = A[1] & sh(Z, 1, 6) & sh(G, 1, 16) & sh(Z, 1, 18) & sh(L, 1, 22) & sh(G, 1, 24);
}

// [phase:3 sieve: the samples themselves, re-read through the tile's descriptor]
// m = floor(sqrt(n)) as utils.rs:46-52: trunc(sqrtf(n + 0.5)) is exact for n <= 32768 (sqrt(n + 0.5) stays >= 1.3e-3 away from
// every integer there).  All values are the bit patterns 0x4B000000 + n (what the dot leaves), whose order is n's.
__device__ __forceinline__ uint32_t sv_root(uint32_t fbits) { return (uint32_t)__builtin_amdgcn_sqrtf(__builtin_bit_cast(float, fbits) - 8388607.5f); }
// the K samples from tile sample s0 on, from the raw image (img_lds: its LDS byte address): ds_read_u16 zero-extends, the dword
// [I, Q, 0, 0] is the dot's operand as it is.  (Dots in asm blocks of 13 / 8: VOP3P with the accumulator in an SGPR -- the builtin
// costs a v_mov per dot -- and an asm statement takes at most 30 operands.)
typedef const __attribute__((address_space(3))) uint16_t *sv_lds_u16;
__device__ __forceinline__ void sv_dots13(const uint32_t *x, uint32_t *n, const int acc)
{
    asm(
        "v_dot4_i32_i8 %0, %13, %13, %26\n\t"
        "v_dot4_i32_i8 %1, %14, %14, %26\n\t"
        "v_dot4_i32_i8 %2, %15, %15, %26\n\t"
        "v_dot4_i32_i8 %3, %16, %16, %26\n\t"
        "v_dot4_i32_i8 %4, %17, %17, %26\n\t"
        "v_dot4_i32_i8 %5, %18, %18, %26\n\t"
        "v_dot4_i32_i8 %6, %19, %19, %26\n\t"
        "v_dot4_i32_i8 %7, %20, %20, %26\n\t"
        "v_dot4_i32_i8 %8, %21, %21, %26\n\t"
        "v_dot4_i32_i8 %9, %22, %22, %26\n\t"
        "v_dot4_i32_i8 %10, %23, %23, %26\n\t"
        "v_dot4_i32_i8 %11, %24, %24, %26\n\t"
        "v_dot4_i32_i8 %12, %25, %25, %26\n\t"
        "s_nop 2"
        : "=&v"(n[0]), "=&v"(n[1]), "=&v"(n[2]), "=&v"(n[3]), "=&v"(n[4]), "=&v"(n[5]), "=&v"(n[6]), "=&v"(n[7]), "=&v"(n[8]), "=&v"(n[9]), "=&v"(n[10]), "=&v"(n[11]), "=&v"(n[12])
        : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]), "v"(x[8]), "v"(x[9]), "v"(x[10]), "v"(x[11]), "v"(x[12]), "s"(acc));
}
__device__ __forceinline__ void sv_dots8(const uint32_t *x, uint32_t *n, const int acc)
{
    asm(
        "v_dot4_i32_i8 %0, %8, %8, %16\n\t"
        "v_dot4_i32_i8 %1, %9, %9, %16\n\t"
        "v_dot4_i32_i8 %2, %10, %10, %16\n\t"
        "v_dot4_i32_i8 %3, %11, %11, %16\n\t"
        "v_dot4_i32_i8 %4, %12, %12, %16\n\t"
        "v_dot4_i32_i8 %5, %13, %13, %16\n\t"
        "v_dot4_i32_i8 %6, %14, %14, %16\n\t"
        "v_dot4_i32_i8 %7, %15, %15, %16\n\t"
        "s_nop 2"
        : "=&v"(n[0]), "=&v"(n[1]), "=&v"(n[2]), "=&v"(n[3]), "=&v"(n[4]), "=&v"(n[5]), "=&v"(n[6]), "=&v"(n[7])
        : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]), "s"(acc));
}
// Where the candidates' samples come from: the LDS image (its byte address) or the tile's buffer descriptor.
struct SvSrc {
    uint32_t lds;
    __amdgpu_buffer_rsrc_t rsrc;
};
// K = 13 / 8 samples from tile sample s0 on, as the zero-extended dwords [I, Q, 0, 0]
template <int K> __device__ __forceinline__ void sv_fetch(const SvSrc &src, const uint32_t s0, uint32_t (&x)[K])
{
#if ADSB_SV_IMG
    const uint32_t a0 = src.lds + 2u * s0;
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = *(sv_lds_u16)(uintptr_t)(a0 + 2u * k);
#else
    // two 16-byte loads from a 4-byte-aligned start cover 2 K + 2 bytes (K <= 14); reads past the channel end return zeros
    const uint32_t b = 2u * s0, base = b & ~3u, shift = (b & 2u) * 8u;
    const u32x4 q0 = __builtin_amdgcn_raw_buffer_load_b128(src.rsrc, base, 0, 0), q1 = __builtin_amdgcn_raw_buffer_load_b128(src.rsrc, base + 16u, 0, 0);
    const uint32_t d[9] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, 0u};
#pragma unroll
    for (int m = 0; m < (K + 1) / 2; ++m) {
        const uint32_t w = __builtin_amdgcn_alignbit(d[m + 1], d[m], shift); // samples 2m, 2m+1
        x[2 * m] = w & 0xFFFFu;
        if (2 * m + 1 < K) x[2 * m + 1] = w >> 16;
    }
#endif
}
__device__ __forceinline__ void sv_samples13(const SvSrc &src, const uint32_t s0, uint32_t (&n)[13])
{
    uint32_t x[13];
    sv_fetch<13>(src, s0, x);
    sv_dots13(x, n, 0x4B000000);
}
__device__ __forceinline__ void sv_samples8(const SvSrc &src, const uint32_t s0, uint32_t (&n)[8])
{
    uint32_t x[8];
    sv_fetch<8>(src, s0, x);
    sv_dots8(x, n, 0x4B000000);
}
// The exact gate (demod.rs:17-57) of the candidate at tile offset `off`, by one lane: min over highs of m >= max over lows of m;
// floor(sqrt) is monotone, so min and max are taken on n and two roots decide: floor(sqrt(h)) >= floor(sqrt(l))  <=>
// (floor(sqrt(h)) + 1)^2 > l.  (Two blocks of 13 samples, the first reduced before the second is read: the next tile's loads hold
// 40 registers while this runs.)
__device__ __forceinline__ bool sieve_gate_lane(const SvSrc &img_lds, const uint32_t off)
{
    auto mn = [](uint32_t a, uint32_t b) { return a < b ? a : b; };
    auto mx = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
    // preamble (demod.rs:20-22): highs 0 2 7 9, lows the other twelve; DF17 (demod.rs:41-44): highs 16 19 21 23 24, lows 17 18 20 22 25
    uint32_t ph, pl;
    {
        uint32_t n[13]; // samples 0 .. 12
        sv_samples13(img_lds, off, n);
        ph = mn(mn(n[0], n[2]), mn(n[7], n[9]));
        pl = mx(mx(mx(n[1], n[3]), mx(n[4], n[5])), mx(mx(n[6], n[8]), mx(mx(n[10], n[11]), n[12])));
    }
    asm volatile("" : "+v"(ph), "+v"(pl)); // (the first block is finished before the second starts)
    uint32_t n[13]; // samples 13 .. 25
    sv_samples13(img_lds, off + 13u, n);
    pl = mx(pl, mx(mx(n[0], n[1]), n[2]));
    const uint32_t dh = mn(mn(mn(n[3], n[6]), mn(n[8], n[10])), n[11]);
    const uint32_t dl = mx(mx(mx(n[4], n[5]), mx(n[7], n[9])), n[12]);
    const uint32_t r1 = sv_root(ph) + 1u, r2 = sv_root(dh) + 1u;
    return (__umul24(r1, r1) + 0x4B000000u) > pl && (__umul24(r2, r2) + 0x4B000000u) > dl;
}
// The PPM slice of one survivor by a 16-lane group.  Lane l < 14: frame byte l = samples off + 16 + 16 l .. + 15 (lanes 14, 15
// compute a byte nobody uses).  PPM bit (demod.rs:92-131, 180-201): m[x] > m[y]  <=>  r^2 > n[y] with r = m[x] (r^2 is the largest
// square <= n[x]): one root per pair.  bit k = r2[k] > y[k], MSB first: one compare per pair into its own SGPR pair, then nibble =
// nibble + nibble + carry-in per pair (v_addc): no v_cndmask (20 cycles here).  Two blocks of 8 samples.
__device__ __forceinline__ uint32_t sieve_slice_byte(const SvSrc &img_lds, const uint32_t off, const uint32_t l)
{
    const uint32_t s0 = off + 16u + 16u * (l < 14u ? l : 13u);
    uint32_t byte = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        uint32_t n[8], r2[4];
        sv_samples8(img_lds, s0 + 8u * h, n);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t r = sv_root(n[2 * k]);
            r2[k] = __umul24(r, r) + 0x4B000000u;
        }
        uint64_t m0, m1, m2, m3;
        asm("v_cmp_gt_u32_e64 %1, %5, %9\n\t"
            "v_cmp_gt_u32_e64 %2, %6, %10\n\t"
            "v_cmp_gt_u32_e64 %3, %7, %11\n\t"
            "v_cmp_gt_u32_e64 %4, %8, %12\n\t"
            "s_nop 0\n\t"
            "v_addc_co_u32_e64 %0, vcc, %0, %0, %1\n\t"
            "v_addc_co_u32_e64 %0, vcc, %0, %0, %2\n\t"
            "v_addc_co_u32_e64 %0, vcc, %0, %0, %3\n\t"
            "v_addc_co_u32_e64 %0, vcc, %0, %0, %4"
            : "+v"(byte), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3)
            : "v"(r2[0]), "v"(r2[1]), "v"(r2[2]), "v"(r2[3]), "v"(n[1]), "v"(n[3]), "v"(n[5]), "v"(n[7])
            : "vcc");
        asm volatile("" : "+v"(byte));
    }
    return byte;
}

// [phase:end]
// A tile's loads, all in flight at once: per sweep the lane's 16 bytes (8 samples).  The ninth sample a lane needs is its
// neighbour's first: one DPP move -- except for lane 63, whose neighbour is in another wave: it comes from a 4-byte load of the
// dword behind the wave's 1024 bytes (one address per wave).  Bounds-checked descriptor: reads past the channel end return
// zeros; `live` = false (there is no such tile) clips it to zero records.
struct SieveRegs {
    u32x4 raw[kSvSweeps];
    uint32_t nxt[kSvSweeps]; // the dword behind the wave's 1024 bytes of a sweep (every lane of the wave names the same address)
};
__device__ __forceinline__ void sieve_issue_loads(const DemodArgs &p, const uint32_t tile, const bool live, SieveRegs &r)
{
    const uint32_t tid = threadIdx.x;
    const TilePos tp = tile_pos<kSvTile>(p, tile);
    __amdgpu_buffer_rsrc_t rsrc = tile_rsrc<2, kSvMag>(p, tp, live);
#pragma unroll
    for (int it = 0; it < kSvSweeps; ++it) {
        r.raw[it] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, tid * 16, (uint32_t)it * (kThreads * 16), ADSB_SV_AUX);
        r.nxt[it] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (tid | 63u) * 16 + 16, (uint32_t)it * (kThreads * 16), 0);
    }
}

// The tile body of the sieve scan (same contract as scan_tile: Seg, slots, header flags) on the loads `cur` holds.  has_next
// (the persistent A/B form only, ADSB_SIEVE_PERSIST): the NEXT tile's loads are issued into the same registers as soon as
// phase 1 has freed them, so that they are in flight while this tile's latency-bound tail (taps, candidate list, gate, slices:
// ~1.5 us) runs -- measured slower than one tile per workgroup (profiles/r04_ab_sieve.txt).
__device__ __forceinline__ void sieve_tile_body(const DemodArgs &p, const uint32_t tile, const bool first, unsigned char *smem,
                                                SieveRegs &cur, const bool has_next = false, const uint32_t next_tile = 0)
{
    typedef SieveLds L;
    unsigned char *gbytes = smem + L::kOffG, *lbytes = smem + L::kOffL;
    uint32_t *cand = reinterpret_cast<uint32_t *>(smem + L::kOffCand);
    uint16_t *list = reinterpret_cast<uint16_t *>(smem + L::kOffList);
    uint32_t *misc = reinterpret_cast<uint32_t *>(smem + L::kOffMisc);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const TilePos tp = tile_pos<kSvTile>(p, tile);
    const uint64_t sample0 = tp.sample0;
    const uint32_t n_valid = tp.n_valid;
    u32x4 (&raw)[kSvSweeps] = cur.raw;
    u32x4 raw_h = {0, 0, 0, 0};
    if (wave == 0) { // the halo: 256 samples behind the tile (lanes 0-31; the other lanes' addresses are clipped to the last of
                     // those); not part of the prefetched set: it is used last in phase 1
        __amdgpu_buffer_rsrc_t rsrc = tile_rsrc<2, kSvMag>(p, tp, true);
        const uint32_t a = (tid < (uint32_t)kSvHaloLanes ? tid : (uint32_t)kSvHaloLanes - 1u) * 16u;
        raw_h = __builtin_amdgcn_raw_buffer_load_b128(rsrc, a, (uint32_t)kSvSweeps * (kThreads * 16), ADSB_SV_AUX);
    }
    SvSrc src;
    src.lds = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned char *)(smem + L::kOffImg);
    src.rsrc = tile_rsrc<2, kSvMag>(p, tp, true);
    clear_launch_flags(p, first, tid);
    if (tid < 16) misc[tid] = 0; // [4 + wave]: the wave's candidates; [8]: valid frames (tiles without slots only); [13]: survivors;
                                 // [14]: the workgroup path is needed
    // [phase:1 sieve: relation bits]
    {
        const int acc = 0x4B000000;            // 2^23 as float bits: the dot's accumulator
        f32x2 mul = {1.125f, 1.125f}, add = {-1048567.0f, -1048567.0f};
        asm("" : "+v"(mul), "+v"(add));        // (held in registers: hipcc otherwise re-materialises the constants per use)
        uint32_t sg = 0, sl = 0;
        u32x4 *img4 = reinterpret_cast<u32x4 *>(smem + L::kOffImg);
#pragma unroll
        for (int it = 0; it < kSvSweeps; ++it) {
            if (ADSB_SV_IMG) img4[it * kThreads + tid] = raw[it]; // the raw samples, for the candidates
            const uint32_t x8 = (uint32_t)__builtin_amdgcn_update_dpp((int)cur.nxt[it], (int)raw[it].x, 0x130 /* wave_shl:1 */, 0xF, 0xF, false);
            const uint32_t gl = sv_relation_bytes(raw[it], x8, acc, mul, add, sg, sl);
            gbytes[it * kThreads + tid] = (unsigned char)gl;          // relation bits of samples it * 2048 + 8 tid .. + 7
            lbytes[it * kThreads + tid] = (unsigned char)(gl >> 8);
        }
        if (wave == 0) { // (relation bits of the halo's first 32 samples are all the sieve reads: four lanes' bytes)
            if (ADSB_SV_IMG && tid < (uint32_t)kSvHaloLanes) img4[kSvSweeps * kThreads + tid] = raw_h;
            const uint32_t x8 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)raw_h.x, 0x130 /* wave_shl:1 */, 0xF, 0xF, false);
            const uint32_t gl = sv_relation_bytes(raw_h, x8, acc, mul, add, sg, sl);
            if (tid < 4u) {
                gbytes[kSvSweeps * kThreads + tid] = (unsigned char)gl;
                lbytes[kSvSweeps * kThreads + tid] = (unsigned char)(gl >> 8);
            }
        }
    }
    __syncthreads();
    if (has_next) sieve_issue_loads(p, next_tile, true, cur); // (persistent form, workgroup-uniform: the registers are free now)
#if ADSB_SV_ABL == 1
    if (smem[tid * 160] == 0xFD && smem[tid * 160 + 1] == 0xFE && n_valid == 7) misc[12] = 1; // (keeps the LDS stores alive)
#else
    // [phase:2 sieve: taps, candidate list]
    {
        // the lane's window: stream bits kSvOpl tid .. + 95 (its kSvOpl offsets + 25 bits of taps), from byte kSvOpl / 8 * tid
        uint32_t G[3], Lr[3];
        if constexpr (kSvOpl % 32 == 0) {
            const uint32_t *gw = reinterpret_cast<const uint32_t *>(gbytes) + (kSvOpl / 32) * tid, *lw = reinterpret_cast<const uint32_t *>(lbytes) + (kSvOpl / 32) * tid;
#pragma unroll
            for (int k = 0; k < 3; ++k) { G[k] = gw[k]; Lr[k] = lw[k]; }
        } else { // (48 offsets per lane: the window starts on an even byte -- four aligned dwords, shifted by 0 or 16 bits)
            const uint32_t b0_ = (uint32_t)(kSvOpl / 8) * tid, sh = (b0_ & 3u) * 8u;
            const uint32_t *gw = reinterpret_cast<const uint32_t *>(gbytes + (b0_ & ~3u)), *lw = reinterpret_cast<const uint32_t *>(lbytes + (b0_ & ~3u));
            const uint32_t g4[4] = {gw[0], gw[1], gw[2], gw[3]}, l4[4] = {lw[0], lw[1], lw[2], lw[3]};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                G[k] = __builtin_amdgcn_alignbit(g4[k + 1], g4[k], sh);
                Lr[k] = __builtin_amdgcn_alignbit(l4[k + 1], l4[k], sh);
            }
        }
        uint32_t b0, b1;
        sv_taps(G, Lr, b0, b1);
        if constexpr (kSvOpl < 64) b1 &= (1u << (kSvOpl - 32)) - 1u;
        const uint32_t o0 = tid * (uint32_t)kSvOpl;
        // offsets at or beyond n_valid do not exist in the reference loop (adsb.rs:98): the ragged last tile of a channel
        if (n_valid < (uint32_t)kSvTile) { // (wave-uniform)
            const uint32_t v = n_valid > o0 ? n_valid - o0 : 0u;
            b0 &= v >= 32u ? 0xFFFFFFFFu : ((1u << v) - 1u);
            b1 &= v >= 64u ? 0xFFFFFFFFu : (v > 32u ? ((1u << (v - 32u)) - 1u) : 0u);
        }
        { // the bitmap (the workgroup path reads it): kSvOpl / 16 half-words per lane
            uint16_t *c16 = reinterpret_cast<uint16_t *>(cand) + (kSvOpl / 16) * tid;
            c16[0] = (uint16_t)b0;
            c16[1] = (uint16_t)(b0 >> 16);
            c16[2] = (uint16_t)b1;
            if constexpr (kSvOpl == 64) c16[3] = (uint16_t)(b1 >> 16);
        }
        // [phase:3 sieve: the usual path, wave by wave]
        // Each wave decides its own candidates (~10): no workgroup barrier, no shared list.  Its lanes append their offsets to
        // the wave's list (one LDS atomic), lane ci runs the exact gate on candidate ci, the survivors (~2) take slots of the
        // tile's own region through one counter, and 16-lane groups slice them.  Anything unusual -- more than 64 candidates in
        // a wave, more than kQuota survivors in the tile -- raises misc[14]: the workgroup path below redoes the tile.
        // (Measured alternatives, all bit-exact, profiles/r04_ab_sieve.txt: one list per tile decided by wave 0 between two
        // workgroup barriers 0.200 ms; by every wave redundantly 0.208; by the last wave to arrive 0.219; this form 0.200.)
        const SvSrc &img_lds = src;
#if ADSB_SV_POOLED
        // (A/B) the tile's candidates pooled: one list, the exact gate by lane ci on candidate ci behind a barrier, the
        // survivors' slices by the workgroup's 16-lane groups behind another
        if (!p.fused_pass_only && ADSB_SV_ABL == 0) {
            if (b0 | b1) {
                uint32_t pos = atomicAdd(&misc[12], (uint32_t)(__builtin_popcount(b0) + __builtin_popcount(b1)));
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    uint32_t bits = k ? b1 : b0;
                    while (bits) {
                        const uint32_t b = (uint32_t)__builtin_ctz(bits);
                        bits &= bits - 1;
                        if (pos < (uint32_t)kSparseCap) list[pos] = (uint16_t)(o0 + 32u * k + b);
                        ++pos;
                    }
                }
            }
            __syncthreads();
            const uint32_t n_c = misc[12];
            uint16_t *sv = list + 256;
            if (n_c > (uint32_t)kSparseCap) {
                if (tid == 0) misc[14] = 1u;
            } else if (n_c != 0) { // (workgroup-uniform)
                if (64u * wave < n_c) {
                    const bool have = tid < n_c;
                    const uint32_t coff = have ? list[tid] : 0u;
                    const bool ok = have && sieve_gate_lane(img_lds, coff);
                    const unsigned long long okm = __builtin_amdgcn_ballot_w64(ok);
                    if (okm != 0) {
                        uint32_t wb = 0;
                        if (lane == 0) wb = atomicAdd(&misc[13], (uint32_t)__builtin_popcountll(okm));
                        wb = __builtin_amdgcn_readfirstlane(wb);
                        if (ok) sv[wb + __builtin_amdgcn_mbcnt_hi((uint32_t)(okm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)okm, 0u))] = (uint16_t)coff;
                    }
                }
                __syncthreads();
                const uint32_t n_s = misc[13];
                if (n_s > kQuota) {
                    if (tid == 0) misc[14] = 1u;
                } else {
                    const uint64_t abs0 = sample0 + p.offset_base;
                    const uint32_t g = tid >> 4, l = tid & 15u;
                    for (uint32_t r = 0; r < n_s; r += kThreads / 16) {
                        if (r + 4 * wave >= n_s) break;
                        const uint32_t ci = r + g;
                        const bool have2 = ci < n_s;
                        const uint32_t off = have2 ? sv[ci] : 0u;
                        const uint32_t byte = sieve_slice_byte(img_lds, off, l);
                        if (have2) put_record(p.slots + (size_t)(tile * kQuota + ci), abs0 + off, byte, l);
                    }
                }
            }
        }
#else
        uint16_t *wc = list + 128 * wave, *ws = wc + 64;
        if (!p.fused_pass_only && ADSB_SV_ABL == 0) {
            if (b0 | b1) {
                uint32_t pos = atomicAdd(&misc[4 + wave], (uint32_t)(__builtin_popcount(b0) + __builtin_popcount(b1)));
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    uint32_t bits = k ? b1 : b0;
                    while (bits) {
                        const uint32_t b = (uint32_t)__builtin_ctz(bits);
                        bits &= bits - 1;
                        if (pos < 64u) wc[pos] = (uint16_t)(o0 + 32u * k + b);
                        ++pos;
                    }
                }
            }
            const uint32_t n_w = __builtin_amdgcn_readfirstlane(misc[4 + wave]); // (after this wave's atomics: LDS is in order)
            if (n_w > 64u) {
                if (lane == 0) atomicOr(&misc[14], 1u);
            } else if (n_w != 0) {
                const bool have = lane < n_w;
                const uint32_t coff = have ? wc[lane] : 0u;
                const bool ok = have && sieve_gate_lane(img_lds, coff);
                const unsigned long long okm = __builtin_amdgcn_ballot_w64(ok);
                const uint32_t n_s = (uint32_t)__builtin_popcountll(okm);
                if (n_s != 0) {
                    uint32_t sb = 0;
                    if (lane == 0) sb = atomicAdd(&misc[13], n_s);
                    sb = __builtin_amdgcn_readfirstlane(sb);
                    if (ok) ws[__builtin_amdgcn_mbcnt_hi((uint32_t)(okm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)okm, 0u))] = (uint16_t)coff;
                    if (sb + n_s > kQuota) {
                        if (lane == 0) atomicOr(&misc[14], 1u);
                    } else {
                        const uint64_t abs0 = sample0 + p.offset_base; // absolute offset of this tile's offset 0
                        const uint32_t gi = lane >> 4, l = lane & 15u;
                        for (uint32_t r = 0; r < n_s; r += 4) {
                            const uint32_t ci = r + gi;
                            const bool have2 = ci < n_s; // uniform within the 16-lane group
                            const uint32_t off = have2 ? ws[ci] : 0u;
                            const uint32_t byte = sieve_slice_byte(img_lds, off, l);
                            if (have2) put_record(p.slots + (size_t)(tile * kQuota + sb + ci), abs0 + off, byte, l);
                        }
                    }
                }
            }
        }
#endif
    }
#endif
    __syncthreads();
    if (misc[14] == 0) { // (workgroup-uniform) the usual case: Seg::cand counts SURVIVORS, as after the root scan
        if (tid == 0) write_seg(p, tile, tile * kQuota, misc[13], 0);
        return;
    }

    // [phase:3 sieve: the workgroup path (coarse or constant input: many candidates)]
    // The root scan's hand-over on the candidate bitmap (there is no list: kCountBitmap): compacted in offset order by
    // workgroup-wide prefix sums, every candidate gets a slot from the pool, the exact gate runs one LANE per entry of a chunk
    // (kListCap <= kThreads) and marks what it rejects in place (bit 15), the others are sliced by 16-lane groups; a rejected
    // entry leaves a record whose offset is all ones (finish_order skips it).
    const SvSrc &img_lds = src;
    __syncthreads(); // (every thread has read misc[14]: misc[0 .. 3] are free)
    hand_over<kSvTile, 32>(
        p, tile, sample0, kCountBitmap, cand, list, misc, tid, lane, wave,
        [&](const bool have, const uint32_t ent, const uint32_t l, bool &dropped) {
            dropped = (ent & 0x8000u) != 0;
            uint32_t byte = 0;
            if (__builtin_amdgcn_ballot_w64(have && !dropped) != 0) byte = sieve_slice_byte(img_lds, ent & 0x7FFFu, l); // (wave-uniform)
            return byte;
        },
        [&](uint16_t *entries, const uint32_t n) {
            if (tid < n) {
                const uint32_t off = entries[tid];
                if (!sieve_gate_lane(img_lds, off)) entries[tid] = (uint16_t)(off | 0x8000u);
            }
            __syncthreads();
        });
}

// one tile (the small-buffer kernel's workgroups)
__device__ __forceinline__ void scan_tile_sieve(const DemodArgs &p, const uint32_t tile, const bool first, unsigned char *smem)
{
    SieveRegs r;
    sieve_issue_loads(p, tile, true, r);
    sieve_tile_body(p, tile, first, smem, r);
}

// ADSB_SIEVE_PERSIST (A/B): persistent workgroups, four per CU; workgroup b takes tiles b, b + gridDim.x, ...; the next tile's
// loads are issued into the registers phase 1 has freed, so they are in flight during the tail.  Every workgroup does the same
// work at the same speed: without a stagger at the start all of them load at the same time and compute at the same time.
#ifndef ADSB_SIEVE_PERSIST
#define ADSB_SIEVE_PERSIST 0
#endif
#ifndef ADSB_SIEVE_STAGGER
#define ADSB_SIEVE_STAGGER 1
#endif
constexpr bool kSievePersistent = ADSB_SIEVE_PERSIST != 0;
#if ADSB_AB_KERNELS
__global__ __launch_bounds__(kThreads, ADSB_SV_WAVES) void demod_tiles_sieve(DemodArgs p)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[SieveLds::kTotal];
#if ADSB_SIEVE_PERSIST
    const uint32_t stride = gridDim.x, t_end = p.tile_first + p.tile_count;
    uint32_t t = p.tile_first + blockIdx.x;
#if ADSB_SIEVE_STAGGER
    { // a pseudo-random start delay of up to ~5 us (a tile takes ~5): the workgroups' phases stay spread
        const uint32_t h = (blockIdx.x * 2654435761u) >> 28; // 0 .. 15
        for (uint32_t k = 0; k < h; ++k) __builtin_amdgcn_s_sleep(12); // 12 x 64 cycles each
    }
#endif
    SieveRegs r;
    sieve_issue_loads(p, t, true, r);
    for (;;) {
        const uint32_t t2 = t + stride;
        const bool has2 = t2 < t_end;
        sieve_tile_body(p, t, t == p.tile_first, smem, r, has2, t2);
        if (!has2) break;
        __syncthreads(); // (the LDS image and lists are the next tile's now)
        t = t2;
    }
#else
    scan_tile_sieve(p, p.tile_first + tile_of_workgroup(blockIdx.x, p.tile_count), blockIdx.x == 0, smem);
#endif
}
#endif
