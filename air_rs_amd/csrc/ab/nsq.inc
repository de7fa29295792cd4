// ab/nsq.inc -- the NSQ scan (i8, kScanNsq); included by adsb_kernels.hip inside namespace adsbk.
//
// The root scan's three phases on an image of n = I^2+Q^2 instead of floor(sqrt(n)): no root per sample, the gate exact
// all the same (DESIGN.md section 4.1b).  Fewer VALU issue slots than the root scan, but 2 bytes of LDS per sample -- half the
// resident workgroups: the round-3 A/B kernel (bit-exact, slower; profiles/r03_ab_nsq_vs_root.txt).  Tile prologue and
// survivor hand-over are the root scan's (adsb_kernels.hip); nsq_pack16, nsq_band and nsq_root also serve the register
// scan (ab/reg.inc).

// ---- the nsq image (i8, kScanNsq): what phase 1 leaves in LDS for the gate and the slicer ------------------------
// One dword per PAIR of samples half a tile apart: logical dword q in [0, kNsqLog) holds v(q) in its low half and
// v(q + kNsqHalf) in its high half, v(k) = I_k^2 + Q_k^2 + 72 (<= 32840).  That pair is exactly what lane L's
// two runs (offsets 32 L + o and kNsqHalf + 32 L + o) need in one VGPR at step o: the gate reads it as it is, no
// unpacking.  Dwords kNsqHalf .. kNsqHalf+255 repeat samples as low halves that dwords 0..255 hold as high halves
// (the halo of run A's last lanes).  Physical dword = q + 4 (q >> 6): four pad dwords per 64 put the 16-byte reads
// of a ds_read_b128 lane group (lane L starts at 32 L) on sixteen different slots of the 64 banks.
constexpr int kNsqBias = 72;                 // 9 * 8: (v >> 3) = (n >> 3) + 9 exactly
constexpr int kNsqHalf = kTile / 2;          // 8192
constexpr int kNsqLog = kNsqHalf + kHalo;    // logical dwords
#ifndef ADSB_NSQ_PAD_SHIFT
#define ADSB_NSQ_PAD_SHIFT 6 // four pad dwords per 2^6 logical dwords (5: per 32 -- also conflict-free for the stores, 6 % more LDS)
#endif
constexpr int kNsqPadShift = ADSB_NSQ_PAD_SHIFT;
__host__ __device__ constexpr uint32_t nsq_phys(uint32_t q) { return q + 4u * (q >> kNsqPadShift); }
constexpr int kNsqPhys = (int)nsq_phys(kNsqLog);  // 8976 dwords = 35904 bytes
static_assert(kNsqHalf % 64 == 0 && kHalo % 64 == 0 && kRun == 32 && (kNsqPadShift == 5 || kNsqPadShift == 6),
              "nsq image: pads every 32 or 64 dwords, runs of 32");

struct NsqLds {
    static constexpr int kOffCand = kNsqPhys * 4;                  // one word per run of 32 offsets: survivor bitmap
    static constexpr int kOffList = kOffCand + 2 * kThreads * 4;   // kListCap x u16
    static constexpr int kOffMisc = kOffList + kListCap * 2;       // 16 x u32
    static constexpr int kTotal = kOffMisc + 64;
};

// [phase:1 nsq (loads, dots, stores)]
// ---- phase 1 of the nsq scan: raw i8 IQ -> the nsq image --------------------------------------------------------
// One sweep of a lane = 16 bytes at sample q0 (eight "A" samples, low halves) and 16 bytes at sample q0 + kNsqHalf
// (eight "B" samples, high halves) -> eight packed dwords -> two ds_write_b128.  kNsqIters sweeps of the workgroup
// cover the image; the last one is the 256-dword halo (lanes 0-31 only).
constexpr int kNsqIters = (kNsqLog + kThreads * 8 - 1) / (kThreads * 8);
constexpr int kNsqFull = kNsqLog / (kThreads * 8);  // sweeps every lane takes part in
constexpr int kNsqTail = kNsqLog % (kThreads * 8);  // logical dwords of the last, partial sweep (the halo: 256)
static_assert(kNsqIters - kNsqFull <= 1 && kNsqTail % 8 == 0, "at most one partial sweep of whole lanes");

__device__ __forceinline__ void nsq_issue_loads(const DemodArgs &p, const TilePos &tp, uint32_t tid,
                                                u32x4 (&ra)[kNsqIters], u32x4 (&rb)[kNsqIters])
{
    __amdgpu_buffer_rsrc_t rsrc = tile_rsrc<2, kMag>(p, tp, true);
    // (the sweep's constant goes into the SGPR offset, which the descriptor's bounds check covers:
    // tools/ubench/soffset_probe.hip; reads past the channel end return zeros)
#pragma unroll
    for (int it = 0; it < kNsqFull; ++it) {
        ra[it] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, tid * 16, (uint32_t)it * (kThreads * 16), ADSB_LOAD_AUX);
        rb[it] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, tid * 16, (uint32_t)it * (kThreads * 16) + 2 * kNsqHalf, ADSB_LOAD_AUX);
    }
    if (kNsqTail && __builtin_amdgcn_readfirstlane(tid & ~63u) * 8 < (uint32_t)kNsqTail) { // (whole waves past the halo skip it)
        ra[kNsqFull] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, tid * 16, (uint32_t)kNsqFull * (kThreads * 16), ADSB_LOAD_AUX);
        rb[kNsqFull] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, tid * 16, (uint32_t)kNsqFull * (kThreads * 16) + 2 * kNsqHalf, ADSB_LOAD_AUX);
    }
}

// 8 A samples + 8 B samples -> 8 dwords (B's v << 16) | A's v, v = I^2 + Q^2 + 72.
//   A: v_and (the sample's two bytes) + v_dot4_i32_i8 accumulating onto the SGPR constant 0x00480048 (the bias of
//      both halves at once);
//   B: v_perm to the i16 pair (I * 256, Q * 256) + v_dot2_i32_i16 accumulating onto A's result: (I^2 + Q^2) << 16.
//      (n = 32768, I = Q = -128, wraps to the right bits.)
// 2 VALU per sample, packing included.  gfx950 wants 3 wait states between a DOT and a different VALU reading its
// result and hipcc pads nothing inside asm: the dot2 reads its dot4 eight instructions later, and the block ends in
// s_nop 2.
__device__ __forceinline__ void nsq_pack16(u32x4 a, u32x4 b, uint32_t (&d)[8])
{
    const uint32_t a0 = a.x & 0xFFFFu, a1 = a.x & 0xFFFF0000u, a2 = a.y & 0xFFFFu, a3 = a.y & 0xFFFF0000u,
                   a4 = a.z & 0xFFFFu, a5 = a.z & 0xFFFF0000u, a6 = a.w & 0xFFFFu, a7 = a.w & 0xFFFF0000u;
    // bytes [0, I, 0, Q] of the even / odd sample of a dword (selector 0x0C = a zero byte)
    const uint32_t h0 = __builtin_amdgcn_perm(b.x, b.x, 0x010C000Cu), h1 = __builtin_amdgcn_perm(b.x, b.x, 0x030C020Cu),
                   h2 = __builtin_amdgcn_perm(b.y, b.y, 0x010C000Cu), h3 = __builtin_amdgcn_perm(b.y, b.y, 0x030C020Cu),
                   h4 = __builtin_amdgcn_perm(b.z, b.z, 0x010C000Cu), h5 = __builtin_amdgcn_perm(b.z, b.z, 0x030C020Cu),
                   h6 = __builtin_amdgcn_perm(b.w, b.w, 0x010C000Cu), h7 = __builtin_amdgcn_perm(b.w, b.w, 0x030C020Cu);
    const uint32_t bias2 = (uint32_t)kNsqBias * 0x00010001u;
    asm("v_dot4_i32_i8 %0, %8, %12, %28\n\t"
        "v_dot4_i32_i8 %1, %8, %13, %28\n\t"
        "v_dot4_i32_i8 %2, %9, %14, %28\n\t"
        "v_dot4_i32_i8 %3, %9, %15, %28\n\t"
        "v_dot4_i32_i8 %4, %10, %16, %28\n\t"
        "v_dot4_i32_i8 %5, %10, %17, %28\n\t"
        "v_dot4_i32_i8 %6, %11, %18, %28\n\t"
        "v_dot4_i32_i8 %7, %11, %19, %28\n\t"
        "v_dot2_i32_i16 %0, %20, %20, %0\n\t"
        "v_dot2_i32_i16 %1, %21, %21, %1\n\t"
        "v_dot2_i32_i16 %2, %22, %22, %2\n\t"
        "v_dot2_i32_i16 %3, %23, %23, %3\n\t"
        "v_dot2_i32_i16 %4, %24, %24, %4\n\t"
        "v_dot2_i32_i16 %5, %25, %25, %5\n\t"
        "v_dot2_i32_i16 %6, %26, %26, %6\n\t"
        "v_dot2_i32_i16 %7, %27, %27, %7\n\t"
        "s_nop 2"
        : "=&v"(d[0]), "=&v"(d[1]), "=&v"(d[2]), "=&v"(d[3]), "=&v"(d[4]), "=&v"(d[5]), "=&v"(d[6]), "=&v"(d[7])
        : "v"(a.x), "v"(a.y), "v"(a.z), "v"(a.w), "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(a4), "v"(a5), "v"(a6), "v"(a7),
          "v"(h0), "v"(h1), "v"(h2), "v"(h3), "v"(h4), "v"(h5), "v"(h6), "v"(h7), "s"(bias2));
}

// raw IQ -> the nsq image.  Returns (wave-uniform) whether this wave saw a value that is not an ordered f16 bit
// pattern: v >= 0x7C00, i.e. |I| and |Q| both >= 125 (nine values of n, 31752 .. 32768).  The running
// v_pk_minimum3_f16 finds them all: 0x7C01..0x7FFF are NaNs, which minimum3 propagates, 0x8048 (n = 32768) is a
// negative number, and 0x7C00 (+infinity, which a minimum would not see) is no sum of two squares of i8 values.
__device__ __forceinline__ bool nsq_image_to_lds(const u32x4 (&ra)[kNsqIters], const u32x4 (&rb)[kNsqIters], uint32_t *img, uint32_t tid)
{
    uint32_t lo = 0x7BFF7BFFu; // largest finite pattern
    const uint32_t q_t = tid * 8;
    uint32_t *dst = img + nsq_phys(q_t);
    auto sweep = [&](const int it, const bool store) {
        uint32_t d[8];
        nsq_pack16(ra[it], rb[it], d);
#pragma unroll
        for (int k = 0; k < 8; k += 2) lo = pkmin3<true>(lo, d[k], d[k + 1]);
        if (store) { // (8 kThreads is a multiple of 64: the sweep is a constant offset)
            u32x4 *w = reinterpret_cast<u32x4 *>(dst + nsq_phys(it * kThreads * 8));
            w[0] = u32x4{d[0], d[1], d[2], d[3]};
            w[1] = u32x4{d[4], d[5], d[6], d[7]};
        }
    };
#pragma unroll
    for (int it = 0; it < kNsqFull; ++it) sweep(it, true);
    if (kNsqTail && __builtin_amdgcn_readfirstlane(tid & ~63u) * 8 < (uint32_t)kNsqTail) sweep(kNsqFull, q_t < (uint32_t)kNsqTail);
    return __builtin_amdgcn_ballot_w64(((lo & 0xFFFFu) >= 0x7C00u) || ((lo >> 16) >= 0x7C00u)) != 0;
}

// [phase:2 nsq gate: set-up]
// ---- the gate on the nsq image ------------------------------------------------------------------------------------
// The reference orders truncated roots s(.) = floor(sqrt(.)) (demod.rs:27-36, 48-54 on utils.rs:46-52): pass when
// s(a) >= s(b), a = the smallest "high" n, b = the largest "low" n (s is monotone, so the minimum / maximum of the
// roots are the roots of the minimum / maximum).  On n itself:  a >= b passes outright;  a < b passes only if
// s(a) = s(b), which forces b - a <= 2 s(a) <= 2 sqrt(a) <= a / 8 + 8 (AM-GM).  So with the biased values v = n + 72
//     b' <= t(a'),   t(x) = x + (x >> 3)          [ = n_a + (n_a >> 3) + 9 + 72 ]
// is an exact SUPERSET test in two packed instructions; lanes that pass it for the preamble AND the DF17 group are
// survivors at once when a' >= b' in both, and only the rest (a < b inside the band: a handful per million offsets)
// take two roots per group in a cold block.  Per step (two offsets) the common path is 3 three-input max, 2 min,
// shift, add, 2 compares = 9 VALU on values that need no unpacking.
// F16OK: every value of the tile is below 0x7C00, an ordered f16 pattern (v_pk_maximum3_f16 / v_pk_minimum3_f16);
// otherwise pairs of integer v_pk_max_u16 / v_pk_min_u16.
__device__ __forceinline__ uint32_t nsq_band(uint32_t x)
{
    const u16x2 v = __builtin_bit_cast(u16x2, x);
    return __builtin_bit_cast(uint32_t, (u16x2)(v + (v >> 3)));
}
__device__ __forceinline__ uint32_t nsq_root(uint32_t v) // floor(sqrt(v - 72)), exact for v - 72 <= 32768
{
    return (uint32_t)__builtin_amdgcn_sqrtf((float)v - ((float)kNsqBias - 0.5f));
}

#ifndef ADSB_NSQ_AHEAD
#define ADSB_NSQ_AHEAD 12 // granules of four pairs resident ahead of the current block in the nsq gate (>= 8)
#endif
template <bool F16OK>
__device__ __forceinline__ void gate_phase_nsq(const uint32_t *img, uint32_t *cand, uint16_t *list, uint32_t *count,
                                               const uint32_t tid, const uint32_t n_valid)
{
    constexpr int RUN = kRun, NT = kThreads;
    uint32_t *candA = cand + tid, *candB = cand + (tid + NT);
    *candA = 0u;
    *candB = 0u;
    // run A = offsets 32 tid + o, run B = kNsqHalf + 32 tid + o: logical dwords 32 tid + j, j < RUN + 26: this lane's
    // 32 and the first 28 of the next lane's (which may lie behind a pad)
    const u32x4 *g0 = reinterpret_cast<const u32x4 *>(img + nsq_phys(32 * tid));
    const u32x4 *g1 = reinterpret_cast<const u32x4 *>(img + nsq_phys(32 * tid + 32));
    constexpr int kGran = (RUN + 26 + 3) / 4; // 15 granules of four pairs
    constexpr int kAhead = ADSB_NSQ_AHEAD;    // 48 pairs resident ahead of the current block
    uint32_t N[kGran * 4];
    auto fetch = [&](int g) {
        const u32x4 x = g < 8 ? g0[g] : g1[g - 8];
        N[4 * g] = x.x; N[4 * g + 1] = x.y; N[4 * g + 2] = x.z; N[4 * g + 3] = x.w;
    };
#pragma unroll
    for (int g = 0; g < kAhead; ++g) fetch(g);
    //   N[j]  pair of values               H2[j] = min(N[j], N[j+2])
    //   W3[j] = max(N[j..j+2])             F[j]  = max(N[j], W3[j+2], N[j+5])
    // highs of offset o: min(H2[o], H2[o+7]);  lows: max(F[o+1], F[o+8], W3[o+13])
    uint32_t H2[RUN + 8], W3[RUN + 16], F[RUN + 9];
#pragma unroll
    for (int j = 0; j < 7; ++j) H2[j] = pkmin(N[j], N[j + 2]);
#pragma unroll
    for (int j = 3; j < 13; ++j) W3[j] = pkmax3<F16OK>(N[j], N[j + 1], N[j + 2]);
#pragma unroll
    for (int j = 1; j < 8; ++j) F[j] = pkmax3<F16OK>(N[j], W3[j + 2], N[j + 5]);

    // [phase:2 nsq gate: steps]
#pragma unroll
    for (int o = 0; o < RUN; ++o) {
        if (o % 4 == 0) { // keep 48 pairs resident ahead of the block that starts here
            const int g = o / 4 + kAhead;
            if (g < kGran) fetch(g);
        }
        W3[o + 13] = pkmax3<F16OK>(N[o + 13], N[o + 14], N[o + 15]);
        F[o + 8] = pkmax3<F16OK>(N[o + 8], W3[o + 10], N[o + 13]);           // lows 8,10,11,12,13
        const uint32_t lo = pkmax3<F16OK>(F[o + 1], F[o + 8], W3[o + 13]);   // + 1,3,4,5,6 + 13,14,15
        H2[o + 7] = pkmin(N[o + 7], N[o + 9]);
        const uint32_t hi = pkmin(H2[o], H2[o + 7]);                      // highs 0,2,7,9
        const uint32_t t = nsq_band(hi);
        const bool pa = (uint16_t)t >= (uint16_t)lo;
        const bool pb = (t >> 16) >= (lo >> 16);
        // [phase:2 nsq gate: DF17 (cold)]
        // wave-uniform tests (scalar branches, no exec juggling): a block is entered by the whole wave when any
        // lane needs it; its effects are masked by the lanes' own flags
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(pa | pb) != 0, 0)) {
            // DF17 part of the gate (demod.rs:45-54), the same superset test
            const uint32_t dh = pkmin3<F16OK>(pkmin3<F16OK>(N[o + 16], N[o + 19], N[o + 21]), N[o + 23], N[o + 24]);
            const uint32_t dl = pkmax3<F16OK>(pkmax3<F16OK>(N[o + 17], N[o + 18], N[o + 20]), N[o + 22], N[o + 25]);
            const uint32_t t2 = nsq_band(dh);
            bool sa = pa & ((uint16_t)t2 >= (uint16_t)dl);
            bool sb = pb & ((t2 >> 16) >= (dl >> 16));
            if (__builtin_amdgcn_ballot_w64(sa | sb) != 0) {
                // inside both bands.  Exact at once where both groups are ordered on n itself ...
                const bool ea = ((uint16_t)hi >= (uint16_t)lo) & ((uint16_t)dh >= (uint16_t)dl);
                const bool eb = ((hi >> 16) >= (lo >> 16)) & ((dh >> 16) >= (dl >> 16));
                // [phase:2 nsq gate: roots (cold)]
                if (__builtin_expect(__builtin_amdgcn_ballot_w64((sa & !ea) | (sb & !eb)) != 0, 0)) {
                    // ... the rest by the truncated roots themselves (utils.rs:46-52): ties after truncation pass
                    const bool ra = nsq_root(hi & 0xFFFFu) >= nsq_root(lo & 0xFFFFu) && nsq_root(dh & 0xFFFFu) >= nsq_root(dl & 0xFFFFu);
                    const bool rb = nsq_root(hi >> 16) >= nsq_root(lo >> 16) && nsq_root(dh >> 16) >= nsq_root(dl >> 16);
                    sa = sa && (ea || ra);
                    sb = sb && (eb || rb);
                }
                // (offsets at or beyond n_valid are masked out of the bitmap words afterwards, in the one tile per
                // channel that has any)
                uint32_t bit = 1u << o;
                asm("" : "+v"(bit)); // one v_mov for both stores
                if (sa) atomicOr(candA, bit);
                if (sb) atomicOr(candB, bit);
            }
        }
    }
    // [phase:2 nsq gate: survivor list]
    gate_collect<RUN, NT>(candA, candB, list, count, tid, n_valid);
}

// [phase:3 slice_byte (nsq image)]
// The same slice from the nsq image (i8, kScanNsq).  The reference compares truncated roots (demod.rs:106 on the
// output of utils.rs:46-52): bit = floor(sqrt(x)) > floor(sqrt(y)) = (r * r > y) with r = floor(sqrt(x)) -- r * r is the
// largest square <= x, so a square lies in (y, x] exactly when r * r > y.  One root per PAIR, survivors only
// (224 samples per survivor ~ 0.1 roots per sample of the stream).  r = trunc(sqrtf(x + 0.5)) is exact for x <= 32768
// (sqrt(x + 0.5) is >= 1.3e-3 from every integer there; v_sqrt_f32 errs by 1 ulp ~ 1e-5).
// A 16-lane group works on one survivor at tile offset `off`; the group's window of 224 samples starts at logical
// dword q + 16 of its half (half = off >= kNsqHalf).  Lane l reads the 16 consecutive samples of 16-aligned chunk
// (q + 16) / 16 + l, moved up by one sample when q + 16 is odd (so that pairs never straddle two lanes), slices its
// 8 pairs, and frame byte l is put together from the chunks of lanes l and l + 1 (one DPP row shift):
// chunk bit j of lane l is frame bit 8 l + j - sh, sh = ((q + 16) % 16) / 2.  All 16 lanes of a group must be active.
__device__ __forceinline__ uint32_t nsq_slice_byte(const uint32_t *img, const uint32_t off, const uint32_t l)
{
    const uint32_t half = off >= (uint32_t)kNsqHalf ? 1u : 0u;
    const uint32_t base = off - half * (uint32_t)kNsqHalf + 16u; // logical dword of the first data sample
    const uint32_t e = base & 15u, par = e & 1u, sh = e >> 1;
    const uint32_t v = (base >> 4) + l;                            // this lane's 16-sample chunk
    const uint32_t a1 = nsq_phys(16u * v) + par;                  // physical dword of its first sample
    // its last sample sits behind a pad when the chunk ends a padded block and was moved up by one
    constexpr uint32_t kChunksPerBlock = (1u << kNsqPadShift) / 16u;
    const uint32_t a2 = a1 + 15u + (((v & (kChunksPerBlock - 1u)) == kChunksPerBlock - 1u ? 4u : 0u) & (0u - par));
    uint32_t d[16];
#pragma unroll
    for (int j = 0; j < 15; ++j) d[j] = img[a1 + j];
    d[15] = img[a2];
    // (x, y) of a pair into one register: x in the low half, y in the high half (selectors 0-3: 2nd operand)
    const uint32_t sel = half ? 0x07060302u : 0x05040100u;
    uint32_t w[8], r2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        w[j] = __builtin_amdgcn_perm(d[2 * j + 1], d[2 * j], sel);
        const float fx = (float)(w[j] & 0xFFFFu) - ((float)kNsqBias - 0.5f); // n + 0.5
        const uint32_t r = (uint32_t)__builtin_amdgcn_sqrtf(fx);
        r2[j] = __umul24(r, r) + (uint32_t)kNsqBias; // (r <= 181; one v_mad_u32_u24)
    }
    // bit j = r2 > y, MSB first: one SDWA compare per pair into its own SGPR pair, then chunk = chunk + chunk +
    // carry-in per pair (v_addc): no v_cndmask.  All eight compares come first: gfx950 wants 2 wait states between a
    // VALU writing an SGPR and a VALU reading it, and hipcc pads nothing inside asm.
    uint32_t chunk = 0;
    uint64_t m0, m1, m2, m3, m4, m5, m6, m7;
    asm("v_cmp_gt_u32_sdwa %1, %9, %17 src0_sel:DWORD src1_sel:WORD_1\n\t"
        "v_cmp_gt_u32_sdwa %2, %10, %18 src0_sel:DWORD src1_sel:WORD_1\n\t"
        "v_cmp_gt_u32_sdwa %3, %11, %19 src0_sel:DWORD src1_sel:WORD_1\n\t"
        "v_cmp_gt_u32_sdwa %4, %12, %20 src0_sel:DWORD src1_sel:WORD_1\n\t"
        "v_cmp_gt_u32_sdwa %5, %13, %21 src0_sel:DWORD src1_sel:WORD_1\n\t"
        "v_cmp_gt_u32_sdwa %6, %14, %22 src0_sel:DWORD src1_sel:WORD_1\n\t"
        "v_cmp_gt_u32_sdwa %7, %15, %23 src0_sel:DWORD src1_sel:WORD_1\n\t"
        "v_cmp_gt_u32_sdwa %8, %16, %24 src0_sel:DWORD src1_sel:WORD_1\n\t"
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %1\n\t"
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %2\n\t"
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %3\n\t"
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %4\n\t"
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %5\n\t"
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %6\n\t"
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %7\n\t"
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %8"
        : "+v"(chunk), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3), "=&s"(m4), "=&s"(m5), "=&s"(m6), "=&s"(m7)
        : "v"(r2[0]), "v"(r2[1]), "v"(r2[2]), "v"(r2[3]), "v"(r2[4]), "v"(r2[5]), "v"(r2[6]), "v"(r2[7]),
          "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]), "v"(w[4]), "v"(w[5]), "v"(w[6]), "v"(w[7])
        : "vcc");
    const uint32_t next = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)chunk, 0x101 /* row_shl:1 */, 0xF, 0xF, true);
    return (((chunk << 8) | next) >> (8u - sh)) & 0xFFu;
}

// [phase:end]
// The tile body of the nsq scan (same contract as scan_tile: Seg, slots, header flags).  smem: NsqLds::kTotal bytes, 16-byte
// aligned.
__device__ __forceinline__ void scan_tile_nsq(const DemodArgs &p, const uint32_t tile, const bool first, unsigned char *smem)
{
    typedef NsqLds L;
    static_assert(kThreads / 64 <= 4, "misc[4 + wave] must stay below misc[8]");
    uint32_t *img = reinterpret_cast<uint32_t *>(smem);
    uint32_t *cand = reinterpret_cast<uint32_t *>(smem + L::kOffCand);
    uint16_t *list = reinterpret_cast<uint16_t *>(smem + L::kOffList);
    uint32_t *misc = reinterpret_cast<uint32_t *>(smem + L::kOffMisc);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const TilePos tp = tile_pos<kTile>(p, tile);
    // [phase:1 nsq (loads, dots, stores)]
    u32x4 raw_a[kNsqIters], raw_b[kNsqIters];
    nsq_issue_loads(p, tp, tid, raw_a, raw_b); // the loads go out before anything else
    tile_prologue(p, first, misc, tid);
    const bool wave_big = nsq_image_to_lds(raw_a, raw_b, img, tid);
    if (lane == 0) misc[4 + wave] = wave_big ? 1u : 0u; // (every wave writes its own word)
    __syncthreads();
    // [phase:2 nsq gate: call]
    // the 3-input f16 gate whenever every value of the tile is an ordered f16 pattern (unless some sample has |I| and |Q|
    // >= 125); the integer gate otherwise
    uint32_t any_big = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) any_big |= misc[4 + w];
    if (any_big == 0) gate_phase_nsq<true>(img, cand, list, &misc[12], tid, tp.n_valid); // (workgroup-uniform)
    else gate_phase_nsq<false>(img, cand, list, &misc[12], tid, tp.n_valid);
    __syncthreads();
    // [phase:3 hand-over: slots, offsets, sliced bytes]
    hand_over<kTile, 32>(p, tile, tp.sample0, misc[12], cand, list, misc, tid, lane, wave,
                         [img](const bool, const uint32_t off, const uint32_t l, bool &dropped) {
                             dropped = false; // (the slicer compares the truncated roots themselves)
                             return nsq_slice_byte(img, off, l);
                         });
    // [phase:end]
}

#if ADSB_AB_KERNELS
__global__ __launch_bounds__(kThreads, ADSB_SCAN_WAVES) void demod_tiles_nsq(DemodArgs p)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[NsqLds::kTotal];
    scan_tile_nsq(p, p.tile_first + tile_of_workgroup(blockIdx.x, p.tile_count), blockIdx.x == 0, smem);
}
#endif

// (compiled in every build: adsb_debug_nsq_values is part of the C ABI)
// nsq test hook: v = I^2 + Q^2 + 72 of n i8 samples through the scan kernel's own packing code (every group of 8
// samples is packed once as the "A" AND the "B" operand: both halves must agree, else 0xFFFF is reported).
__global__ void nsq_values_kernel(const void *iq, size_t n, uint16_t *out)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t groups = (n + 7) / 8;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        const uint16_t *src = reinterpret_cast<const uint16_t *>(iq) + g * 8;
        uint16_t tmp[8];
        for (int k = 0; k < 8; ++k) tmp[k] = (g * 8 + k < n) ? src[k] : (uint16_t)0;
        u32x4 v;
        v.x = tmp[0] | ((uint32_t)tmp[1] << 16);
        v.y = tmp[2] | ((uint32_t)tmp[3] << 16);
        v.z = tmp[4] | ((uint32_t)tmp[5] << 16);
        v.w = tmp[6] | ((uint32_t)tmp[7] << 16);
        uint32_t d[8];
        nsq_pack16(v, v, d);
        for (int k = 0; k < 8; ++k)
            if (g * 8 + k < n) out[g * 8 + k] = (d[k] & 0xFFFFu) == (d[k] >> 16) ? (uint16_t)(d[k] & 0xFFFFu) : (uint16_t)0xFFFFu;
    }
}

hipError_t launch_nsq_values(hipStream_t s, const void *iq, size_t n, uint16_t *out)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(nsq_values_kernel, dim3(1024), dim3(256), 0, s, iq, n, out);
    return hipGetLastError();
}
