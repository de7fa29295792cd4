// adsb_track.hip -- what the reference does right behind the AdsbPacket channel, for one launch's ordered
// frame list, on the device: the per-ICAO tracker (src/adsb/aircraft.rs:48-165) and the global CPR position
// decode it calls (src/adsb/cpr.rs:22-147).  SURVEY section 8(f) rank 3.
//
// The reference runs a sequential state machine per packet: per ICAO it remembers the last even and the
// last odd position message; a new position message pairs with the last one of the other format if that
// one is at most 10 s old, and the pair yields a latitude/longitude (`first` = the older format).  In
// closed form, for position frame i:   j = the latest frame before i with the same ICAO, a position
// message, the other CPR format;  if j exists and t_i - t_j <= 10 s: position(i) = cpr(pair, first = j).
// That is a "previous matching element in my segment" query:
//   1. stable radix sort of frame indices by ICAO (24 bits; rocPRIM) -> one segment per aircraft, list
//      order (= time order) inside;
//   2. one thread per frame walks back in its segment to its partner (bounded by the 10 s window: an
//      older partner could not be used anyway) and evaluates the CPR formulas in f64;
//   3. one thread per segment tail gathers the aircraft's record (callsign of the last ID message,
//      altitude and time of the last position message, last position that was computed).
// Time is sample offset x seconds_per_sample (the reference stamps packets with the wall clock, which
// is excluded from parity).  O(frames) work, a few MB: a latency-bound epilogue.
//
// The same kernels also serve a persistent aircraft table (adsb_track_table_*; TrackKind::kTable, its device view a
// TrackStoreDev with one receiver): the reference
// keeps ONE HashMap<u32, Aircraft> for the life of its display thread (tui.rs:22-42, web.rs:115), so a pair may
// straddle two launches.  With a table, two steps go between 1. and 2.:
//   1a. per segment, the aircraft's record slot from a direct ICAO index (2^24 words, 0 = absent);
//   1b. an exclusive scan over "new ICAO" segment heads ranks this list's new aircraft in ascending ICAO order,
//       which is the order they are admitted in while the table has room (the rest are UNTRACKED);
// 2. falls back, when its walk reaches the segment start with the window still open, to the record's last
// even / odd position message from before this list; 3. merges the segment into the record in place (one
// thread per segment = per distinct ICAO: no atomics).
//
// A bank (adsb_track_bank_*; TrackKind::kBank, the same TrackStoreDev with N receivers) is N such tables, one per
// receiver, updated by ONE dispatch sequence over a multi-channel list (receiver r's frames, then receiver r+1's,
// ...).  The sort key becomes receiver << 24 | icao over 24 + ceil(log2 N) bits, so segments never mix receivers and
// receiver r's frames sit at [prefix[r], prefix[r+1]) in sorted order.  A direct 2^24 index per receiver would cost 64
// MiB x N, so 1a probes an open-addressing hash of the key instead, once per segment head; 1b scans (segment head, new
// key) pairs in one 64-bit word, which gives every frame its segment and every new key its rank, made per receiver by
// subtracting the rank at prefix[r].  Slots come from that rank alone (receiver r's records live at [r x max_aircraft,
// (r+1) x max_aircraft)), never from where the hash put an entry, so no result depends on insert order.
//
// Table and bank share everything but how a segment finds its record slot (keys, lookup, admit: the table's direct
// index with a 32-bit scan, the bank's hash with a 64-bit one).  What follows admission -- pairs, summaries, merge, and
// expire's mark and compaction -- is one kernel template over TrackKind that reads the state words size[r], flags[r],
// size_next[r] of receiver r, r = 0 for a table.
//
// Expire (adsb_track_table_expire / adsb_track_bank_expire) evicts every record whose last frame of any kind is older
// than a cut, without a host round trip: a mark kernel flags the survivors of [0, size) (sized by max_aircraft, the
// size being a device word), a rocPRIM scan ranks them, and a compaction kernel closes the holes in place: the k-th
// survivor at or above the new size moves into the k-th hole below it, so sources and destinations are disjoint.  The
// table's direct index is fixed by the same kernel (evicted ICAOs cleared, moved ones rewritten); a bank's hash cannot
// drop entries (a hole in a probe chain would hide later keys), so it is cleared and every survivor reinserted.  A bank
// does this per receiver region with one scan over all receivers, each region's rank made local as admission does.
//
// Airborne velocity (DF17 TC 19, which the reference leaves undecoded): with a table or bank, step 3 also finds the
// segment's newest velocity message of subtype 1-4 on its walk and decodes it from the frame bytes into the record's
// `vel`; a segment without one keeps the record's.  Admission starts a record with none, expire moves whole records,
// and the per-launch form (adsb_track_device) has no velocity.
//
// The fused view (adsb_track_bank_fuse) turns a bank's N maps into one picture, each ICAO once, without touching the
// bank: a key kernel writes icao << rbits | receiver for every contributing record (held, last_heard >= since) and
// 1 << (24 + rbits) for every other place, so those sort last and never look like an aircraft (all ones would:
// ICAO FFFFFF on the last of 2^rbits receivers); a rocPRIM sort over 25 + rbits bits makes one run per ICAO with its
// receivers ascending; a scan of the ICAO changes numbers the runs; one group of 1 or 4 lanes per run picks, per
// quantity, the record with the greatest time (ties: the lowest sorted position = the lowest receiver), and the
// workgroup writes its 128-byte output records once, through LDS.  All sizes are device words; the total and the
// truncation flag are published by the last thread of the kernel that stores the run starts.
//
// Per-frame summaries and the changed list (adsb_track_*_summaries_reserve; a table or bank that reserved): what the
// reference's web thread broadcasts, the packet's aircraft as it stands right after every packet (web.rs:117-128).
// Between 2. and 3. (3. overwrites the record the summaries start from): one segmented inclusive max-scan over the
// sorted list (rocPRIM, a 20-byte tuple computed by a transform iterator) gives every frame the sorted position of its
// segment's head and of the last identification message, position message and new position at or before it, plus its
// segment's rank among the tracked ones; one thread per frame then builds the 48-byte summary from at most three source
// frames and the pre-update record, with 3.'s expressions, and stores it at the frame's list index; segment tails
// write their record slot at their rank (the changed list).  Linear in the list however long one aircraft's part is.
//
// Per-aircraft signal levels (adsb_track_*_levels_reserve; the *_update_levels forms): a side array of one 64-byte
// adsb_aircraft_level per record place.  After 2. (which fixes a bank's d.slot), independent of 3.: one segmented
// inclusive scan over the sorted list (rocPRIM, a 48-byte tuple computed by a transform iterator from the frame's level
// record) adds up every segment's counted frames by saturating add / max / "later sorted position"; one thread per
// segment tail merges the result into the side record at slot - 1 and reads last_* from the newest counted frame.
// Admission empties the level record of a place it admits, expire's compaction moves it with the record; both only when
// the side array exists.  The fused view gets one adsb_fused_level per fused record from a kernel of its own after the
// reduction: one thread per ICAO run picks the receiver with the greatest mean by exact cross-multiplication.
//
// Positions from single messages (adsb_track_*_fixes_reserve): a side array of one 64-byte adsb_fix per record place and
// one site per receiver.  After 2., independent of 3.: one thread per frame decodes its bytes against its receiver's site
// (adsb_fix.h: the locally unambiguous CPR decode, range and bearing; the text the CPU mirror compiles too), one
// segmented inclusive scan (16-byte tuple) finds every segment's newest accepted position message and counts, one thread
// per segment tail merges into the side record.  Admission empties the fix of a place it admits, expire's compaction
// moves it with the record; both only when the side array exists.
//
// Multilaterated positions per aircraft (adsb_track_table_mlat_reserve; the update_mlat form): a third side array, one
// 64-byte adsb_aircraft_mlat per record place.  After 2., independent of 3.: one thread per frame takes the frame, its
// adsb_mlat_fix and its slot through adsb_track_mlat.h (the single-message decode with the solved position as the site;
// the text the CPU mirror compiles too) into one adsb_frame_mlat at the list index and one scan operand at the sorted
// position, one segmented inclusive scan (32-byte tuple: integers and one float max) finds every segment's newest valid
// fix, newest checked frame, greatest disagreement and counts, one thread per segment tail merges into the side record.
// Admission and expire treat the array as they treat the other two.  Tables only; the templates compile for a bank too.
//
// Filtered mlat track per aircraft (adsb_track_table_filter_reserve; every update given fixes): a side array of one
// 192-byte adsb_aircraft_filter per record place.  Behind the mlat merge, since it needs d.slot, the sort and the fixes
// and nothing more: one thread per sorted frame writes the frame's 64-byte operand at its sorted position (all the
// trigonometry; adsb_track_filter.h, the text the CPU mirror compiles too), one thread per segment HEAD -- the mirror
// image of the merge kernels' tails -- loads the record, steps through its segment's consecutive operands and stores the
// record once.  No scan: a Kalman step does not combine associatively at a price worth paying, so the critical path is
// the longest aircraft's part of the list, not the list.  Admission and expire treat the array as they treat the
// others.  Tables only.
//
// Mode S replies per aircraft (adsb_track_table_modes_reserve; the update_modes form): a fourth side array, one 64-byte
// adsb_aircraft_modes per record place, and a list keyed by adsb_modes_of's addresses.  Instead of track_keys_kernel, a key
// kernel of its own reads the frame's adsb_modes_rec: the sort key is the address of an accepted frame and 1 << 24 for
// every other one (25 sorted bits: the rejected frames form one last segment), and every frame that is not an accepted
// DF17/18 becomes a frame of kind "other" in the table's fields.  The lookup of such an update gives the last segment no
// slot (kTrackUntracked, never new), so admission, pairs, summaries and the three merges above skip it as they skip an
// aircraft the full table turned away, unchanged.  After them: one thread per frame writes its point (UNADDRESSED) and
// icao where those kernels left the sentinel, and the scan operand of adsb_track_modes.h's contribution at its sorted
// position; one segmented inclusive scan (48-byte tuple, integers only); one thread per segment tail builds the
// segment's part from the winning frames' records and merges it into the side record.  Admission and expire treat the
// array as they treat the other three.  Tables only.
//
// Comm-B registers per aircraft (adsb_track_table_commb_reserve; the update_commb form): a fifth side array, one 128-byte
// adsb_aircraft_commb per record place.  After everything update_modes launches and BEFORE the merge into the main
// records (track_summary_kernel overwrites rec.vel, and the settle reads the velocity held from before this update): one
// segmented scan gives every sorted frame its aircraft's newest velocity frame up to it, one thread per frame settles an
// ambiguous {5,0; 6,0} record against the newest EARLIER one (its predecessor's scan word) or the held velocity
// (adsb_track_commb.h), writes the per-frame output at the list index and a 40-byte operand at the sorted position, one
// segmented inclusive scan, one thread per segment tail merges into the side record.  Tables only.
//
// Extended squitter status per aircraft (adsb_track_table_es_reserve; the update_es form): a sixth side array, one
// 256-byte adsb_aircraft_es per record place.  Beside the levels / fix / mlat merges, since it needs the sort, d.slot
// and its own side array only, and behind either key kernel (a plain key is below kModesNoAddress): one segmented scan
// gives every sorted frame its aircraft's newest frames with a version and with NIC supplements A and C up to it, one
// thread per frame resolves a position message against the newest EARLIER ones (its predecessor's scan words) or the
// held record (adsb_track_es.h), writes the per-frame output at the list index and a 56-byte operand at the sorted
// position, one segmented inclusive scan, one thread per segment tail merges into the side record.  Tables only.
#include <hip/hip_runtime.h>

#include <cstring>

#include <rocprim/rocprim.hpp>

#include "adsb_fix.h"
#include "adsb_kernels.h"
#include "adsb_track_mlat.h"
#include "adsb_track_filter.h"
#include "adsb_track_commb.h"
#include "adsb_track_es.h"
#include "adsb_track_modes.h"

namespace adsbk {

namespace {

__device__ __forceinline__ double cpr_to_float(uint32_t cpr) { return (double)cpr / 131072.0; } // cpr.rs:22-25

// calc_num_zones (cpr.rs:39-54), floor_as_u32 and me_bits: adsb_fix.h, shared with the single-message decode

// cpr.rs:135-147 (+ 63-88, 90-127); first_is_odd: the older message's format
__device__ bool geographic_position(uint32_t even_lat_u, uint32_t even_lon_u, uint32_t odd_lat_u, uint32_t odd_lon_u,
                                    bool first_is_odd, double &latitude, double &longitude)
{
    const double even_cpr_lat = cpr_to_float(even_lat_u), odd_cpr_lat = cpr_to_float(odd_lat_u);
    const double latitude_index = floor(59.0 * even_cpr_lat - 60.0 * odd_cpr_lat + 0.5);
    const double even_latitude = (360.0 / 60.0) * (fmod(latitude_index, 60.0) + even_cpr_lat);
    const double odd_latitude = (360.0 / 59.0) * (fmod(latitude_index, 59.0) + odd_cpr_lat);
    double lat = first_is_odd ? even_latitude : odd_latitude; // the newest format decides
    if (lat > 270.0) lat -= 360.0;
    if (calc_num_zones(even_latitude) != calc_num_zones(odd_latitude)) return false;

    const double lon_cpr_e = cpr_to_float(even_lon_u), lon_cpr_o = cpr_to_float(odd_lon_u);
    const uint32_t nl = calc_num_zones(lat);
    uint32_t nz = first_is_odd ? calc_num_zones(lat) : calc_num_zones(lat - 1.0); // sic: latitude - 1.0
    if (nz < 1) nz = 1;
    const double num_zones = (double)nz;
    const double divisions = 360.0 / num_zones;
    const double m = floor(lon_cpr_e * (double)(uint32_t)(nl - 1u) - lon_cpr_o * (double)nl + 0.5);
    double lon = first_is_odd ? divisions * (fmod(m, num_zones) + lon_cpr_e)
                              : divisions * (fmod(m, num_zones) + lon_cpr_o);
    while (lon < -180.0) lon += 360.0;
    while (lon > 180.0) lon -= 360.0;
    latitude = lat;
    longitude = lon;
    return true;
}

__global__ __launch_bounds__(256) void track_keys_kernel(const adsb_packet_fields *fields, uint32_t n, uint32_t *keys,
                                                         uint32_t *vals)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = fields[i].icao & 0xFFFFFFu;
    vals[i] = i;
}

__device__ __forceinline__ double frame_time(const adsb_frame *frames, uint32_t i, uint64_t sample_base,
                                             double seconds_per_sample)
{
    // the header's t, one ROUNDED product.  Contraction is off for this multiply (hipcc contracts by default, and here
    // __dmul_rn is a plain product that contracts too): inlined into fabs(t_i - t_j) > 10.0 it would otherwise become
    // fma(-x_j, sps, t_i) with x_j * sps unrounded, which calls about half of the pairs that are exactly 10 s apart
    // at 0.5e-6 s per sample too old, while the record fallback, the oracle and the host mirror accept them
#pragma clang fp contract(off)
    return (double)(sample_base + frames[i].offset) * seconds_per_sample;
}

__device__ __forceinline__ TrackRecord empty_record(uint32_t icao)
{
    TrackRecord rec;
    rec.a.latitude = 0.0;
    rec.a.longitude = 0.0;
    rec.a.last_contact = __builtin_nan("");
    rec.a.icao = icao;
    rec.a.altitude = 0;
    rec.a.has_position = 0;
    rec.a.n_frames = 0;
    for (int k = 0; k < 8; ++k) rec.a.callsign[k] = 0;
    rec.t_even = 0.0;
    rec.t_odd = 0.0;
    rec.even_lat = rec.even_lon = rec.odd_lat = rec.odd_lon = 0;
    rec.have = 0;
    rec.pad = 0;
    rec.last_heard = 0.0; // the merge of the admitting list sets it
    rec.vel = adsb_velocity{};
    rec.vel.time = __builtin_nan(""); // subtype 0, flags 0: no velocity message yet
    return rec;
}

__device__ __forceinline__ adsb_aircraft_level empty_level()
{
    adsb_aircraft_level l{};
    l.last_time = __builtin_nan("");
    return l;
}

__device__ __forceinline__ uint64_t sat_add64(uint64_t a, uint64_t b)
{
    const uint64_t c = a + b;
    return c < a ? ~0ull : c;
}

__device__ __forceinline__ uint32_t sat_add32(uint32_t a, uint32_t b)
{
    const uint32_t c = a + b;
    return c < a ? ~0u : c;
}

// An airborne-velocity message (DF17 TC 19, ST 1-4; the header's decode rules) from the 14 frame bytes; false for
// ST 0 and 5-7, which are none.  f64 arithmetic with one rounding to f32; the sum of squares is exact in int32.
__device__ bool velocity_decode(const uint8_t *bytes, double time, adsb_velocity &v)
{
    uint64_t me = 0;
    for (int k = 4; k < 11; ++k) me = me << 8 | bytes[k];
    const uint32_t st = me_bits(me, 5, 3);
    if (st < 1 || st > 4) return false;
    const int k = (st == 2 || st == 4) ? 4 : 1;
    v = adsb_velocity{};
    v.time = time;
    v.subtype = (uint8_t)st;
    if (st <= 2) {
        const uint32_t vew = me_bits(me, 14, 10), vns = me_bits(me, 25, 10);
        if (vew != 0 && vns != 0) {
            const int ew = (me_bits(me, 13, 1) ? -1 : 1) * (int)(vew - 1u) * k;
            const int ns = (me_bits(me, 24, 1) ? -1 : 1) * (int)(vns - 1u) * k;
            const double speed = sqrt((double)(ew * ew + ns * ns));
            v.v_ew_kt = (int16_t)ew;
            v.v_ns_kt = (int16_t)ns;
            v.speed_kt = (float)speed;
            v.flags = ADSB_VELOCITY_SPEED;
            if (speed > 0.0) {
                double d = atan2((double)ew, (double)ns) * 180.0 / 3.14159265358979323846264338327950288;
                if (d < 0.0) d += 360.0;
                v.direction_deg = (float)d;
                v.flags |= ADSB_VELOCITY_DIRECTION;
            }
        }
    } else {
        if (me_bits(me, 13, 1)) {
            v.direction_deg = (float)((double)me_bits(me, 14, 10) * 360.0 / 1024.0);
            v.flags = ADSB_VELOCITY_DIRECTION;
        }
        const uint32_t airspeed = me_bits(me, 25, 10);
        if (airspeed != 0) {
            v.speed_kt = (float)((double)(airspeed - 1u) * k);
            v.airspeed_tas = (uint8_t)me_bits(me, 24, 1);
            v.flags |= ADSB_VELOCITY_SPEED;
        }
    }
    const uint32_t vr = me_bits(me, 37, 9);
    if (vr != 0) {
        v.vertical_rate_fpm = (me_bits(me, 36, 1) ? -1 : 1) * (int32_t)(vr - 1u) * 64;
        v.vrate_baro = (uint8_t)me_bits(me, 35, 1);
        v.flags |= ADSB_VELOCITY_VRATE;
    }
    return true;
}

// table only, 1a: the record slot (+1, 0 = absent) of every sorted frame's aircraft; is_new marks the head of a
// segment whose ICAO the table does not hold yet
__global__ __launch_bounds__(256) void track_lookup_kernel(const uint32_t *skeys, uint32_t n, const uint32_t *index,
                                                           uint32_t *slot, uint32_t *is_new)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t icao = skeys[s]; // < 2^24: track_keys_kernel masks
    const uint32_t idx = index[icao];
    slot[s] = idx;
    is_new[s] = (idx == 0 && (s == 0 || skeys[s - 1] != icao)) ? 1u : 0u;
}

// table only, 1b: rank = exclusive scan of is_new; new aircraft get the slots size, size + 1, ... in ascending ICAO
// order while they are below max_aircraft.  The new size goes to size_next[0] (every thread here reads size[0]);
// track_pairs_kernel moves it to size[0].
__global__ __launch_bounds__(256) void track_admit_kernel(const uint32_t *skeys, uint32_t n, const uint32_t *is_new,
                                                          const uint32_t *rank, TrackStoreDev t)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t size0 = t.size[0];
    if (s + 1 == n) {
        const uint64_t grown = (uint64_t)size0 + rank[s] + is_new[s];
        t.size_next[0] = grown < t.max_aircraft ? (uint32_t)grown : t.max_aircraft;
    }
    if (t.slot[s] != 0) return; // the table holds this aircraft
    const bool head = is_new[s] != 0;
    const uint64_t r = (uint64_t)size0 + rank[s] - (head ? 0u : 1u); // a non-head follows its head's 1 in the scan
    if (r >= t.max_aircraft) {
        t.slot[s] = kTrackUntracked;
        if (head) atomicOr(&t.flags[0], ADSB_TRACK_TABLE_FULL);
        return;
    }
    t.slot[s] = (uint32_t)r + 1u;
    if (!head) return;
    const uint32_t icao = skeys[s];
    t.index[icao] = (uint32_t)r + 1u;
    t.rec[r] = empty_record(icao);
    if (t.lvl) t.lvl[r] = empty_level();
    if (t.fix) ((FixWords *)t.fix)[r] = fix_empty();
    if (t.mlat) ((MlatWords *)t.mlat)[r] = mlat_empty();
    if (t.modes) ((ModesWords *)t.modes)[r] = modes_empty();
    if (t.commb) ((CommbWords *)t.commb)[r] = commb_empty();
    if (t.es) ((EsWords *)t.es)[r] = es_track_empty();
    if (t.filter) ((FilterWords *)t.filter)[r] = filter_empty();
}

// bank only: the receiver split clipped to the list (prefix[0] = 0, prefix[k] = n for k >= n_src), as adsb_fetch's
// per_channel_counts cut the first n frames
__device__ __forceinline__ uint32_t bank_prefix(const TrackStoreDev &b, uint32_t k, uint32_t n)
{
    if (k == 0) return 0;
    if (k >= b.n_src) return n;
    const uint64_t p = b.src_prefix[k];
    return p < n ? (uint32_t)p : n;
}

__device__ __forceinline__ uint64_t bank_hash(uint32_t key) // fmix64 (MurmurHash3's finaliser)
{
    uint64_t x = key;
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// bank only: key = receiver << 24 | icao (receiver of frame i: the last k with prefix[k] <= i); threads 0..N also
// write the clipped prefix the later kernels read
__global__ __launch_bounds__(256) void track_bank_keys_kernel(const adsb_packet_fields *fields, uint32_t n,
                                                              TrackStoreDev b, uint32_t *keys, uint32_t *vals)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= b.n_receivers) b.prefix[i] = bank_prefix(b, i, n);
    if (i >= n) return;
    uint32_t lo = 0, hi = b.n_src < b.n_receivers ? b.n_src : b.n_receivers; // prefix[lo] <= i < prefix[hi] (= n)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (bank_prefix(b, mid, n) <= i)
            lo = mid;
        else
            hi = mid;
    }
    keys[i] = lo << 24 | (fields[i].icao & 0xFFFFFFu);
    vals[i] = i;
}

// bank only, 1a: segment heads probe the hash (slot[s] = record slot + 1 or 0); mark = head << 32 | new key
__global__ __launch_bounds__(256) void track_bank_lookup_kernel(const uint32_t *skeys, uint32_t n, TrackStoreDev b)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = skeys[s];
    if (s != 0 && skeys[s - 1] == key) {
        b.mark[s] = 0;
        return;
    }
    uint32_t found = 0;
    for (uint64_t h = bank_hash(key) & b.hash_mask;; h = (h + 1) & b.hash_mask) { // load <= 1/2: an empty entry exists
        const unsigned long long e = b.hash[h];
        if (e == 0) break;
        if ((uint32_t)e == key) {
            found = (uint32_t)(e >> 32);
            break;
        }
    }
    b.slot[s] = found;
    b.mark[s] = 1ull << 32 | (found ? 0u : 1u);
}

// bank only, 1b: excl = exclusive scan of mark: hi = segment number of a head, lo = new keys before s.  A new key of
// receiver r gets slot size[r] + (its rank - the rank at prefix[r]) while that is below max_aircraft; the head
// inserts it into the hash (distinct keys: no two threads insert the same one) and publishes its segment's slot in
// seg_slot.  The last frame of each receiver stages the receiver's new size in size_next (every thread here reads
// size); track_pairs_kernel moves it.
__global__ __launch_bounds__(256) void track_bank_admit_kernel(const uint32_t *skeys, uint32_t n, TrackStoreDev b)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = skeys[s], r = key >> 24;
    const uint64_t m = b.mark[s], e = b.excl[s];
    const uint32_t rank0 = (uint32_t)b.excl[b.prefix[r]], size0 = b.size[r];
    if (s + 1 == b.prefix[r + 1]) {
        const uint64_t grown = (uint64_t)size0 + (uint32_t)e + (uint32_t)m - rank0;
        b.size_next[r] = grown < b.max_aircraft ? (uint32_t)grown : b.max_aircraft;
    }
    if (!(m >> 32)) return; // not a segment head
    const uint32_t g = (uint32_t)(e >> 32);
    if (b.slot[s] != 0) { // the receiver holds this aircraft
        b.seg_slot[g] = b.slot[s];
        return;
    }
    const uint64_t local = (uint64_t)size0 + (uint32_t)e - rank0;
    if (local >= b.max_aircraft) {
        b.seg_slot[g] = kTrackUntracked;
        atomicOr(&b.flags[r], ADSB_TRACK_TABLE_FULL);
        return;
    }
    const uint32_t a = r * b.max_aircraft + (uint32_t)local; // < n_receivers x max_aircraft < 2^32 - 1 (create checks)
    const unsigned long long entry = (unsigned long long)(a + 1u) << 32 | key;
    for (uint64_t h = bank_hash(key) & b.hash_mask;; h = (h + 1) & b.hash_mask)
        if (atomicCAS(&b.hash[h], 0ull, entry) == 0ull) break;
    b.rec[a] = empty_record(key & 0xFFFFFFu);
    if (b.lvl) b.lvl[a] = empty_level();
    if (b.fix) ((FixWords *)b.fix)[a] = fix_empty();
    if (b.mlat) ((MlatWords *)b.mlat)[a] = mlat_empty();
    b.seg_slot[g] = a + 1u;
}

// d: the table / bank (kLaunch: unused, tail_flag instead).  r: the frame's receiver, 0 for a table.
template <TrackKind K>
__global__ __launch_bounds__(256) void track_pairs_kernel(const adsb_frame *frames, const adsb_packet_fields *fields,
                                                          const uint32_t *skeys, const uint32_t *svals, uint32_t n,
                                                          double seconds_per_sample, uint64_t sample_base,
                                                          TrackStoreDev d, adsb_track_point *points,
                                                          uint32_t *tail_flag)
{
    constexpr bool kBank = K == TrackKind::kBank, kStore = K != TrackKind::kLaunch;
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = skeys[s], i = svals[s];
    const uint32_t icao = kBank ? key & 0xFFFFFFu : key, r = kBank ? key >> 24 : 0u;
    adsb_track_point pt;
    pt.latitude = 0.0;
    pt.longitude = 0.0;
    pt.icao = icao;
    pt.flags = 0;
    uint32_t slot = 0;
    if (kStore) {
        if (kBank) sample_base = d.sample_base[r];
        if (s + 1 == (kBank ? d.prefix[r + 1] : n)) d.size[r] = d.size_next[r]; // nothing reads size in this kernel
        if (kBank) { // every frame takes its segment's slot (seg_slot) and keeps it in d.slot for the kernels below
            const bool head = s == 0 || skeys[s - 1] != key;
            slot = d.seg_slot[(uint32_t)(d.excl[s] >> 32) - (head ? 0u : 1u)];
            d.slot[s] = slot;
        } else {
            slot = d.slot[s];
        }
        if (slot == kTrackUntracked) { // turned away by the full table: only icao is valid
            pt.flags = ADSB_TRACK_UNTRACKED;
            points[i] = pt;
            return;
        }
    } else {
        tail_flag[s] = (s + 1 == n || skeys[s + 1] != icao) ? 1u : 0u;
    }
    const adsb_packet_fields f = fields[i];
    if (f.msg_kind == 1) { // AircraftPosition (aircraft.rs:54)
        const bool i_odd = f.cpr_odd != 0;
        const double t_i = frame_time(frames, i, sample_base, seconds_per_sample);
        bool open = true, pair = false; // open: neither a partner nor a frame outside the window found yet
        uint32_t p_lat = 0, p_lon = 0;
        for (uint32_t w = s; w > 0;) {
            --w;
            if (skeys[w] != key) break;
            const uint32_t j = svals[w];
            const double t_j = frame_time(frames, j, sample_base, seconds_per_sample);
            if (fabs(t_i - t_j) > 10.0) { // aircraft.rs:68-70, 84-86: too old (and so is anything before it)
                open = false;
                break;
            }
            const adsb_packet_fields g = fields[j];
            if (g.msg_kind != 1 || g.cpr_odd == f.cpr_odd) continue;
            // the partner: last_odd_packet / last_even_packet at the time frame i arrives
            open = false;
            pair = true;
            p_lat = g.cpr_latitude;
            p_lon = g.cpr_longitude;
            break;
        }
        if (open && kStore) { // the walk reached the segment start: the partner is the record's, from an earlier list
            const TrackRecord &rec = d.rec[slot - 1];
            if (rec.have & (i_odd ? 1u : 2u)) {
                const double t_j = i_odd ? rec.t_even : rec.t_odd;
                if (!(fabs(t_i - t_j) > 10.0)) {
                    pair = true;
                    p_lat = i_odd ? rec.even_lat : rec.odd_lat;
                    p_lon = i_odd ? rec.even_lon : rec.odd_lon;
                }
            }
        }
        if (pair) {
            const uint32_t e_lat = i_odd ? p_lat : f.cpr_latitude, e_lon = i_odd ? p_lon : f.cpr_longitude;
            const uint32_t o_lat = i_odd ? f.cpr_latitude : p_lat, o_lon = i_odd ? f.cpr_longitude : p_lon;
            double lat, lon;
            if (geographic_position(e_lat, e_lon, o_lat, o_lon, /*first_is_odd=*/!i_odd, lat, lon)) {
                pt.latitude = lat;
                pt.longitude = lon;
                pt.flags = ADSB_TRACK_NEW_POSITION;
            }
        }
    }
    points[i] = pt;
}

// one thread per segment tail: without a table, the aircraft's record from an empty map into out[tail_pos];
// with one (or a bank), this list's frames merged into the aircraft's record in place
template <TrackKind K>
__global__ __launch_bounds__(256) void track_summary_kernel(const adsb_frame *frames, const adsb_packet_fields *fields,
                                                            const adsb_track_point *points, const uint32_t *skeys,
                                                            const uint32_t *svals, const uint32_t *tail_flag,
                                                            const uint32_t *tail_pos, uint32_t n,
                                                            double seconds_per_sample, uint64_t sample_base,
                                                            TrackStoreDev d, adsb_aircraft_record *out,
                                                            uint32_t max_aircraft, uint64_t *n_aircraft)
{
    constexpr bool kBank = K == TrackKind::kBank, table = K != TrackKind::kLaunch; // table: a table or a bank
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = skeys[s];
    const uint32_t icao = kBank ? key & 0xFFFFFFu : key;
    if (kBank) sample_base = d.sample_base[key >> 24];
    uint32_t a;
    TrackRecord r;
    if (table) {
        if (s + 1 != n && skeys[s + 1] == key) return;
        a = d.slot[s];
        if (a == kTrackUntracked) return;
        r = d.rec[--a];
    } else {
        if (!tail_flag[s]) return;
        if (s + 1 == n) *n_aircraft = (uint64_t)tail_pos[s] + 1u;
        a = tail_pos[s];
        if (a >= max_aircraft) return;
        r.a = empty_record(icao).a;
    }
    bool have_id = false, have_pos_msg = false, have_fix = false, have_even = false, have_odd = false;
    uint32_t count = 0, vel_j = kTrackUntracked; // vel_j: the newest velocity message (table / bank only)
    for (uint32_t w = s + 1; w > 0;) { // newest to oldest
        --w;
        if (skeys[w] != key) break;
        const uint32_t j = svals[w];
        const adsb_packet_fields g = fields[j];
        ++count;
        if (table && g.msg_type == 19 && vel_j == kTrackUntracked) { // TC 19: ST 1-4 only (velocity_decode)
            const uint32_t st = frames[j].bytes[4] & 7u;
            if (st >= 1 && st <= 4) vel_j = j;
        }
        if (g.msg_kind == 0 && !have_id) { // aircraft.rs:105-107
            have_id = true;
            for (int k = 0; k < 8; ++k) r.a.callsign[k] = g.callsign[k];
        } else if (g.msg_kind == 1) {
            if (!have_pos_msg) { // aircraft.rs:55-56
                have_pos_msg = true;
                r.a.altitude = g.altitude;
                r.a.last_contact = frame_time(frames, j, sample_base, seconds_per_sample);
            }
            if (!have_fix && (points[j].flags & ADSB_TRACK_NEW_POSITION)) { // aircraft.rs:97-102
                have_fix = true;
                r.a.has_position = 1;
                r.a.latitude = points[j].latitude;
                r.a.longitude = points[j].longitude;
            }
            if (table && g.cpr_odd && !have_odd) { // aircraft.rs:80-82
                have_odd = true;
                r.have |= 2u;
                r.odd_lat = g.cpr_latitude;
                r.odd_lon = g.cpr_longitude;
                r.t_odd = frame_time(frames, j, sample_base, seconds_per_sample);
            } else if (table && !g.cpr_odd && !have_even) { // aircraft.rs:64-66
                have_even = true;
                r.have |= 1u;
                r.even_lat = g.cpr_latitude;
                r.even_lon = g.cpr_longitude;
                r.t_even = frame_time(frames, j, sample_base, seconds_per_sample);
            }
        }
    }
    r.a.n_frames += count;
    if (table) {
        r.last_heard = frame_time(frames, svals[s], sample_base, seconds_per_sample); // the segment's last frame
        if (vel_j != kTrackUntracked)
            (void)velocity_decode(frames[vel_j].bytes, frame_time(frames, vel_j, sample_base, seconds_per_sample),
                                  r.vel);
        d.rec[a] = r;
    } else {
        out[a] = r.a;
    }
}

// ---- per-frame summaries and the changed list (table / bank with a summaries reserve) -----------------------------
// The scan's input at sorted position s, computed where the scan loads it (no tuple buffer, no kernel of its own):
// s + 1 in every component that frame s "writes", by the merge's own tests.  Frames of an aircraft the table turned
// away write nothing and are not counted.
struct SumInput {
    const uint32_t *skeys, *svals, *slot;
    const adsb_packet_fields *fields;
    const adsb_track_point *points;
    __device__ __forceinline__ TrackSumTuple operator()(uint32_t s) const
    {
        const bool head = s == 0 || skeys[s - 1] != skeys[s];
        const bool tracked = slot[s] != kTrackUntracked;
        const uint32_t i = svals[s], kind = fields[i].msg_kind, at = tracked ? s + 1u : 0u;
        TrackSumTuple v;
        v.head = head ? s + 1u : 0u;
        v.id = kind == 0 ? at : 0u;                                                       // aircraft.rs:105-107
        v.pos = kind == 1 ? at : 0u;                                                      // aircraft.rs:55-56
        v.fix = (kind == 1 && (points[i].flags & ADSB_TRACK_NEW_POSITION)) ? at : 0u;     // aircraft.rs:97-102
        v.cnt = (head && tracked) ? 1u : 0u;
        return v;
    }
};

// Segmented max: a right operand that holds a segment head starts over (its components are those of its last
// segment); otherwise the left head stays and the later writer wins.  Associative, so the scan's result does not depend
// on how rocPRIM groups the operands; cnt is summed across segments.
struct SumOp {
    __device__ __forceinline__ TrackSumTuple operator()(const TrackSumTuple &l, const TrackSumTuple &r) const
    {
        TrackSumTuple o = r;
        if (!r.head) {
            o.head = l.head;
            o.id = l.id > r.id ? l.id : r.id;
            o.pos = l.pos > r.pos ? l.pos : r.pos;
            o.fix = l.fix > r.fix ? l.fix : r.fix;
        }
        o.cnt = l.cnt + r.cnt;
        return o;
    }
};

// One thread per sorted frame s, after the scan and BEFORE the merge (d.rec[slot] still is the record from before this
// update; admission wrote empty_record for a new aircraft): the aircraft as Aircraft::handle_packet leaves it after
// frame s, from at most three source frames and that record, with the merge's expressions, stored at the frame's list
// index.  A segment tail also puts its record slot on the changed list at its rank.
template <TrackKind K>
__global__ __launch_bounds__(256) void track_frame_summary_kernel(const adsb_frame *frames,
                                                                  const adsb_packet_fields *fields,
                                                                  const adsb_track_point *points, const uint32_t *skeys,
                                                                  const uint32_t *svals, uint32_t n,
                                                                  double seconds_per_sample, uint64_t sample_base,
                                                                  TrackStoreDev d, TrackSumDev sum)
{
    constexpr bool kBank = K == TrackKind::kBank;
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = skeys[s], i = svals[s], slot = d.slot[s];
    const uint32_t icao = kBank ? key & 0xFFFFFFu : key;
    if (kBank) sample_base = d.sample_base[key >> 24];
    const TrackSumTuple w = sum.scan[s];
    if (s + 1 == n) *sum.n_changed = w.cnt;
    adsb_aircraft_record r;
    if (slot == kTrackUntracked) {
        r = empty_record(icao).a;
    } else {
        r = d.rec[slot - 1].a;
        r.icao = icao;
        if (w.id) {
            const adsb_packet_fields g = fields[svals[w.id - 1]];
            for (int k = 0; k < 8; ++k) r.callsign[k] = g.callsign[k];
        }
        if (w.pos) {
            const uint32_t j = svals[w.pos - 1];
            r.altitude = fields[j].altitude;
            r.last_contact = frame_time(frames, j, sample_base, seconds_per_sample);
        }
        if (w.fix) {
            const uint32_t j = svals[w.fix - 1];
            r.has_position = 1;
            r.latitude = points[j].latitude;
            r.longitude = points[j].longitude;
        }
        r.n_frames += s + 2u - w.head; // w.head - 1 = the segment's first sorted position
        if (s + 1 == n || skeys[s + 1] != key) sum.changed[w.cnt - 1] = slot - 1; // a tracked segment: cnt >= 1
    }
    sum.out[i] = r;
}

// the changed list's records, eight lanes per 128-byte record
__global__ __launch_bounds__(256) void track_changed_gather_kernel(const TrackRecord *rec, const uint32_t *changed,
                                                                   const uint32_t *n_changed, uint32_t max_n,
                                                                   TrackRecord *out)
{
    const uint32_t g = (blockIdx.x * blockDim.x + threadIdx.x) >> 3, lane = threadIdx.x & 7u;
    const uint32_t nc = *n_changed;
    if (g >= (nc < max_n ? nc : max_n)) return;
    ((uint4 *)(out + g))[lane] = ((const uint4 *)(rec + changed[g]))[lane];
}

template <TrackKind K>
hipError_t launch_frame_summaries(hipStream_t st, const TrackArgs &a, const TrackStoreDev &d)
{
    const TrackSumDev &sum = *a.sum;
    const auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0u),
                                                     SumInput{a.skeys, a.svals, d.slot, a.fields, a.points});
    size_t tb = sum.temp_bytes;
    hipError_t e = rocprim::inclusive_scan(sum.temp, tb, in, sum.scan, (size_t)a.n, SumOp(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(track_frame_summary_kernel<K>, dim3((a.n + 255) / 256), dim3(256), 0, st, a.frames, a.fields,
                       (const adsb_track_point *)a.points, (const uint32_t *)a.skeys, (const uint32_t *)a.svals, a.n,
                       a.seconds_per_sample, a.sample_base, d, sum);
    return hipSuccess;
}

// ---- per-aircraft signal levels (table / bank with a levels reserve) -----------------------------------------------
// The scan's input at sorted position s, computed where the scan loads it: the frame's level record if the frame is
// counted (its aircraft tracked, the record valid), else nothing but the head mark.
struct LvlInput {
    const uint32_t *skeys, *svals, *slot;
    const adsb_frame_level *levels;
    __device__ __forceinline__ TrackLvlTuple operator()(uint32_t s) const
    {
        TrackLvlTuple v{};
        v.head = (s == 0 || skeys[s - 1] != skeys[s]) ? 1u : 0u;
        if (slot[s] != kTrackUntracked) {
            const adsb_frame_level l = levels[svals[s]];
            if (l.flags & ADSB_LEVEL_VALID) {
                v.signal = v.max_signal = l.signal_sum;
                v.noise = l.noise_sum;
                v.n = 1;
                v.peak = l.peak;
                v.weak = l.weak_bits;
                v.newest = s + 1u;
            }
        }
        return v;
    }
};

// Segmented: a right operand that holds a segment head starts over; otherwise saturating sums, maxima, and the later
// counted position (positions ascend, so the later one is the greater one).  Associative.
struct LvlOp {
    __device__ __forceinline__ TrackLvlTuple operator()(const TrackLvlTuple &l, const TrackLvlTuple &r) const
    {
        TrackLvlTuple o = r;
        if (!r.head) {
            o.head = l.head;
            o.signal = sat_add64(l.signal, r.signal);
            o.noise = sat_add64(l.noise, r.noise);
            o.max_signal = l.max_signal > r.max_signal ? l.max_signal : r.max_signal;
            o.n = sat_add32(l.n, r.n);
            o.peak = l.peak > r.peak ? l.peak : r.peak;
            o.weak = sat_add32(l.weak, r.weak);
            o.newest = l.newest > r.newest ? l.newest : r.newest;
        }
        return o;
    }
};

// One thread per segment tail with a counted frame: this update's part merged into the aircraft's level record
template <TrackKind K>
__global__ __launch_bounds__(256) void track_levels_merge_kernel(const adsb_frame *frames,
                                                                 const adsb_frame_level *levels, const uint32_t *skeys,
                                                                 const uint32_t *svals, uint32_t n,
                                                                 double seconds_per_sample, uint64_t sample_base,
                                                                 TrackStoreDev d, const TrackLvlTuple *scan)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = skeys[s];
    if (s + 1 != n && skeys[s + 1] == key) return;
    const uint32_t slot = d.slot[s];
    if (slot == kTrackUntracked) return;
    const TrackLvlTuple w = scan[s];
    if (!w.newest) return; // no counted frame: the record stays
    if (K == TrackKind::kBank) sample_base = d.sample_base[key >> 24];
    const uint32_t j = svals[w.newest - 1];
    const adsb_frame_level last = levels[j];
    adsb_aircraft_level a = d.lvl[slot - 1];
    a.signal_total = sat_add64(a.signal_total, w.signal);
    a.noise_total = sat_add64(a.noise_total, w.noise);
    a.last_signal_sum = last.signal_sum;
    a.last_noise_sum = last.noise_sum;
    a.max_signal_sum = a.max_signal_sum > w.max_signal ? a.max_signal_sum : w.max_signal;
    a.last_time = frame_time(frames, j, sample_base, seconds_per_sample);
    a.n_levels = sat_add32(a.n_levels, w.n);
    a.peak = a.peak > w.peak ? a.peak : w.peak;
    a.weak_bits_total = sat_add32(a.weak_bits_total, w.weak);
    a.reserved = 0;
    d.lvl[slot - 1] = a;
}

template <TrackKind K>
hipError_t launch_levels_merge(hipStream_t st, const TrackArgs &a, const TrackStoreDev &d)
{
    const TrackLvlDev &lv = *a.lvl;
    const auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0u),
                                                     LvlInput{a.skeys, a.svals, d.slot, a.levels});
    size_t tb = lv.temp_bytes;
    hipError_t e = rocprim::inclusive_scan(lv.temp, tb, in, lv.scan, (size_t)a.n, LvlOp(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(track_levels_merge_kernel<K>, dim3((a.n + 255) / 256), dim3(256), 0, st, a.frames, a.levels,
                       (const uint32_t *)a.skeys, (const uint32_t *)a.svals, a.n, a.seconds_per_sample, a.sample_base, d,
                       (const TrackLvlTuple *)lv.scan);
    return hipSuccess;
}

__global__ __launch_bounds__(256) void track_levels_clear_kernel(adsb_aircraft_level *lvl, uint64_t places)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < places) lvl[p] = empty_level();
}

// ---- positions from single messages (table / bank with a fixes reserve) --------------------------------------------
// One thread per sorted frame s, after the pairs kernel (which fixes a bank's d.slot): the frame's bytes decoded against
// its receiver's site (adsb_fix.h) into out / rem at the frame's LIST index.  A frame of an aircraft the table turned
// away gets its icao and nothing else, so the scan below counts nothing for it.
template <TrackKind K>
__global__ __launch_bounds__(256) void track_fix_decode_kernel(const adsb_frame *frames, const uint32_t *skeys,
                                                               const uint32_t *svals, uint32_t n, TrackStoreDev d,
                                                               TrackFixDev fx)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t i = svals[s]; // < n: a permutation of the list
    const uint32_t r = K == TrackKind::kBank ? skeys[s] >> 24 : 0u; // < n_receivers (track_bank_keys_kernel)
    adsb_frame_fix f;
    FixRem rem;
    fix_decode(d.site[r], frames[i].bytes, f, rem);
    if (d.slot[s] == kTrackUntracked) {
        const uint32_t icao = f.icao;
        f = adsb_frame_fix{};
        f.icao = icao;
        rem = FixRem{};
    }
    fx.out[i] = f;
    fx.rem[i] = rem;
}

// The scan's input at sorted position s, computed where the scan loads it from the frame's decoded flags
struct FixInput {
    const uint32_t *skeys, *svals;
    const adsb_frame_fix *out;
    __device__ __forceinline__ TrackFixTuple operator()(uint32_t s) const
    {
        const uint32_t flags = out[svals[s]].flags;
        TrackFixTuple v;
        v.head = (s == 0 || skeys[s - 1] != skeys[s]) ? 1u : 0u;
        v.newest = (flags & ADSB_FIX_VALID) ? s + 1u : 0u;
        v.n_ok = (flags & ADSB_FIX_VALID) ? 1u : 0u;
        v.n_rej = (flags & ADSB_FIX_REJECTED) ? 1u : 0u;
        return v;
    }
};

// Segmented: a right operand that holds a segment head starts over; otherwise saturating sums and the later accepted
// position (positions ascend, so the later one is the greater one).  Associative.
struct FixOp {
    __device__ __forceinline__ TrackFixTuple operator()(const TrackFixTuple &l, const TrackFixTuple &r) const
    {
        TrackFixTuple o = r;
        if (!r.head) {
            o.head = l.head;
            o.newest = l.newest > r.newest ? l.newest : r.newest;
            o.n_ok = sat_add32(l.n_ok, r.n_ok);
            o.n_rej = sat_add32(l.n_rej, r.n_rej);
        }
        return o;
    }
};

// One thread per segment tail with a position message: this update's part merged into the aircraft's fix
template <TrackKind K>
__global__ __launch_bounds__(256) void track_fix_merge_kernel(const adsb_frame *frames, const uint32_t *skeys,
                                                              const uint32_t *svals, uint32_t n,
                                                              double seconds_per_sample, uint64_t sample_base,
                                                              TrackStoreDev d, TrackFixDev fx)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = skeys[s];
    if (s + 1 != n && skeys[s + 1] == key) return;
    const uint32_t slot = d.slot[s];
    if (slot == kTrackUntracked) return;
    const TrackFixTuple w = fx.scan[s];
    if (!w.n_ok && !w.n_rej) return; // no position message: the fix stays
    if (K == TrackKind::kBank) sample_base = d.sample_base[key >> 24];
    FixWords words = ((const FixWords *)d.fix)[slot - 1];
    adsb_fix a;
    __builtin_memcpy(&a, &words, sizeof(a));
    if (w.newest) {
        const uint32_t j = svals[w.newest - 1];
        fix_take(a, fx.out[j], fx.rem[j], frame_time(frames, j, sample_base, seconds_per_sample));
    }
    a.n_fixes = sat_add32(a.n_fixes, w.n_ok);
    a.n_rejected = sat_add32(a.n_rejected, w.n_rej);
    __builtin_memcpy(&words, &a, sizeof(a));
    ((FixWords *)d.fix)[slot - 1] = words;
}

template <TrackKind K>
hipError_t launch_fix_merge(hipStream_t st, const TrackArgs &a, const TrackStoreDev &d)
{
    const TrackFixDev &fx = *a.fix;
    const dim3 grid((a.n + 255) / 256);
    hipLaunchKernelGGL(track_fix_decode_kernel<K>, grid, dim3(256), 0, st, a.frames, (const uint32_t *)a.skeys,
                       (const uint32_t *)a.svals, a.n, d, fx);
    const auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0u),
                                                     FixInput{a.skeys, a.svals, fx.out});
    size_t tb = fx.temp_bytes;
    hipError_t e = rocprim::inclusive_scan(fx.temp, tb, in, fx.scan, (size_t)a.n, FixOp(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(track_fix_merge_kernel<K>, grid, dim3(256), 0, st, a.frames, (const uint32_t *)a.skeys,
                       (const uint32_t *)a.svals, a.n, a.seconds_per_sample, a.sample_base, d, fx);
    return hipSuccess;
}

__global__ __launch_bounds__(256) void track_fixes_clear_kernel(FixWords *fix, uint64_t places)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < places) fix[p] = fix_empty();
}

// ---- multilaterated positions per aircraft (table with an mlat reserve) ----------------------------------------------
// One thread per sorted frame s, after the pairs kernel: the frame's bytes and its fix (both at the frame's LIST index
// i = svals[s] < n, a permutation of the list) through adsb_track_mlat.h into out[i], and the scan's operand into in[s].
// A frame of an aircraft the table turned away gets its icao and nothing else, and counts nowhere.
template <TrackKind K>
__global__ __launch_bounds__(256) void track_mlat_frame_kernel(const adsb_frame *frames, const adsb_mlat_fix *fixes,
                                                               const uint32_t *skeys, const uint32_t *svals, uint32_t n,
                                                               TrackStoreDev d, TrackMlatDev ml)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = skeys[s], i = svals[s];
    MlatFrame m{};
    if (d.slot[s] != kTrackUntracked) m = mlat_frame(ml.max_disagreement_m, frames[i].bytes, fixes[i]);
    adsb_frame_mlat f;
    f.disagreement_m = m.disagreement_m;
    f.icao = K == TrackKind::kBank ? key & 0xFFFFFFu : key;
    f.flags = m.flags;
    f.reserved = 0;
    ml.out[i] = f;
    const bool valid = (m.flags & ADSB_TRACK_MLAT_VALID) != 0, checked = (m.flags & ADSB_TRACK_MLAT_CHECKED) != 0;
    TrackMlatTuple v;
    v.head = (s == 0 || skeys[s - 1] != key) ? 1u : 0u;
    v.newest_valid = valid ? s + 1u : 0u;
    v.newest_checked = checked ? s + 1u : 0u;
    v.max_m = m.disagreement_m;
    v.n_attempted = m.attempted;
    v.n_valid = valid ? 1u : 0u;
    v.n_checked = checked ? 1u : 0u;
    v.n_disagree = (m.flags & ADSB_TRACK_MLAT_DISAGREE) ? 1u : 0u;
    ml.in[s] = v;
}

// Segmented: a right operand that holds a segment head starts over; otherwise saturating sums, the float maximum (of
// values that are >= 0 and never NaN) and the later positions (positions ascend, so the later one is the greater one).
// Associative.
struct MlatOp {
    __device__ __forceinline__ TrackMlatTuple operator()(const TrackMlatTuple &l, const TrackMlatTuple &r) const
    {
        TrackMlatTuple o = r;
        if (!r.head) {
            o.head = l.head;
            o.newest_valid = l.newest_valid > r.newest_valid ? l.newest_valid : r.newest_valid;
            o.newest_checked = l.newest_checked > r.newest_checked ? l.newest_checked : r.newest_checked;
            o.max_m = l.max_m > r.max_m ? l.max_m : r.max_m;
            o.n_attempted = sat_add32(l.n_attempted, r.n_attempted);
            o.n_valid = sat_add32(l.n_valid, r.n_valid);
            o.n_checked = sat_add32(l.n_checked, r.n_checked);
            o.n_disagree = sat_add32(l.n_disagree, r.n_disagree);
        }
        return o;
    }
};

// One thread per segment tail whose segment adds something: this update's part merged into the aircraft's mlat record
template <TrackKind K>
__global__ __launch_bounds__(256) void track_mlat_merge_kernel(const adsb_frame *frames, const adsb_mlat_fix *fixes,
                                                               const uint32_t *skeys, const uint32_t *svals, uint32_t n,
                                                               double seconds_per_sample, uint64_t sample_base,
                                                               TrackStoreDev d, TrackMlatDev ml)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = skeys[s];
    if (s + 1 != n && skeys[s + 1] == key) return;
    const uint32_t slot = d.slot[s];
    if (slot == kTrackUntracked) return;
    const TrackMlatTuple w = ml.scan[s];
    if (!w.n_attempted && !w.n_valid) return; // nothing counted (checked implies valid): the record stays
    if (K == TrackKind::kBank) sample_base = d.sample_base[key >> 24];
    MlatWords words = ((const MlatWords *)d.mlat)[slot - 1];
    adsb_aircraft_mlat a;
    __builtin_memcpy(&a, &words, sizeof(a));
    if (w.newest_checked) { // <= n: a sorted position + 1 of this list
        a.last_disagreement_m = ml.out[svals[w.newest_checked - 1]].disagreement_m;
        a.flags |= ADSB_TRACK_MLAT_CHECKED;
    }
    if (w.newest_valid) {
        const uint32_t j = svals[w.newest_valid - 1];
        mlat_take(a, fixes[j], frame_time(frames, j, sample_base, seconds_per_sample));
    }
    a.max_disagreement_m = a.max_disagreement_m > w.max_m ? a.max_disagreement_m : w.max_m;
    a.n_attempted = sat_add32(a.n_attempted, w.n_attempted);
    a.n_valid = sat_add32(a.n_valid, w.n_valid);
    a.n_checked = sat_add32(a.n_checked, w.n_checked);
    a.n_disagree = sat_add32(a.n_disagree, w.n_disagree);
    __builtin_memcpy(&words, &a, sizeof(a));
    ((MlatWords *)d.mlat)[slot - 1] = words;
}

template <TrackKind K>
hipError_t launch_mlat_merge(hipStream_t st, const TrackArgs &a, const TrackStoreDev &d)
{
    const TrackMlatDev &ml = *a.mlat;
    const dim3 grid((a.n + 255) / 256);
    hipLaunchKernelGGL(track_mlat_frame_kernel<K>, grid, dim3(256), 0, st, a.frames, a.mlat_fixes,
                       (const uint32_t *)a.skeys, (const uint32_t *)a.svals, a.n, d, ml);
    size_t tb = ml.temp_bytes;
    hipError_t e = rocprim::inclusive_scan(ml.temp, tb, (const TrackMlatTuple *)ml.in, ml.scan, (size_t)a.n, MlatOp(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(track_mlat_merge_kernel<K>, grid, dim3(256), 0, st, a.frames, a.mlat_fixes,
                       (const uint32_t *)a.skeys, (const uint32_t *)a.svals, a.n, a.seconds_per_sample, a.sample_base, d,
                       ml);
    return hipSuccess;
}

__global__ __launch_bounds__(256) void track_mlat_clear_kernel(MlatWords *mlat, uint64_t places)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < places) mlat[p] = mlat_empty();
}

// ---- filtered mlat track per aircraft (table with a filter reserve) --------------------------------------------------
// One thread per sorted frame s: the operand of frame i = svals[s] at s, so that the walk reads consecutive records, and
// the 32 zero bytes of a frame that is not usable at out[i] (the walk writes the usable ones).  sin, cos and the root of
// the whole feature are here.
template <TrackKind K>
__global__ __launch_bounds__(256) void track_filter_operand_kernel(const adsb_frame *frames, const adsb_mlat_fix *fixes,
                                                                   const uint32_t *skeys, const uint32_t *svals,
                                                                   uint32_t n, double seconds_per_sample,
                                                                   uint64_t sample_base, TrackStoreDev d,
                                                                   TrackFilterDev fl)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t i = svals[s];
    if (K == TrackKind::kBank) sample_base = d.sample_base[skeys[s] >> 24];
    const adsb_filter_operand o = filter_operand(fl.cfg, fixes[i], frame_time(frames, i, sample_base, seconds_per_sample),
                                                 d.slot[s] != kTrackUntracked);
    fl.op[s] = o;
    if (!(o.flags & ADSB_TRACK_FILTER_USABLE)) fl.out[i] = adsb_frame_filter{};
}

// One thread per segment HEAD: the aircraft's record through filter_step, frame after frame in list order, one
// adsb_frame_filter per usable frame at the frame's list index, the record stored once.  A wave takes as long as the
// longest segment that begins in it, and its other lanes idle meanwhile.  Workgroups are ONE wave: waves share nothing,
// a long segment holds up no more than the heads among its own 64 frames, and the waves spread over every CU.  Measured
// against a build with 256-thread workgroups (profiles/track_filter_timing.txt): 15-23 us faster on
// 32 768 frames of 2 048 aircraft, 3-8 % slower on 32 768 frames of one.  The record (48 registers) and two operands (16
// each) stay in registers; a step is some sixty dependent f64 operations, ten of them divisions, and needs three loads
// (the next key, the 64-byte operand, its list index) whose addresses do not depend on the step before: frame j + 1's
// are issued BEFORE frame j's step, so their latency lies under its arithmetic (13 % off the one-aircraft list).  The
// next operand is read whoever it belongs to; the last frame of the list reads itself again, so no index passes n - 1.
#ifndef ADSB_FILTER_WALK_BLOCK
#define ADSB_FILTER_WALK_BLOCK 64 // the 256-thread build of that measurement sets it
#endif
constexpr uint32_t kFilterWalkBlock = ADSB_FILTER_WALK_BLOCK;
template <TrackKind K>
__global__ __launch_bounds__(kFilterWalkBlock) void track_filter_walk_kernel(const uint32_t *skeys, const uint32_t *svals,
                                                                             uint32_t n, TrackStoreDev d,
                                                                             TrackFilterDev fl)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = skeys[s];
    if (s != 0 && skeys[s - 1] == key) return; // not a head
    const uint32_t slot = d.slot[s];
    if (slot == kTrackUntracked) return; // none of its frames is usable: the operand kernel wrote their outputs
    FilterWords words = ((const FilterWords *)d.filter)[slot - 1];
    adsb_aircraft_filter a;
    __builtin_memcpy(&a, &words, sizeof(a));
    bool touched = false;
    adsb_filter_operand o = fl.op[s];
    uint32_t i = svals[s];
    for (uint32_t j = s;;) {
        const uint32_t jn = j + 1, jc = jn < n ? jn : j; // the last frame of the list reads itself again: no branch
        const uint32_t key_n = skeys[jc], i_n = svals[jc];
        const adsb_filter_operand o_n = fl.op[jc];
        if (o.flags & ADSB_TRACK_FILTER_USABLE) {
            adsb_frame_filter f;
            filter_step(fl.cfg, a, o, f);
            fl.out[i] = f;
            touched = true;
        }
        if (jn >= n || key_n != key) break;
        o = o_n;
        i = i_n;
        j = jn;
    }
    if (!touched) return;
    for (int k = 0; k < 8; ++k) a.reserved[k] = 0; // what it was: written as constants, the array stays out of memory
    __builtin_memcpy(&words, &a, sizeof(a));
    ((FilterWords *)d.filter)[slot - 1] = words;
}

template <TrackKind K>
hipError_t launch_filter(hipStream_t st, const TrackArgs &a, const TrackStoreDev &d)
{
    const TrackFilterDev &fl = *a.filter;
    hipLaunchKernelGGL(track_filter_operand_kernel<K>, dim3((a.n + 255) / 256), dim3(256), 0, st, a.frames, a.mlat_fixes,
                       (const uint32_t *)a.skeys, (const uint32_t *)a.svals, a.n, a.seconds_per_sample, a.sample_base, d,
                       fl);
    hipLaunchKernelGGL(track_filter_walk_kernel<K>, dim3((a.n + kFilterWalkBlock - 1) / kFilterWalkBlock),
                       dim3(kFilterWalkBlock), 0, st, (const uint32_t *)a.skeys, (const uint32_t *)a.svals, a.n, d, fl);
    return hipSuccess;
}

__global__ __launch_bounds__(256) void track_filter_clear_kernel(FilterWords *filter, uint64_t places)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < places) filter[p] = filter_empty();
}

// ---- Mode S replies per aircraft (table with a modes reserve) --------------------------------------------------------
// update_modes' key kernel, in place of track_keys_kernel: one thread per frame i < n.  The key is the record's address
// (< 2^24) for an accepted frame and kModesNoAddress for every other; fields[i] gets that address, and unless the frame
// is an accepted DF17/18 it becomes a frame of kind "other" (the field decode reads bytes[4] >> 3 of any frame as a type
// code).
__global__ __launch_bounds__(256) void track_modes_keys_kernel(adsb_packet_fields *fields, const adsb_modes_rec *recs,
                                                               uint32_t n, uint32_t *keys, uint32_t *vals)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const adsb_modes_rec r = recs[i];
    const bool accepted = modes_accepted(r);
    const uint32_t address = r.address & 0xFFFFFFu;
    fields[i].icao = address;
    if (!accepted || !modes_squitter(r.df)) {
        fields[i].msg_kind = 2;
        fields[i].msg_type = 0;
    }
    keys[i] = accepted ? address : kModesNoAddress;
    vals[i] = i;
}

// update_modes' lookup, in place of track_lookup_kernel: the same, but the segment of kModesNoAddress is no aircraft
// (index has 2^24 words and is not read there): no slot, never new
__global__ __launch_bounds__(256) void track_modes_lookup_kernel(const uint32_t *skeys, uint32_t n, const uint32_t *index,
                                                                 uint32_t *slot, uint32_t *is_new)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = skeys[s]; // <= 2^24: track_modes_keys_kernel
    if (key >= kModesNoAddress) {
        slot[s] = kTrackUntracked;
        is_new[s] = 0;
        return;
    }
    const uint32_t idx = index[key];
    slot[s] = idx;
    is_new[s] = (idx == 0 && (s == 0 || skeys[s - 1] != key)) ? 1u : 0u;
}

// One thread per sorted frame s, after the pairs kernel and the other per-frame kernels of this update (svals[s] < n, a
// permutation of the list).  A frame that is not accepted: the kernels before wrote what they write for an aircraft the
// table turned away, with the sentinel as icao; here its point becomes UNADDRESSED and every per-frame icao the
// record's address.  An accepted frame that is no squitter: its frame fix carries the address, not bytes[1..3].  Then
// the scan's operand: adsb_track_modes.h's contribution of a counted frame, nothing but the head mark otherwise.
__global__ __launch_bounds__(256) void track_modes_frame_kernel(const adsb_modes_rec *recs, const uint32_t *skeys,
                                                                const uint32_t *svals, uint32_t n, TrackStoreDev d,
                                                                adsb_track_point *points, adsb_aircraft_record *sum_out,
                                                                adsb_frame_fix *fix_out, adsb_frame_mlat *mlat_out,
                                                                TrackModesTuple *in)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = skeys[s], i = svals[s];
    const adsb_modes_rec r = recs[i];
    TrackModesTuple v{};
    v.head = (s == 0 || skeys[s - 1] != key) ? 1u : 0u;
    if (key >= kModesNoAddress) {
        adsb_track_point pt;
        pt.latitude = 0.0;
        pt.longitude = 0.0;
        pt.icao = r.address;
        pt.flags = ADSB_TRACK_UNADDRESSED;
        points[i] = pt;
        if (sum_out) sum_out[i].icao = r.address;
        if (fix_out) fix_out[i].icao = r.address;
        if (mlat_out) mlat_out[i].icao = r.address;
        in[s] = v;
        return;
    }
    if (fix_out && !modes_squitter(r.df)) fix_out[i].icao = key;
    if (d.slot[s] != kTrackUntracked) {
        const uint32_t w = modes_what(r), at = s + 1u;
        v.squitter = (w & kModesSquitter) ? 1u : 0u;
        v.alt = (w & kModesAlt) ? at : 0u;
        v.squawk = (w & kModesSquawk) ? at : 0u;
        v.callsign = (w & kModesCallsign) ? at : 0u;
        v.status = (w & kModesStatus) ? at : 0u;
        v.ground = (w & kModesGround) ? at : 0u;
        v.any = at;
        v.n_replies = (w & kModesReply) ? 1u : 0u;
        v.n_allcall = (w & kModesAllcall) ? 1u : 0u;
        v.n_surveillance = (w & kModesSurveillance) ? 1u : 0u;
        v.n_airair = (w & kModesAirAir) ? 1u : 0u;
    }
    in[s] = v;
}

// Segmented: a right operand that holds a segment head starts over; otherwise OR, the later positions (positions ascend,
// so the later one is the greater one) and saturating sums.  Associative.
struct ModesOp {
    __device__ __forceinline__ TrackModesTuple operator()(const TrackModesTuple &l, const TrackModesTuple &r) const
    {
        TrackModesTuple o = r;
        if (!r.head) {
            o.head = l.head;
            o.squitter = l.squitter | r.squitter;
            o.alt = l.alt > r.alt ? l.alt : r.alt;
            o.squawk = l.squawk > r.squawk ? l.squawk : r.squawk;
            o.callsign = l.callsign > r.callsign ? l.callsign : r.callsign;
            o.status = l.status > r.status ? l.status : r.status;
            o.ground = l.ground > r.ground ? l.ground : r.ground;
            o.any = l.any > r.any ? l.any : r.any;
            o.n_replies = sat_add32(l.n_replies, r.n_replies);
            o.n_allcall = sat_add32(l.n_allcall, r.n_allcall);
            o.n_surveillance = sat_add32(l.n_surveillance, r.n_surveillance);
            o.n_airair = sat_add32(l.n_airair, r.n_airair);
        }
        return o;
    }
};

// One thread per segment tail with a counted frame: the segment's part (adsb_track_modes.h) from the winning frames'
// records and times, merged into the aircraft's modes record.  Every position is <= n: a sorted position + 1 of this list.
__global__ __launch_bounds__(256) void track_modes_merge_kernel(const adsb_frame *frames, const adsb_modes_rec *recs,
                                                                const uint32_t *skeys, const uint32_t *svals, uint32_t n,
                                                                double seconds_per_sample, uint64_t sample_base,
                                                                TrackStoreDev d, const TrackModesTuple *scan)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = skeys[s];
    if (s + 1 != n && skeys[s + 1] == key) return;
    const uint32_t slot = d.slot[s];
    if (slot == kTrackUntracked) return; // turned away, or the segment of the frames that are not accepted
    const TrackModesTuple w = scan[s];
    if (!w.any) return; // nothing counted: the record stays
    // the winning frames' records where they lie (null: the segment has no such frame), and the three times
    const adsb_modes_rec *r_alt = w.alt ? recs + svals[w.alt - 1] : nullptr;
    const adsb_modes_rec *r_squawk = w.squawk ? recs + svals[w.squawk - 1] : nullptr;
    const adsb_modes_rec *r_callsign = w.callsign ? recs + svals[w.callsign - 1] : nullptr;
    const adsb_modes_rec *r_status = w.status ? recs + svals[w.status - 1] : nullptr;
    const adsb_modes_rec *r_ground = w.ground ? recs + svals[w.ground - 1] : nullptr;
    const double t_alt = w.alt ? frame_time(frames, svals[w.alt - 1], sample_base, seconds_per_sample) : 0.0;
    const double t_squawk = w.squawk ? frame_time(frames, svals[w.squawk - 1], sample_base, seconds_per_sample) : 0.0;
    const double t_callsign = w.callsign ? frame_time(frames, svals[w.callsign - 1], sample_base, seconds_per_sample) : 0.0;
    ModesCounts c;
    c.n_replies = w.n_replies;
    c.n_allcall = w.n_allcall;
    c.n_surveillance = w.n_surveillance;
    c.n_airair = w.n_airair;
    c.squitter = w.squitter;
    const adsb_aircraft_modes part = modes_part(c, recs + svals[w.any - 1], r_alt, t_alt, r_squawk, t_squawk, r_callsign,
                                                t_callsign, r_status, r_ground);
    ModesWords words = ((const ModesWords *)d.modes)[slot - 1];
    adsb_aircraft_modes a;
    __builtin_memcpy(&a, &words, sizeof(a));
    modes_merge(a, part);
    __builtin_memcpy(&words, &a, sizeof(a));
    ((ModesWords *)d.modes)[slot - 1] = words;
}

hipError_t launch_modes_merge(hipStream_t st, const TrackArgs &a, const TrackStoreDev &d)
{
    const TrackModesDev &mo = *a.modes;
    const dim3 grid((a.n + 255) / 256);
    hipLaunchKernelGGL(track_modes_frame_kernel, grid, dim3(256), 0, st, a.modes_recs, (const uint32_t *)a.skeys,
                       (const uint32_t *)a.svals, a.n, d, a.points, a.sum ? a.sum->out : nullptr,
                       (a.fix && d.fix) ? a.fix->out : nullptr, (a.mlat && d.mlat) ? a.mlat->out : nullptr, mo.in);
    size_t tb = mo.temp_bytes;
    hipError_t e = rocprim::inclusive_scan(mo.temp, tb, (const TrackModesTuple *)mo.in, mo.scan, (size_t)a.n, ModesOp(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(track_modes_merge_kernel, grid, dim3(256), 0, st, a.frames, a.modes_recs,
                       (const uint32_t *)a.skeys, (const uint32_t *)a.svals, a.n, a.seconds_per_sample, a.sample_base, d,
                       (const TrackModesTuple *)mo.scan);
    return hipSuccess;
}

__global__ __launch_bounds__(256) void track_modes_clear_kernel(ModesWords *modes, uint64_t places)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < places) modes[p] = modes_empty();
}

// ---- Comm-B registers per aircraft (table with a modes and a commb reserve) ------------------------------------------
// The first scan's input at sorted position s, computed where the scan loads it: s + 1 if the frame is an airborne-
// velocity message by the merge's own test (track_summary_kernel: type code 19 of a frame the key kernel left a
// squitter, ST 1-4), of an accepted frame
struct CommbRefInput {
    const uint32_t *skeys, *svals;
    const adsb_packet_fields *fields;
    const adsb_frame *frames;
    __device__ __forceinline__ TrackCommbRefTuple operator()(uint32_t s) const
    {
        TrackCommbRefTuple v;
        const uint32_t key = skeys[s], j = svals[s];
        v.head = (s == 0 || skeys[s - 1] != key) ? 1u : 0u;
        v.vel = 0u;
        if (key < kModesNoAddress && fields[j].msg_type == 19) {
            const uint32_t st = frames[j].bytes[4] & 7u;
            if (st >= 1 && st <= 4) v.vel = s + 1u;
        }
        return v;
    }
};

struct CommbRefOp {
    __device__ __forceinline__ TrackCommbRefTuple operator()(const TrackCommbRefTuple &l, const TrackCommbRefTuple &r) const
    {
        TrackCommbRefTuple o = r;
        if (!r.head) {
            o.head = l.head;
            o.vel = l.vel > r.vel ? l.vel : r.vel;
        }
        return o;
    }
};

// One thread per sorted frame s (svals[s] < n, a permutation of the list; d.slot[s] - 1 < max_aircraft unless
// kTrackUntracked; ref[s - 1].vel - 1 < s is a sorted position of the same segment).  Runs before track_summary_kernel:
// d.rec[slot - 1].vel is the velocity held from before this update (admission emptied a new aircraft's).
__global__ __launch_bounds__(256) void track_commb_frame_kernel(const adsb_frame *frames, const adsb_commb_rec *commb,
                                                                const uint32_t *skeys, const uint32_t *svals, uint32_t n,
                                                                double seconds_per_sample, uint64_t sample_base,
                                                                TrackStoreDev d, const TrackCommbRefTuple *ref,
                                                                adsb_commb_settle_cfg cfg, adsb_commb_rec *out,
                                                                TrackCommbTuple *in)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = skeys[s], i = svals[s];
    adsb_commb_rec o = commb[i];
    TrackCommbTuple v{};
    v.head = (s == 0 || skeys[s - 1] != key) ? 1u : 0u;
    const uint32_t slot = d.slot[s];
    if (key < kModesNoAddress && slot != kTrackUntracked && o.state != ADSB_COMMB_NOT_COMMB) { // counted
        if (commb_can_settle(o)) {
            const uint32_t p = v.head ? 0u : ref[s - 1].vel;
            CommbRef r;
            if (p) {
                const uint32_t j = svals[p - 1];
                r = commb_ref_of_frame(modes_bytes(frames[j].bytes), frame_time(frames, j, sample_base, seconds_per_sample));
            } else {
                r = commb_ref_of_velocity(d.rec[slot - 1].vel);
            }
            o = commb_settle(modes_bytes(frames[i].bytes), o, r, frame_time(frames, i, sample_base, seconds_per_sample), cfg);
        }
        const uint32_t sort = commb_sort_of(o), at = s + 1u;
        v.newest[0] = sort == kCommbSort40 ? at : 0u;
        v.newest[1] = sort == kCommbSort50 ? at : 0u;
        v.newest[2] = sort == kCommbSort60 ? at : 0u;
        v.newest[3] = sort == kCommbSort17 ? at : 0u;
        v.newest[4] = sort == kCommbSort30 ? at : 0u;
        const CommbCounts c = commb_counts_of(o);
        v.n_commb = c.n_commb;
        v.n_settled = c.n_settled;
        v.n_ambiguous = c.n_ambiguous;
        v.n_none = c.n_none;
    }
    out[i] = o;
    in[s] = v;
}

struct CommbOp {
    __device__ __forceinline__ TrackCommbTuple operator()(const TrackCommbTuple &l, const TrackCommbTuple &r) const
    {
        TrackCommbTuple o = r;
        if (!r.head) {
            o.head = l.head;
            o.newest[0] = l.newest[0] > r.newest[0] ? l.newest[0] : r.newest[0];
            o.newest[1] = l.newest[1] > r.newest[1] ? l.newest[1] : r.newest[1];
            o.newest[2] = l.newest[2] > r.newest[2] ? l.newest[2] : r.newest[2];
            o.newest[3] = l.newest[3] > r.newest[3] ? l.newest[3] : r.newest[3];
            o.newest[4] = l.newest[4] > r.newest[4] ? l.newest[4] : r.newest[4];
            o.n_commb = sat_add32(l.n_commb, r.n_commb);
            o.n_settled = sat_add32(l.n_settled, r.n_settled);
            o.n_ambiguous = sat_add32(l.n_ambiguous, r.n_ambiguous);
            o.n_none = sat_add32(l.n_none, r.n_none);
        }
        return o;
    }
};

// One thread per segment tail with a counted frame: the segment's part (adsb_track_commb.h) from the winning frames'
// per-frame outputs and times, merged into the aircraft's commb record.  Every position is <= n: a sorted position + 1.
__global__ __launch_bounds__(256) void track_commb_merge_kernel(const adsb_frame *frames, const adsb_commb_rec *out,
                                                                const uint32_t *skeys, const uint32_t *svals, uint32_t n,
                                                                double seconds_per_sample, uint64_t sample_base,
                                                                TrackStoreDev d, const TrackCommbTuple *scan)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = skeys[s];
    if (s + 1 != n && skeys[s + 1] == key) return;
    const uint32_t slot = d.slot[s];
    if (key >= kModesNoAddress || slot == kTrackUntracked) return;
    const TrackCommbTuple w = scan[s];
    if (!w.n_commb) return; // nothing counted: the record stays
    const uint32_t p40 = w.newest[0], p50 = w.newest[1], p60 = w.newest[2], p17 = w.newest[3], p30 = w.newest[4];
    const uint32_t i40 = p40 ? svals[p40 - 1] : 0u, i50 = p50 ? svals[p50 - 1] : 0u, i60 = p60 ? svals[p60 - 1] : 0u,
                   i30 = p30 ? svals[p30 - 1] : 0u;
    CommbCounts c;
    c.n_commb = w.n_commb;
    c.n_settled = w.n_settled;
    c.n_ambiguous = w.n_ambiguous;
    c.n_none = w.n_none;
    const adsb_aircraft_commb part =
        commb_part(c, p40 ? out + i40 : nullptr, p40 ? frame_time(frames, i40, sample_base, seconds_per_sample) : 0.0,
                   p50 ? out + i50 : nullptr, p50 ? frame_time(frames, i50, sample_base, seconds_per_sample) : 0.0,
                   p60 ? out + i60 : nullptr, p60 ? frame_time(frames, i60, sample_base, seconds_per_sample) : 0.0,
                   p17 ? out + svals[p17 - 1] : nullptr, p30 ? out + i30 : nullptr,
                   p30 ? frame_time(frames, i30, sample_base, seconds_per_sample) : 0.0);
    CommbWords words = ((const CommbWords *)d.commb)[slot - 1];
    adsb_aircraft_commb a;
    __builtin_memcpy(&a, &words, sizeof(a));
    commb_merge(a, part);
    __builtin_memcpy(&words, &a, sizeof(a));
    ((CommbWords *)d.commb)[slot - 1] = words;
}

hipError_t launch_commb_merge(hipStream_t st, const TrackArgs &a, const TrackStoreDev &d)
{
    const TrackCommbDev &cb = *a.commb;
    const dim3 grid((a.n + 255) / 256);
    const auto in = rocprim::make_transform_iterator(
        rocprim::counting_iterator<uint32_t>(0u),
        CommbRefInput{(const uint32_t *)a.skeys, (const uint32_t *)a.svals, a.fields, a.frames});
    size_t tb = cb.temp_bytes;
    hipError_t e = rocprim::inclusive_scan(cb.temp, tb, in, cb.ref, (size_t)a.n, CommbRefOp(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(track_commb_frame_kernel, grid, dim3(256), 0, st, a.frames, a.commb_recs, (const uint32_t *)a.skeys,
                       (const uint32_t *)a.svals, a.n, a.seconds_per_sample, a.sample_base, d,
                       (const TrackCommbRefTuple *)cb.ref, cb.cfg, cb.out, cb.in);
    tb = cb.temp_bytes;
    e = rocprim::inclusive_scan(cb.temp, tb, (const TrackCommbTuple *)cb.in, cb.scan, (size_t)a.n, CommbOp(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(track_commb_merge_kernel, grid, dim3(256), 0, st, a.frames, (const adsb_commb_rec *)cb.out,
                       (const uint32_t *)a.skeys, (const uint32_t *)a.svals, a.n, a.seconds_per_sample, a.sample_base, d,
                       (const TrackCommbTuple *)cb.scan);
    return hipSuccess;
}

__global__ __launch_bounds__(256) void track_commb_clear_kernel(CommbWords *commb, uint64_t places)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < places) commb[p] = commb_empty();
}

// ---- Extended squitter status per aircraft (table with an es reserve) -------------------------------------------------
// The first scan's input at sorted position s, computed where the scan loads it: s + 1 in each word whose present bit
// the frame's es record has.  A frame that has one of them is an extended squitter (never NOT_ES or FOREIGN), and key
// and slot are its whole segment's, so within a counted segment these are exactly the counted frames.
struct EsRefInput {
    const uint32_t *skeys, *svals;
    const adsb_es_rec *es;
    __device__ __forceinline__ TrackEsRefTuple operator()(uint32_t s) const
    {
        TrackEsRefTuple v;
        const uint32_t present = es_track_counted(es[svals[s]]) ? es[svals[s]].present : 0u;
        v.head = (s == 0 || skeys[s - 1] != skeys[s]) ? 1u : 0u;
        v.version = (present & ADSB_ES_HAS_VERSION) ? s + 1u : 0u;
        v.a = (present & ADSB_ES_HAS_NIC_A) ? s + 1u : 0u;
        v.c = (present & ADSB_ES_HAS_NIC_C) ? s + 1u : 0u;
        return v;
    }
};

struct EsRefOp {
    __device__ __forceinline__ TrackEsRefTuple operator()(const TrackEsRefTuple &l, const TrackEsRefTuple &r) const
    {
        TrackEsRefTuple o = r;
        if (!r.head) {
            o.head = l.head;
            o.version = l.version > r.version ? l.version : r.version;
            o.a = l.a > r.a ? l.a : r.a;
            o.c = l.c > r.c ? l.c : r.c;
        }
        return o;
    }
};

// One thread per sorted frame s (svals[s] < n, a permutation of the list; d.slot[s] - 1 < max_aircraft unless
// kTrackUntracked; ref[s - 1]'s words - 1 < s are sorted positions of the same segment).  d.es[slot - 1] is the record
// from before this update: the merge kernel below is the only writer and runs after the second scan.
__global__ __launch_bounds__(256) void track_es_frame_kernel(const adsb_frame *frames, const adsb_es_rec *es,
                                                             const uint32_t *skeys, const uint32_t *svals, uint32_t n,
                                                             double seconds_per_sample, uint64_t sample_base,
                                                             TrackStoreDev d, const TrackEsRefTuple *ref, double max_age_s,
                                                             adsb_frame_integrity *out, TrackEsTuple *in)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = skeys[s], i = svals[s];
    const adsb_es_rec r = es[i];
    TrackEsTuple v{};
    adsb_frame_integrity o{};
    v.head = (s == 0 || skeys[s - 1] != key) ? 1u : 0u;
    const uint32_t slot = d.slot[s];
    if (key < kModesNoAddress && slot != kTrackUntracked && es_track_counted(r)) {
        TrackEsRefTuple p{};
        if (!v.head) p = ref[s - 1];
        const adsb_aircraft_es *held = d.es + (slot - 1);
        EsKnown k;
        if (p.version) {
            const uint32_t j = svals[p.version - 1];
            k.version = es[j].version;
            k.version_time = frame_time(frames, j, sample_base, seconds_per_sample);
        } else {
            k.version = held->version;
            k.version_time = held->version_time;
        }
        if (p.a) {
            const uint32_t j = svals[p.a - 1];
            k.a = es[j].nic_a;
            k.a_time = frame_time(frames, j, sample_base, seconds_per_sample);
        } else {
            k.a = held->nic_a;
            k.a_time = held->nic_a_time;
        }
        if (p.c) {
            const uint32_t j = svals[p.c - 1];
            k.c = es[j].nic_c;
            k.c_time = frame_time(frames, j, sample_base, seconds_per_sample);
        } else {
            k.c = held->nic_c;
            k.c_time = held->nic_c_time;
        }
        o = es_track_resolve(r, frame_time(frames, i, sample_base, seconds_per_sample), k, max_age_s);
        const uint32_t m = es_track_writes(r), at = s + 1u;
#pragma unroll
        for (uint32_t g = 0; g < kEsTrackGroups; ++g) v.newest[g] = ((m >> g) & 1u) ? at : 0u;
        v.n_es = 1u;
        v.n_position = (m >> kEsTrackPosition) & 1u;
    }
    out[i] = o;
    in[s] = v;
}

struct EsOp {
    __device__ __forceinline__ TrackEsTuple operator()(const TrackEsTuple &l, const TrackEsTuple &r) const
    {
        TrackEsTuple o = r;
        if (!r.head) {
            o.head = l.head;
#pragma unroll
            for (uint32_t g = 0; g < kEsTrackGroups; ++g) o.newest[g] = l.newest[g] > r.newest[g] ? l.newest[g] : r.newest[g];
            o.n_es = sat_add32(l.n_es, r.n_es);
            o.n_position = sat_add32(l.n_position, r.n_position);
        }
        return o;
    }
};

// group G of the part from the segment's winner at sorted position p - 1 (p = 0: the segment has none)
template <uint32_t G>
__device__ __forceinline__ void es_part_take(adsb_aircraft_es &part, uint32_t p, const adsb_frame *frames,
                                             const adsb_es_rec *es, const adsb_frame_integrity *out,
                                             const uint32_t *svals, double seconds_per_sample, uint64_t sample_base)
{
    if (!p) return;
    const uint32_t j = svals[p - 1];
    adsb_frame_integrity f{};
    if (G == kEsTrackPosition) f = out[j];
    es_track_set(part, G, es[j], f, frame_time(frames, j, sample_base, seconds_per_sample));
}

// One thread per segment tail with a counted frame: the segment's part (adsb_track_es.h) from the winning frames' es
// records, per-frame outputs and times, merged into the aircraft's es record.  Every position is <= n: a sorted
// position + 1.
__global__ __launch_bounds__(256) void track_es_merge_kernel(const adsb_frame *frames, const adsb_es_rec *es,
                                                             const adsb_frame_integrity *out, const uint32_t *skeys,
                                                             const uint32_t *svals, uint32_t n, double seconds_per_sample,
                                                             uint64_t sample_base, TrackStoreDev d, const TrackEsTuple *scan)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t key = skeys[s];
    if (s + 1 != n && skeys[s + 1] == key) return;
    const uint32_t slot = d.slot[s];
    if (key >= kModesNoAddress || slot == kTrackUntracked) return;
    const TrackEsTuple w = scan[s];
    if (!w.n_es) return; // nothing counted: the record stays
    adsb_aircraft_es part = es_track_empty_record();
    part.n_es = w.n_es;
    part.n_position = w.n_position;
    es_part_take<kEsTrackOpAir>(part, w.newest[0], frames, es, out, svals, seconds_per_sample, sample_base);
    es_part_take<kEsTrackOpSurface>(part, w.newest[1], frames, es, out, svals, seconds_per_sample, sample_base);
    es_part_take<kEsTrackTargetState>(part, w.newest[2], frames, es, out, svals, seconds_per_sample, sample_base);
    es_part_take<kEsTrackEmergency>(part, w.newest[3], frames, es, out, svals, seconds_per_sample, sample_base);
    es_part_take<kEsTrackAcasRa>(part, w.newest[4], frames, es, out, svals, seconds_per_sample, sample_base);
    es_part_take<kEsTrackVersion>(part, w.newest[5], frames, es, out, svals, seconds_per_sample, sample_base);
    es_part_take<kEsTrackNicA>(part, w.newest[6], frames, es, out, svals, seconds_per_sample, sample_base);
    es_part_take<kEsTrackNicC>(part, w.newest[7], frames, es, out, svals, seconds_per_sample, sample_base);
    es_part_take<kEsTrackPosition>(part, w.newest[8], frames, es, out, svals, seconds_per_sample, sample_base);
    es_part_take<kEsTrackCategory>(part, w.newest[9], frames, es, out, svals, seconds_per_sample, sample_base);
    es_part_take<kEsTrackNacV>(part, w.newest[10], frames, es, out, svals, seconds_per_sample, sample_base);
    EsWords words = ((const EsWords *)d.es)[slot - 1];
    adsb_aircraft_es a;
    __builtin_memcpy(&a, &words, sizeof(a));
    es_track_merge(a, part);
    __builtin_memcpy(&words, &a, sizeof(a));
    ((EsWords *)d.es)[slot - 1] = words;
}

hipError_t launch_es_merge(hipStream_t st, const TrackArgs &a, const TrackStoreDev &d)
{
    const TrackEsDev &x = *a.es;
    const dim3 grid((a.n + 255) / 256);
    const auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0u),
                                                     EsRefInput{(const uint32_t *)a.skeys, (const uint32_t *)a.svals, a.es_recs});
    size_t tb = x.temp_bytes;
    hipError_t e = rocprim::inclusive_scan(x.temp, tb, in, x.ref, (size_t)a.n, EsRefOp(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(track_es_frame_kernel, grid, dim3(256), 0, st, a.frames, a.es_recs, (const uint32_t *)a.skeys,
                       (const uint32_t *)a.svals, a.n, a.seconds_per_sample, a.sample_base, d,
                       (const TrackEsRefTuple *)x.ref, x.max_age_s, x.out, x.in);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    tb = x.temp_bytes;
    e = rocprim::inclusive_scan(x.temp, tb, (const TrackEsTuple *)x.in, x.scan, (size_t)a.n, EsOp(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(track_es_merge_kernel, grid, dim3(256), 0, st, a.frames, a.es_recs,
                       (const adsb_frame_integrity *)x.out, (const uint32_t *)a.skeys, (const uint32_t *)a.svals, a.n,
                       a.seconds_per_sample, a.sample_base, d, (const TrackEsTuple *)x.scan);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void track_es_clear_kernel(EsWords *es, uint64_t places)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < places) es[p] = es_track_empty();
}

// expire, 1: keep[g] = 1 for a record in use whose last frame is not older than the cut (last_heard < before evicts).
// Record g is slot i of receiver r (a table: r = 0).  Slot 0 stages the old size where the compaction kernel reads it
// (size_next[r]), since that kernel writes the new one; the pairs kernel of an update has consumed its own staging before
// anything later on the stream runs.
template <TrackKind K>
__global__ __launch_bounds__(256) void track_expire_mark_kernel(TrackStoreDev d, ExpireCut cut, uint32_t *keep,
                                                                uint64_t n_rec)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_rec) return;
    const uint32_t r = K == TrackKind::kBank ? (uint32_t)(g / d.max_aircraft) : 0u;
    const uint32_t i = (uint32_t)(g - (uint64_t)r * d.max_aircraft);
    const uint32_t size = d.size[r];
    if (i == 0) d.size_next[r] = size;
    keep[g] = (i < size && !(d.rec[g].last_heard < cut.before[r])) ? 1u : 0u;
}

// expire, 2 (after the exclusive scan rank of keep): the new size S = survivors; an evicted record below S is a hole
// that takes the k-th survivor at or above S (k = holes before it), found by a binary search over the local ranks.
// Holes are below S and the survivors they take at or above it, so no thread reads a record another one writes.  A
// table fixes its index here: the entries of evicted ICAOs are cleared, the moved ones point at their new slot.
template <TrackKind K>
__global__ __launch_bounds__(256) void track_expire_compact_kernel(TrackStoreDev d, const uint32_t *keep,
                                                                   const uint32_t *rank, uint64_t n_rec)
{
    constexpr bool kBank = K == TrackKind::kBank;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_rec) return;
    const uint32_t r = kBank ? (uint32_t)(g / d.max_aircraft) : 0u;
    const uint64_t base = (uint64_t)r * d.max_aircraft;
    const uint32_t i = (uint32_t)(g - base);
    const uint32_t size = d.size_next[r];
    const uint32_t rank0 = rank[base];
    const uint32_t survivors = size ? rank[base + size - 1] + keep[base + size - 1] - rank0 : 0u;
    if (i == 0) d.size[r] = survivors;
    if (i >= size || keep[g]) return;
    if (!kBank) d.index[d.rec[g].a.icao] = 0;
    if (i >= survivors) return;
    // a hole below `survivors` (so at least one survivor sits in [survivors, size)): k-th hole <- k-th such survivor,
    // the one whose local rank is m; it is the last slot in [survivors, size) with local rank <= m
    const uint32_t m = rank[base + survivors] - rank0 + (i - (rank[g] - rank0));
    uint32_t lo = survivors, hi = size; // local rank(lo) <= m; hi = size or local rank(hi) > m
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (rank[base + mid] - rank0 > m)
            hi = mid;
        else
            lo = mid;
    }
    const TrackRecord moved = d.rec[base + lo];
    d.rec[g] = moved;
    if (d.lvl) d.lvl[g] = d.lvl[base + lo];
    if (d.fix) ((FixWords *)d.fix)[g] = ((const FixWords *)d.fix)[base + lo];
    if (d.mlat) ((MlatWords *)d.mlat)[g] = ((const MlatWords *)d.mlat)[base + lo];
    if (d.modes) ((ModesWords *)d.modes)[g] = ((const ModesWords *)d.modes)[base + lo];
    if (d.commb) ((CommbWords *)d.commb)[g] = ((const CommbWords *)d.commb)[base + lo];
    if (d.es) ((EsWords *)d.es)[g] = ((const EsWords *)d.es)[base + lo];
    if (d.filter) ((FilterWords *)d.filter)[g] = ((const FilterWords *)d.filter)[base + lo];
    if (!kBank) d.index[moved.a.icao] = i + 1u;
}

// expire, 3 (bank only, after the hash was cleared): every surviving record reinserts (slot + 1) << 32 | key
__global__ __launch_bounds__(256) void track_bank_rehash_kernel(TrackStoreDev b, uint64_t n_rec)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_rec) return;
    const uint32_t r = (uint32_t)(g / b.max_aircraft);
    if ((uint32_t)(g - (uint64_t)r * b.max_aircraft) >= b.size[r]) return;
    const uint32_t key = r << 24 | (b.rec[g].a.icao & 0xFFFFFFu);
    const unsigned long long entry = (unsigned long long)(g + 1u) << 32 | key;
    for (uint64_t h = bank_hash(key) & b.hash_mask;; h = (h + 1) & b.hash_mask) // load <= 1/2: an empty entry exists
        if (atomicCAS(&b.hash[h], 0ull, entry) == 0ull) break;
}

// ---- the fused view of a bank --------------------------------------------------------------------------------------
constexpr uint32_t kFuseNone = 0xFFFFFFFFu; // a sorted position: no record yet

// fuse, 1: one thread per place p = r x max_aircraft + slot
template <class K>
__global__ __launch_bounds__(256) void fuse_keys_kernel(TrackStoreDev b, double since, uint32_t rbits, K *keys,
                                                        uint32_t *vals, uint64_t places)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= places) return;
    const uint32_t r = (uint32_t)(p / b.max_aircraft);
    K key = (K)1 << (24 + rbits);
    if ((uint32_t)(p - (uint64_t)r * b.max_aircraft) < b.size[r]) {
        const TrackRecord &rec = b.rec[p];
        if (rec.last_heard >= since) key = (K)(rec.a.icao & 0xFFFFFFu) << rbits | r;
    }
    keys[p] = key;
    vals[p] = (uint32_t)p;
}

// 1 where an ICAO's run starts in sorted order (the scan's input, and fuse_starts_kernel's test)
template <class K>
struct FuseHead {
    const K *skeys;
    uint32_t rbits;
    __device__ __forceinline__ uint32_t operator()(uint32_t s) const
    {
        const uint32_t icao = (uint32_t)(skeys[s] >> rbits);
        return (icao < (1u << 24) && (s == 0 || (uint32_t)(skeys[s - 1] >> rbits) != icao)) ? 1u : 0u;
    }
};

// fuse, 3 (after the exclusive scan excl of the heads): run g starts at seg_start[g]; the last thread publishes the
// counts and the flag
template <class K>
__global__ __launch_bounds__(256) void fuse_starts_kernel(FuseHead<K> head, const uint32_t *excl, uint64_t places,
                                                          uint64_t max_fused, uint32_t *seg_start, uint64_t *counts)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= places) return;
    const uint32_t h = head((uint32_t)s), g = excl[s];
    if (h && g < max_fused) seg_start[g] = (uint32_t)s;
    if (s + 1 == places) {
        const uint64_t total = (uint64_t)g + h;
        counts[0] = total < max_fused ? total : max_fused;
        counts[1] = total;
        counts[2] = total > max_fused ? ADSB_TRACK_FUSED_TRUNCATED : 0u;
    }
}

// the newest record so far for one quantity: the greatest time, and among equal times the lowest sorted position
struct FuseBest {
    double t;
    uint32_t w; // sorted position, kFuseNone: no candidate
    __device__ __forceinline__ void take(double t2, uint32_t w2)
    {
        if (w2 != kFuseNone && (w == kFuseNone || t2 > t || (t2 == t && w2 < w))) {
            t = t2;
            w = w2;
        }
    }
    template <int G>
    __device__ __forceinline__ void across() // every lane of the group ends with the group's best
    {
        for (int m = G / 2; m > 0; m >>= 1) take(__shfl_xor(t, m, G), __shfl_xor(w, m, G));
    }
};

// fuse, 4: G lanes per ICAO run (1 .. n_receivers records, receivers ascending), 256 / G runs per workgroup.  Lane l
// looks at the run's records l, l + G, ...; a butterfly leaves every lane with the five winners, the frame sum and the
// count; lane 0 copies the winners' fields into the workgroup's stage in LDS, and the whole workgroup stores the stage
// as consecutive 16-byte pieces (a lane storing its own 128-byte record would touch every line eight times).
template <class K, int G>
__global__ __launch_bounds__(256) void fuse_reduce_kernel(const TrackRecord *rec, const K *skeys, const uint32_t *svals,
                                                          const uint32_t *seg_start, const uint64_t *counts,
                                                          uint32_t rbits, uint64_t places, adsb_fused_aircraft *out)
{
    constexpr uint32_t kRuns = 256 / G;
    __shared__ __attribute__((aligned(16))) adsb_fused_aircraft stage[kRuns];
    const uint64_t n_out = counts[0], g0 = (uint64_t)blockIdx.x * kRuns;
    if (g0 >= n_out) return; // the whole workgroup leaves
    const uint32_t run = threadIdx.x / G, lane = threadIdx.x % G;
    if (g0 + run < n_out) { // a group is inside as a whole: the shuffles below stay among its G lanes
        const uint32_t start = seg_start[g0 + run];
        const uint32_t icao = (uint32_t)(skeys[start] >> rbits);
        FuseBest heard{0.0, kFuseNone}, contact{0.0, kFuseNone}, fix{0.0, kFuseNone}, ident{0.0, kFuseNone},
            vel{0.0, kFuseNone};
        uint64_t frames = 0;
        uint32_t n = 0;
        for (uint64_t w = (uint64_t)start + lane; w < places && (uint32_t)(skeys[w] >> rbits) == icao; w += G) {
            const TrackRecord &r = rec[svals[w]];
            const double lc = r.a.last_contact, lh = r.last_heard;
            uint64_t cs;
            __builtin_memcpy(&cs, r.a.callsign, 8);
            heard.take(lh, (uint32_t)w);
            if (lc == lc) contact.take(lc, (uint32_t)w);
            if (r.a.has_position) fix.take(lc, (uint32_t)w);
            if (cs != 0) ident.take(lh, (uint32_t)w);
            if (r.vel.subtype != 0) vel.take(r.vel.time, (uint32_t)w);
            frames += r.a.n_frames;
            ++n;
        }
        heard.across<G>();
        contact.across<G>();
        fix.across<G>();
        ident.across<G>();
        vel.across<G>();
        for (int m = G / 2; m > 0; m >>= 1) {
            frames += __shfl_xor(frames, m, G);
            n += __shfl_xor(n, m, G);
        }
        if (lane == 0) {
            const uint32_t rmask = (1u << rbits) - 1u;
            adsb_fused_aircraft f{}; // reserved, and every quantity nobody has: 0
            f.icao = icao;
            f.n_frames = frames;
            f.n_receivers = (uint16_t)n;
            f.heard_receiver = (uint16_t)((uint32_t)skeys[heard.w] & rmask); // a run has at least one record
            f.last_heard = heard.t;
            f.contact_receiver = f.position_receiver = f.callsign_receiver = f.velocity_receiver = ADSB_FUSED_NONE;
            f.last_contact = f.position_time = f.velocity_time = __builtin_nan("");
            if (contact.w != kFuseNone) {
                f.contact_receiver = (uint16_t)((uint32_t)skeys[contact.w] & rmask);
                f.last_contact = contact.t;
                f.altitude = rec[svals[contact.w]].a.altitude;
            }
            if (fix.w != kFuseNone) {
                const TrackRecord &r = rec[svals[fix.w]];
                f.position_receiver = (uint16_t)((uint32_t)skeys[fix.w] & rmask);
                f.has_position = 1;
                f.latitude = r.a.latitude;
                f.longitude = r.a.longitude;
                f.position_time = r.a.last_contact;
            }
            if (ident.w != kFuseNone) {
                f.callsign_receiver = (uint16_t)((uint32_t)skeys[ident.w] & rmask);
                __builtin_memcpy(f.callsign, rec[svals[ident.w]].a.callsign, 8);
            }
            if (vel.w != kFuseNone) {
                const adsb_velocity v = rec[svals[vel.w]].vel; // field by field: plain moves keep every bit
                f.velocity_receiver = (uint16_t)((uint32_t)skeys[vel.w] & rmask);
                f.velocity_time = v.time;
                f.speed_kt = v.speed_kt;
                f.direction_deg = v.direction_deg;
                f.vertical_rate_fpm = v.vertical_rate_fpm;
                f.v_ew_kt = v.v_ew_kt;
                f.v_ns_kt = v.v_ns_kt;
                f.velocity_subtype = v.subtype;
                f.velocity_flags = v.flags;
                f.vrate_baro = v.vrate_baro;
                f.airspeed_tas = v.airspeed_tas;
                f.velocity_reserved = v.reserved;
            }
            stage[run] = f;
        }
    }
    __syncthreads();
    const uint32_t pieces = (uint32_t)(n_out - g0 < kRuns ? n_out - g0 : kRuns) * (uint32_t)(sizeof(adsb_fused_aircraft) / 16);
    const uint4 *src = (const uint4 *)stage;
    uint4 *dst = (uint4 *)(out + g0); // 128-byte records in hipMalloc'ed memory: 16-byte aligned
    for (uint32_t i = threadIdx.x; i < pieces; i += 256) dst[i] = src[i];
}

// fuse, 5 (banks with a levels reserve): one thread per written fused record walks its ICAO run (receivers ascending)
// over the level records beside the bank's records.  a is stronger than b iff a.signal_total x b.n_levels >
// b.signal_total x a.n_levels, as 96-bit products (high and low word of a 64 x 64 multiply); only a strictly greater
// mean replaces the best so far, so ties stay with the lowest receiver.
template <class K>
__global__ __launch_bounds__(256) void fuse_levels_kernel(const adsb_aircraft_level *lvl, const K *skeys,
                                                          const uint32_t *svals, const uint32_t *seg_start,
                                                          const uint64_t *counts, uint32_t rbits, uint64_t places,
                                                          adsb_fused_level *out)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= counts[0]) return;
    const uint32_t start = seg_start[g], rmask = (1u << rbits) - 1u;
    const uint32_t icao = (uint32_t)(skeys[start] >> rbits);
    adsb_fused_level f{};
    adsb_aircraft_level strongest = empty_level(); // f's first 64 bytes
    f.strongest_receiver = ADSB_FUSED_NONE;
    uint64_t best_total = 0, best_n = 0, best_w = 0; // the strongest so far: its totals and sorted position; n 0 = none
    uint32_t heard = 0;
    for (uint64_t w = start; w < places && (uint32_t)(skeys[w] >> rbits) == icao; ++w) {
        const adsb_aircraft_level &a = lvl[svals[w]];
        const uint64_t total = a.signal_total, n = a.n_levels;
        f.signal_total = sat_add64(f.signal_total, total);
        f.noise_total = sat_add64(f.noise_total, a.noise_total);
        f.n_levels += n;
        if (n == 0) continue;
        ++heard;
        bool better = best_n == 0;
        if (!better) { // total x best_n against best_total x n
            const uint64_t new_lo = total * best_n, new_hi = __umul64hi(total, best_n);
            const uint64_t old_lo = best_total * n, old_hi = __umul64hi(best_total, n);
            better = new_hi > old_hi || (new_hi == old_hi && new_lo > old_lo);
        }
        if (better) {
            best_total = total;
            best_n = n;
            best_w = w;
        }
    }
    if (best_n) { // the record whole, from memory, once
        strongest = lvl[svals[best_w]];
        f.strongest_receiver = (uint16_t)((uint32_t)skeys[best_w] & rmask);
    }
    __builtin_memcpy(&f, &strongest, sizeof(strongest));
    f.level_receivers = (uint16_t)heard;
    out[g] = f;
}

template <class K>
hipError_t fuse_sort_scan(void *temp, size_t &sort_bytes, size_t &scan_bytes, const K *keys, K *skeys,
                          const uint32_t *vals, uint32_t *svals, uint32_t *excl, size_t places, uint32_t rbits,
                          hipStream_t st)
{
    hipError_t e = rocprim::radix_sort_pairs(temp, sort_bytes, keys, skeys, vals, svals, places, 0, 25 + rbits, st);
    if (e != hipSuccess) return e;
    const auto heads = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0u),
                                                        FuseHead<K>{skeys, rbits});
    return rocprim::exclusive_scan(temp, scan_bytes, heads, excl, 0u, places, rocprim::plus<uint32_t>(), st);
}

template <class K>
hipError_t launch_fuse(hipStream_t st, const FuseArgs &a)
{
    const TrackStoreDev b = *a.bank;
    const uint64_t places = (uint64_t)b.n_receivers * b.max_aircraft;
    const uint32_t rbits = b.key_bits - 24, blocks = (uint32_t)((places + 255) / 256);
    K *keys = (K *)a.keys, *skeys = (K *)a.skeys;
    hipLaunchKernelGGL(fuse_keys_kernel<K>, dim3(blocks), dim3(256), 0, st, b, a.since, rbits, keys, a.vals, places);
    size_t sort_bytes = a.temp_bytes, scan_bytes = a.temp_bytes;
    uint32_t *excl = a.vals; // the sort has read vals
    hipError_t e = fuse_sort_scan<K>(a.temp, sort_bytes, scan_bytes, keys, skeys, a.vals, a.svals, excl, (size_t)places,
                                     rbits, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fuse_starts_kernel<K>, dim3(blocks), dim3(256), 0, st, FuseHead<K>{skeys, rbits},
                       (const uint32_t *)excl, places, a.max_fused, a.seg_start, a.counts);
    const dim3 grid((uint32_t)((a.max_fused * a.lanes + 255) / 256)); // workgroups past counts[0] leave at once
#define ADSB_FUSE_REDUCE(G)                                                                                            \
    hipLaunchKernelGGL((fuse_reduce_kernel<K, G>), grid, dim3(256), 0, st, (const TrackRecord *)b.rec,                 \
                       (const K *)skeys, (const uint32_t *)a.svals, (const uint32_t *)a.seg_start,                     \
                       (const uint64_t *)a.counts, rbits, places, a.out)
    switch (a.lanes) {
    case 1: ADSB_FUSE_REDUCE(1); break;
    case 4: ADSB_FUSE_REDUCE(4); break;
    default: return hipErrorInvalidValue;
    }
#undef ADSB_FUSE_REDUCE
    if (a.lvl_out) // workgroups past counts[0] leave at once
        hipLaunchKernelGGL(fuse_levels_kernel<K>, dim3((uint32_t)((a.max_fused + 255) / 256)), dim3(256), 0, st,
                           (const adsb_aircraft_level *)b.lvl, (const K *)skeys, (const uint32_t *)a.svals,
                           (const uint32_t *)a.seg_start, (const uint64_t *)a.counts, rbits, places, a.lvl_out);
    return hipGetLastError();
}

} // namespace

size_t track_expire_temp_bytes(size_t n_rec)
{
    size_t scan_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, scan_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, n_rec,
                                  rocprim::plus<uint32_t>(), (hipStream_t)0);
    return scan_bytes + 256;
}

namespace {
// mark -> scan -> compaction; a bank then clears its hash and reinserts the survivors
template <TrackKind K>
hipError_t track_expire(hipStream_t st, const ExpireArgs &a)
{
    const TrackStoreDev d = *a.store;
    const uint64_t n_rec = (uint64_t)d.max_aircraft * d.n_receivers;
    if (n_rec == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)((n_rec + 255) / 256);
    hipLaunchKernelGGL(track_expire_mark_kernel<K>, dim3(blocks), dim3(256), 0, st, d, a.cut, a.keep, n_rec);
    size_t tb = a.temp_bytes;
    hipError_t e = rocprim::exclusive_scan(a.temp, tb, (const uint32_t *)a.keep, a.rank, 0u, (size_t)n_rec,
                                           rocprim::plus<uint32_t>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(track_expire_compact_kernel<K>, dim3(blocks), dim3(256), 0, st, d, (const uint32_t *)a.keep,
                       (const uint32_t *)a.rank, n_rec);
    if (K == TrackKind::kBank) {
        if ((e = hipMemsetAsync(d.hash, 0, sizeof(unsigned long long) * (d.hash_mask + 1), st)) != hipSuccess) return e;
        hipLaunchKernelGGL(track_bank_rehash_kernel, dim3(blocks), dim3(256), 0, st, d, n_rec);
    }
    return hipGetLastError();
}
} // namespace

hipError_t launch_track_expire(hipStream_t st, const ExpireArgs &a)
{
    return a.kind == TrackKind::kBank ? track_expire<TrackKind::kBank>(st, a) : track_expire<TrackKind::kTable>(st, a);
}

size_t track_fuse_temp_bytes(size_t places, uint32_t n_receivers)
{
    uint32_t rbits = 0;
    while ((1u << rbits) < n_receivers) ++rbits;
    size_t sort_bytes = 0, scan_bytes = 0;
    if (n_receivers > kFuseWideReceivers)
        (void)fuse_sort_scan<uint64_t>(nullptr, sort_bytes, scan_bytes, nullptr, nullptr, nullptr, nullptr, nullptr, places,
                                       rbits, (hipStream_t)0);
    else
        (void)fuse_sort_scan<uint32_t>(nullptr, sort_bytes, scan_bytes, nullptr, nullptr, nullptr, nullptr, nullptr, places,
                                       rbits, (hipStream_t)0);
    return (sort_bytes > scan_bytes ? sort_bytes : scan_bytes) + 256;
}

hipError_t launch_track_fuse(hipStream_t st, const FuseArgs &a)
{
    return a.bank->n_receivers > kFuseWideReceivers ? launch_fuse<uint64_t>(st, a) : launch_fuse<uint32_t>(st, a);
}

size_t track_sort_temp_bytes(size_t n)
{
    size_t sort_bytes = 0, scan_bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                    (const uint32_t *)nullptr, (uint32_t *)nullptr, n, 0, 24, (hipStream_t)0);
    (void)rocprim::exclusive_scan(nullptr, scan_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, n,
                                  rocprim::plus<uint32_t>(), (hipStream_t)0);
    return (sort_bytes > scan_bytes ? sort_bytes : scan_bytes) + 256;
}

size_t track_bank_temp_bytes(size_t n)
{
    size_t sort_bytes = 0, scan_bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                    (const uint32_t *)nullptr, (uint32_t *)nullptr, n, 0, 32, (hipStream_t)0);
    (void)rocprim::exclusive_scan(nullptr, scan_bytes, (const unsigned long long *)nullptr,
                                  (unsigned long long *)nullptr, 0ull, n, rocprim::plus<unsigned long long>(),
                                  (hipStream_t)0);
    return (sort_bytes > scan_bytes ? sort_bytes : scan_bytes) + 256;
}

size_t track_summaries_temp_bytes(size_t n)
{
    size_t scan_bytes = 0;
    (void)rocprim::inclusive_scan(nullptr, scan_bytes, (const TrackSumTuple *)nullptr, (TrackSumTuple *)nullptr, n,
                                  SumOp(), (hipStream_t)0);
    return scan_bytes + 256;
}

size_t track_levels_temp_bytes(size_t n)
{
    size_t scan_bytes = 0;
    (void)rocprim::inclusive_scan(nullptr, scan_bytes, (const TrackLvlTuple *)nullptr, (TrackLvlTuple *)nullptr, n,
                                  LvlOp(), (hipStream_t)0);
    return scan_bytes + 256;
}

size_t track_fixes_temp_bytes(size_t n)
{
    size_t scan_bytes = 0;
    (void)rocprim::inclusive_scan(nullptr, scan_bytes, (const TrackFixTuple *)nullptr, (TrackFixTuple *)nullptr, n,
                                  FixOp(), (hipStream_t)0);
    return scan_bytes + 256;
}

size_t track_mlat_temp_bytes(size_t n)
{
    size_t scan_bytes = 0;
    (void)rocprim::inclusive_scan(nullptr, scan_bytes, (const TrackMlatTuple *)nullptr, (TrackMlatTuple *)nullptr, n,
                                  MlatOp(), (hipStream_t)0);
    return scan_bytes + 256;
}

size_t track_modes_temp_bytes(size_t n)
{
    size_t sort_bytes = 0, excl_bytes = 0, scan_bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                    (const uint32_t *)nullptr, (uint32_t *)nullptr, n, 0, 25, (hipStream_t)0);
    (void)rocprim::exclusive_scan(nullptr, excl_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, n,
                                  rocprim::plus<uint32_t>(), (hipStream_t)0);
    (void)rocprim::inclusive_scan(nullptr, scan_bytes, (const TrackModesTuple *)nullptr, (TrackModesTuple *)nullptr, n,
                                  ModesOp(), (hipStream_t)0);
    const size_t most = sort_bytes > excl_bytes ? sort_bytes : excl_bytes;
    return (most > scan_bytes ? most : scan_bytes) + 256;
}

size_t track_commb_temp_bytes(size_t n)
{
    size_t ref_bytes = 0, scan_bytes = 0;
    const auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0u),
                                                     CommbRefInput{nullptr, nullptr, nullptr, nullptr});
    (void)rocprim::inclusive_scan(nullptr, ref_bytes, in, (TrackCommbRefTuple *)nullptr, n, CommbRefOp(), (hipStream_t)0);
    (void)rocprim::inclusive_scan(nullptr, scan_bytes, (const TrackCommbTuple *)nullptr, (TrackCommbTuple *)nullptr, n,
                                  CommbOp(), (hipStream_t)0);
    return (ref_bytes > scan_bytes ? ref_bytes : scan_bytes) + 256;
}

hipError_t launch_track_commb_clear(hipStream_t st, adsb_aircraft_commb *commb, size_t places)
{
    if (places == 0) return hipSuccess;
    hipLaunchKernelGGL(track_commb_clear_kernel, dim3((uint32_t)((places + 255) / 256)), dim3(256), 0, st,
                       (CommbWords *)commb, (uint64_t)places);
    return hipGetLastError();
}

size_t track_es_temp_bytes(size_t n)
{
    size_t ref_bytes = 0, scan_bytes = 0;
    const auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0u),
                                                     EsRefInput{nullptr, nullptr, nullptr});
    (void)rocprim::inclusive_scan(nullptr, ref_bytes, in, (TrackEsRefTuple *)nullptr, n, EsRefOp(), (hipStream_t)0);
    (void)rocprim::inclusive_scan(nullptr, scan_bytes, (const TrackEsTuple *)nullptr, (TrackEsTuple *)nullptr, n, EsOp(),
                                  (hipStream_t)0);
    return (ref_bytes > scan_bytes ? ref_bytes : scan_bytes) + 256;
}

hipError_t launch_track_es_clear(hipStream_t st, adsb_aircraft_es *es, size_t places)
{
    if (places == 0) return hipSuccess;
    hipLaunchKernelGGL(track_es_clear_kernel, dim3((uint32_t)((places + 255) / 256)), dim3(256), 0, st, (EsWords *)es,
                       (uint64_t)places);
    return hipGetLastError();
}

hipError_t launch_track_modes_clear(hipStream_t st, adsb_aircraft_modes *modes, size_t places)
{
    if (places == 0) return hipSuccess;
    hipLaunchKernelGGL(track_modes_clear_kernel, dim3((uint32_t)((places + 255) / 256)), dim3(256), 0, st,
                       (ModesWords *)modes, (uint64_t)places);
    return hipGetLastError();
}

hipError_t launch_track_mlat_clear(hipStream_t st, adsb_aircraft_mlat *mlat, size_t places)
{
    if (places == 0) return hipSuccess;
    hipLaunchKernelGGL(track_mlat_clear_kernel, dim3((uint32_t)((places + 255) / 256)), dim3(256), 0, st,
                       (MlatWords *)mlat, (uint64_t)places);
    return hipGetLastError();
}

hipError_t launch_track_filter_clear(hipStream_t st, adsb_aircraft_filter *filter, size_t places)
{
    if (places == 0) return hipSuccess;
    hipLaunchKernelGGL(track_filter_clear_kernel, dim3((uint32_t)((places + 255) / 256)), dim3(256), 0, st,
                       (FilterWords *)filter, (uint64_t)places);
    return hipGetLastError();
}

hipError_t launch_track_fixes_clear(hipStream_t st, adsb_fix *fix, size_t places)
{
    if (places == 0) return hipSuccess;
    hipLaunchKernelGGL(track_fixes_clear_kernel, dim3((uint32_t)((places + 255) / 256)), dim3(256), 0, st,
                       (FixWords *)fix, (uint64_t)places);
    return hipGetLastError();
}

hipError_t launch_track_levels_clear(hipStream_t st, adsb_aircraft_level *lvl, size_t places)
{
    if (places == 0) return hipSuccess;
    hipLaunchKernelGGL(track_levels_clear_kernel, dim3((uint32_t)((places + 255) / 256)), dim3(256), 0, st, lvl,
                       (uint64_t)places);
    return hipGetLastError();
}

hipError_t launch_track_changed(hipStream_t st, const TrackRecord *rec, const TrackSumDev &sum, uint32_t max_n,
                                TrackRecord *out)
{
    if (max_n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((uint64_t)max_n * 8 + 255) / 256); // eight lanes per record
    hipLaunchKernelGGL(track_changed_gather_kernel, dim3(blocks), dim3(256), 0, st, rec, (const uint32_t *)sum.changed,
                       (const uint32_t *)sum.n_changed, max_n, out);
    return hipGetLastError();
}

namespace {
// What follows the sort (and, with a table or bank, lookup and admission): pairs, then per-frame summaries if reserved
// and the merge into the records; the per-launch form ranks its segment tails and summarises into a.aircraft instead.
template <TrackKind K>
hipError_t track_tail(hipStream_t st, const TrackArgs &a, const TrackStoreDev &d)
{
    constexpr bool kStore = K != TrackKind::kLaunch;
    const uint32_t n = a.n, blocks = (n + 255) / 256;
    uint32_t *tail_flag = kStore ? nullptr : a.keys, *tail_pos = kStore ? nullptr : a.vals; // reused
    hipLaunchKernelGGL(track_pairs_kernel<K>, dim3(blocks), dim3(256), 0, st, a.frames, a.fields, a.skeys, a.svals, n,
                       a.seconds_per_sample, a.sample_base, d, a.points, tail_flag);
    hipError_t e = hipSuccess;
    if constexpr (kStore) {
        if (a.lvl && d.lvl) e = launch_levels_merge<K>(st, a, d); // needs d.slot only: independent of the record merge
        if (e != hipSuccess) return e;
        if (a.fix && d.fix) e = launch_fix_merge<K>(st, a, d); // needs d.slot and the frame bytes only
        if (e != hipSuccess) return e;
        if (a.mlat && d.mlat) e = launch_mlat_merge<K>(st, a, d); // needs d.slot, the frame bytes and the fixes only
        if (e != hipSuccess) return e;
        if constexpr (K == TrackKind::kTable) {
            if (a.mlat && d.mlat && a.filter && d.filter) e = launch_filter<K>(st, a, d); // d.slot, the sort, the fixes
            if (e != hipSuccess) return e;
        }
        if constexpr (K == TrackKind::kTable) {
            if (a.es && d.es) e = launch_es_merge(st, a, d); // needs d.slot, the es records and its own side array only
            if (e != hipSuccess) return e;
        }
        if (a.sum) e = launch_frame_summaries<K>(st, a, d); // before the merge
        if constexpr (K == TrackKind::kTable) {
            if (e != hipSuccess) return e;
            if (a.modes && d.modes) e = launch_modes_merge(st, a, d); // after every kernel that writes a per-frame icao
            if (e != hipSuccess) return e;
            if (a.commb && a.modes && d.commb && d.modes) e = launch_commb_merge(st, a, d); // before the merge: rec.vel
        }
    } else {
        size_t tb = a.temp_bytes;
        e = rocprim::exclusive_scan(a.temp, tb, (const uint32_t *)tail_flag, tail_pos, 0u, (size_t)n,
                                    rocprim::plus<uint32_t>(), st);
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(track_summary_kernel<K>, dim3(blocks), dim3(256), 0, st, a.frames, a.fields, a.points, a.skeys,
                       a.svals, (const uint32_t *)tail_flag, (const uint32_t *)tail_pos, n, a.seconds_per_sample,
                       a.sample_base, d, a.aircraft, a.max_aircraft, a.n_aircraft);
    return hipGetLastError();
}
} // namespace

hipError_t launch_track(hipStream_t st, const TrackArgs &a)
{
    const bool store = a.kind != TrackKind::kLaunch;
    if (a.n == 0) return store ? hipSuccess : hipMemsetAsync(a.n_aircraft, 0, sizeof(uint64_t), st);
    const uint32_t n = a.n, blocks = (n + 255) / 256;
    const TrackStoreDev d = store ? *a.store : TrackStoreDev{};
    size_t tb = a.temp_bytes;
    if (a.kind == TrackKind::kBank) {
        const uint32_t kblocks = ((n > d.n_receivers ? n : d.n_receivers + 1u) + 255u) / 256u;
        hipLaunchKernelGGL(track_bank_keys_kernel, dim3(kblocks), dim3(256), 0, st, a.fields, n, d, a.keys, a.vals);
        hipError_t e = rocprim::radix_sort_pairs(a.temp, tb, (const uint32_t *)a.keys, a.skeys,
                                                 (const uint32_t *)a.vals, a.svals, (size_t)n, 0, d.key_bits, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(track_bank_lookup_kernel, dim3(blocks), dim3(256), 0, st, a.skeys, n, d);
        tb = a.temp_bytes;
        e = rocprim::exclusive_scan(a.temp, tb, (const unsigned long long *)d.mark, d.excl, 0ull, (size_t)n,
                                    rocprim::plus<unsigned long long>(), st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(track_bank_admit_kernel, dim3(blocks), dim3(256), 0, st, a.skeys, n, d);
        return track_tail<TrackKind::kBank>(st, a, d);
    }
    const bool modes = a.kind == TrackKind::kTable && a.modes && d.modes; // update_modes: keyed by the records' addresses
    if (modes)
        hipLaunchKernelGGL(track_modes_keys_kernel, dim3(blocks), dim3(256), 0, st, a.modes_fields, a.modes_recs, n,
                           a.keys, a.vals);
    else
        hipLaunchKernelGGL(track_keys_kernel, dim3(blocks), dim3(256), 0, st, a.fields, n, a.keys, a.vals);
    hipError_t e = rocprim::radix_sort_pairs(a.temp, tb, (const uint32_t *)a.keys, a.skeys, (const uint32_t *)a.vals,
                                             a.svals, (size_t)n, 0, modes ? 25 : 24, st);
    if (e != hipSuccess) return e;
    if (!store) return track_tail<TrackKind::kLaunch>(st, a, d);
    if (modes)
        hipLaunchKernelGGL(track_modes_lookup_kernel, dim3(blocks), dim3(256), 0, st, a.skeys, n, d.index, d.slot,
                           a.keys /* reused: is_new */);
    else
        hipLaunchKernelGGL(track_lookup_kernel, dim3(blocks), dim3(256), 0, st, a.skeys, n, d.index, d.slot,
                           a.keys /* reused: is_new */);
    tb = a.temp_bytes;
    e = rocprim::exclusive_scan(a.temp, tb, (const uint32_t *)a.keys, a.vals /* reused: rank */, 0u, (size_t)n,
                                rocprim::plus<uint32_t>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(track_admit_kernel, dim3(blocks), dim3(256), 0, st, a.skeys, n, a.keys, a.vals, d);
    return track_tail<TrackKind::kTable>(st, a, d);
}

} // namespace adsbk
