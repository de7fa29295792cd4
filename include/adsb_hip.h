/*
 * adsb_hip.h -- C ABI of the MI355X-native ADS-B demodulator (libadsb_hip.so).
 *
 * This is the drop-in boundary for air_rs's thread 2, `process_sdr_data_thread`
 * (reference: src/adsb.rs:92-122).  The reference has no FFI of its own: thread 2 is a
 * private Rust fn fed by `mpsc::Receiver<Vec<Complex<i16>>>` (adsb.rs:131) and feeding
 * `mpsc::Sender<AdsbPacket>` (adsb.rs:146).  A maintainer keeps both channels and replaces the
 * body of the `while let Ok(buf) = rx.recv()` loop (adsb.rs:95-116) with one call to
 * adsb_demod() per received Vec, then builds `AdsbPacket::new(frame.bytes.to_vec())`
 * (adsb.rs:107) for every returned frame, in the order returned.  INTEGRATION.md shows the
 * Rust `extern "C"` block and the replacement loop.
 *
 * Everything here is plain C: opaque handle, pointers and sizes, POD structs, int return
 * codes.  No exceptions cross the boundary.  A context is NOT thread-safe: one context per
 * calling thread (the reference has exactly one consumer thread, adsb.rs:147) and one per GPU.
 */
#ifndef ADSB_HIP_H
#define ADSB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADSB_ABI_VERSION 1

/* ---- return codes ----------------------------------------------------------------------- */
#define ADSB_OK 0
/* n_samples < 240: the reference panics at adsb.rs:98 (`mags.len() - 240` underflows).
 * The caller decides whether to mimic the panic. */
#define ADSB_E_SHORT (-1)
#define ADSB_E_ARG (-2)      /* NULL / misaligned / inconsistent argument                      */
#define ADSB_E_CAPACITY (-3) /* n_samples or n_channels exceeds what the ctx was created for    */
#define ADSB_E_NOMEM (-4)
#define ADSB_E_NODEVICE (-5) /* no HIP device / HIP runtime failure at create                   */
#define ADSB_E_STATE (-6)    /* fetch without a launch, etc.                                    */
/* > 0 : a hipError_t from the HIP runtime */

/* ---- flags returned by fetch/demod ------------------------------------------------------- */
/* More than max_out frames exist; the first max_out (in offset order) were returned.
 * The reference has no cap (unbounded mpsc); see SURVEY F8 for why a cap is needed. */
#define ADSB_FLAG_TRUNCATED 0x1u
/* Only ever seen by device-side consumers (adsb_result_device's header, adsb_set_result_target's blob):
 * the launch ran out of temporary frame slots (far more gate survivors than max_out + one tile: constant or
 * all-zero input), so the list holds n_out entries of which some are not written yet.  The host
 * entry points that wait for a launch (adsb_fetch, adsb_fetch_counts, adsb_fetch_fields, adsb_track_device,
 * adsb_track_bank_update_launch) re-run the affected tiles, complete the list IN PLACE (blob included) and clear the flag; a consumer
 * that reads the device copy directly must check it and call adsb_fetch_counts() first when it is set. */
#define ADSB_FLAG_INCOMPLETE 0x2u

/* ---- sample formats ---------------------------------------------------------------------- */
/* ADSB_SAMPLE_I16 is the reference's `Complex<i16>` memory layout: interleaved {re, im},
 * 4 bytes per sample (adsb.rs:131; file format utils.rs:22-43).
 * ADSB_SAMPLE_I8 is interleaved {re, im} int8, 2 bytes per sample (RTL-SDR class radios,
 * BASELINE.json's metric).  i8 results are by definition those of the reference path on the
 * exactly widened i16 values. */
#define ADSB_SAMPLE_I8 0
#define ADSB_SAMPLE_I16 1

/* One decoded Mode-S extended squitter.  24-byte POD, identical on host and device. */
typedef struct adsb_frame {
    uint64_t offset;    /* index i of the first preamble sample inside its buffer/channel        */
    uint8_t  bytes[14]; /* what extract_packet returns (demod.rs:65-82): 11 data + 3 CRC bytes   */
    uint8_t  status;    /* 0: CRC matched (demod.rs:81); 1: one data bit repaired (crc.rs:49-65) */
    uint8_t  fixed_bit; /* status==1: repaired bit 0..87, MSB-first; otherwise 0xFF              */
} adsb_frame;

typedef struct adsb_cfg {
    uint32_t abi_version;  /* ADSB_ABI_VERSION                                                    */
    int32_t  device;       /* HIP device ordinal                                                  */
    int32_t  sample_type;  /* ADSB_SAMPLE_I8 / ADSB_SAMPLE_I16                                    */
    uint32_t max_channels; /* >= 1: how many independent buffers one launch may carry             */
    uint64_t max_samples;  /* per channel; sizes the segment table (and the H2D staging buffer)   */
    uint64_t max_out;      /* frames kept per launch, all channels together                       */
    void    *stream;       /* hipStream_t to enqueue on; NULL: the ctx creates and owns one       */
    uint32_t host_staging; /* 1: allocate a device staging buffer so adsb_demod() (host pointers)
                              works; 0: device-resident entry points only                         */
    uint32_t reserved;
} adsb_cfg;

typedef struct adsb_ctx adsb_ctx;

/* Replaces nothing in the reference (it has no setup step); owns device buffers and stream. */
int adsb_create(const adsb_cfg *cfg, adsb_ctx **out_ctx);
void adsb_destroy(adsb_ctx *ctx);
/* Static string for a return code of this library (HIP codes: hipGetErrorString). */
const char *adsb_strerror(int code);

/*
 * adsb_demod -- one iteration of the reference loop (adsb.rs:95-116) for one received buffer.
 *   iq        : host pointer, n_samples interleaved samples of cfg.sample_type
 *   out       : host array of max_out frames, filled in ascending offset order
 *   n_out     : number of frames written
 *   flags     : ADSB_FLAG_*
 * Returns ADSB_E_SHORT for n_samples < 240 (reference panics), ADSB_OK with *n_out = 0 for
 * n_samples == 240 (reference: zero iterations).  Blocking.  Requires cfg.host_staging.
 */
int adsb_demod(adsb_ctx *ctx, const void *iq, size_t n_samples, adsb_frame *out, size_t max_out,
               size_t *n_out, uint32_t *flags);

/*
 * Device-resident, asynchronous form (roofline configs, multi-channel batch).
 *   iq_dev          : device pointer, 16-byte aligned
 *   n_channels      : independent buffers; each is its own reference buffer (offsets
 *                     0..n_samples-240 per channel; no window crosses a channel edge)
 *   n_samples       : per channel
 *   channel_stride  : samples between channel starts (>= n_samples, multiple of 8)
 * Enqueues the kernels on the ctx stream and returns; results stay on the device until
 * adsb_fetch()/adsb_result_device().
 */
int adsb_demod_device_async(adsb_ctx *ctx, const void *iq_dev, uint32_t n_channels,
                            size_t n_samples, size_t channel_stride);

/*
 * Waits for the last launch and copies the frame list to the host.
 *   out               : host array of max_out frames: channel 0's frames in ascending offset,
 *                       then channel 1's, ...
 *   n_out             : frames written (all channels)
 *   per_channel_counts: optional array of n_channels uint64 (frames per channel in `out`)
 *   total_found       : optional; number of frames that exist (> *n_out when TRUNCATED)
 */
int adsb_fetch(adsb_ctx *ctx, adsb_frame *out, size_t max_out, size_t *n_out,
               uint64_t *per_channel_counts, uint64_t *total_found, uint32_t *flags);

/* Waits for the last launch and returns only the counters (8+8+4 bytes of D2H). */
int adsb_fetch_counts(adsb_ctx *ctx, uint64_t *n_out, uint64_t *total_found, uint32_t *flags);

/*
 * Zero-copy access for device-side consumers (e.g. an RCCL gather of the packet list):
 *   frames_dev : adsb_frame[ ] in device memory
 *   header_dev : device pointer to { uint64 n_out; uint64 total_found; uint32 flags; ... }
 * Order a consumer stream behind the launch that fills them with adsb_stream_wait_results().
 * If header.flags has ADSB_FLAG_INCOMPLETE the list has holes: call adsb_fetch_counts() (it re-runs what
 * is missing and clears the flag) before using it.
 * A context alternates between two result sets, so these pointers stay valid (and unchanged) until
 * the second-next adsb_demod_device_async() on this context.
 */
int adsb_result_device(adsb_ctx *ctx, const adsb_frame **frames_dev, const void **header_dev);
/*
 * Redirects the ordered frame list of the following launches into caller-owned device memory laid
 * out as [ uint64 n_out | uint64 total_found | uint64 flags | uint64 0 | adsb_frame[...] ]
 * (16-byte aligned; capacity = (blob_bytes - 32) / 24 frames, further capped by cfg.max_out).
 * Lets a consumer fill a multi-launch bucket in place (e.g. one RCCL gather per N launches) with
 * no device-to-device copy.  blob_dev == NULL returns to the context's own buffers.
 */
int adsb_set_result_target(adsb_ctx *ctx, void *blob_dev, size_t blob_bytes);
/*
 * Position of the next launches' sample 0 inside a longer stream: every frame of the following launches is
 * reported with offset = first_sample_index + (index of its first preamble sample inside the buffer), in
 * every channel.  0 (the default) gives the reference's per-buffer offsets (adsb.rs:98).  A rank that owns
 * the slice [first, first + n) of a time-sharded stream sets this to `first`, and the per-rank lists
 * concatenate into one globally ordered list with no host-side rebasing.
 */
int adsb_set_stream_base(adsb_ctx *ctx, uint64_t first_sample_index);
/* Makes `stream` (hipStream_t) wait for the results of the last launch; does not block the host.
 * (It cannot repair an ADSB_FLAG_INCOMPLETE list: that takes the host, see adsb_fetch_counts.) */
int adsb_stream_wait_results(adsb_ctx *ctx, void *stream);

/*
 * ---- streaming front end -------------------------------------------------------------
 * The reference's thread 2 receives one Vec per recv() (src/adsb.rs:95) from the SDR reader (adsb.rs:54-73) or
 * the playback thread (adsb.rs:75-89) and treats each as an island.  A feed takes the same sequence of host
 * buffers and keeps the GPU busy across them: each buffer goes through a pinned host ring to one of two device
 * staging slots by asynchronous DMA on a copy stream, overlapped with the previous buffer's kernels; up to two
 * buffers are in flight, results come back in order from adsb_feed_pop().  The ctx must have been created with
 * max_samples >= max_chunk (+ 240 in carry mode; cfg.host_staging is not needed) and must not be used for other
 * launches while the feed is open.
 *   carry = 0 (default, the reference's behaviour): every buffer is its own reference buffer: offsets
 *     0 .. n-241 of each are examined, frames straddling two buffers are lost (adsb.rs:98); frame
 *     offsets are buffer-relative (*first_sample of adsb_feed_pop says where the buffer began in the stream); a
 *     buffer shorter than 240 samples makes adsb_feed_push return ADSB_E_SHORT (the reference panics).
 *   carry = 1 (NOT reference behaviour): the last 240 samples seen so far stay on the device and are copied,
 *     device to device, in front of the next buffer: the chunked stream decodes exactly like one long buffer of
 *     the same samples; frame offsets are absolute stream positions.
 */
typedef struct adsb_feed adsb_feed;
typedef struct adsb_feed_cfg {
    size_t   max_chunk;   /* largest buffer (samples) that will be pushed                          */
    uint32_t carry;       /* 0 = per-buffer semantics (reference), 1 = carry the 240-sample tail    */
    uint32_t ring_slots;  /* pinned host buffers of max_chunk samples (0: 3)                        */
    /* Rule: a ring slot whose buffer went through the one-dispatch kernel is not handed out (adsb_feed_acquire) or
     * overwritten (adsb_feed_push) until that buffer has been popped or its list is complete (ADSB_FLAG_INCOMPLETE
     * cleared in its result blob): the kernel reads its samples from the slot itself, and a list with tiles over
     * their slots is rebuilt from those same samples.  With 2 slots and two buffers in flight the slot handed out
     * belongs to the oldest, unpopped buffer: acquire / push then wait for its kernel and, if need be, rebuild its
     * list first.  With 3 or more slots the slot always belongs to a popped buffer. */
} adsb_feed_cfg;
int adsb_feed_open(adsb_ctx *ctx, const adsb_feed_cfg *cfg, adsb_feed **out_feed);
/* Optional zero-copy producer path: a pinned ring slot (max_chunk samples) to fill in place; hand it over with
 * adsb_feed_push(feed, NULL, n).  Blocks only if the DMA out of that slot, or the unpopped one-dispatch launch that
 * reads it (see ring_slots), has not finished yet. */
int adsb_feed_acquire(adsb_feed *feed, void **host_slot);
/* Enqueues one buffer (copied into the ring unless it was acquired) and returns without waiting for the GPU.
 * ADSB_E_STATE when two buffers are already in flight (pop first). */
int adsb_feed_push(adsb_feed *feed, const void *iq_host, size_t n_samples);
/* Waits for the OLDEST buffer in flight and returns its frames in ascending offset order; *first_sample
 * (optional) = stream position of that buffer's first sample.  ADSB_E_STATE when nothing is in flight. */
int adsb_feed_pop(adsb_feed *feed, adsb_frame *out, size_t max_out, size_t *n_out, uint32_t *flags,
                  uint64_t *first_sample);
int adsb_feed_in_flight(const adsb_feed *feed); /* 0, 1 or 2 */
/* 1: adsb_feed_pop() would return the oldest buffer's frames without waiting for the GPU; 0: it would wait;
 * ADSB_E_STATE: nothing is in flight.  Lets a consumer hand packets on as soon as they exist instead of one buffer
 * late (the reference sends a buffer's packets before its next recv(), src/adsb.rs:95-116). */
int adsb_feed_ready(adsb_feed *feed);
void adsb_feed_close(adsb_feed *feed);

/*
 * On-device field decode of the last launch's frame list: what AdsbPacket::new
 * computes per frame (src/adsb/packet.rs:25-49, src/adsb/msgs.rs:70-102,150-201), as one 32-byte
 * record per frame, in frame order.  Lets the host wrapper only wrap when output volumes are large.
 */
typedef struct adsb_packet_fields {
    uint32_t icao;                /* packet.rs:28 */
    int32_t  altitude;            /* AircraftPosition (msgs.rs:70-75), feet; 0 otherwise */
    uint32_t cpr_latitude;        /* msgs.rs:84-86 */
    uint32_t cpr_longitude;       /* msgs.rs:87-89 */
    uint8_t  downlink_format;     /* packet.rs:26 */
    uint8_t  capability;          /* packet.rs:27 (mask 5, as in the reference) */
    uint8_t  msg_type;            /* packet.rs:29 */
    uint8_t  msg_kind;            /* 0 AircraftID, 1 AircraftPosition, 2 Uknown (msgs.rs:6-11) */
    uint8_t  surveillance_status; /* msgs.rs:78 */
    uint8_t  nic_supplement;      /* msgs.rs:79 */
    uint8_t  cpr_time;            /* msgs.rs:80 */
    uint8_t  cpr_odd;             /* msgs.rs:81-82: 1 = CprFormat::Odd */
    char     callsign[8];         /* AircraftID (msgs.rs:180-201), not NUL terminated; zeros otherwise */
} adsb_packet_fields;
/* Enqueues the decode after the last launch (ctx stream); needs cfg.max_out records of ctx memory
 * (allocated on first use). */
int adsb_decode_fields_device_async(adsb_ctx *ctx);
/* Waits and copies the records to the host; *n_out = number of frames decoded. */
int adsb_fetch_fields(adsb_ctx *ctx, adsb_packet_fields *out, size_t max_out, size_t *n_out);
/* Device pointer to the records (valid until the next decode on this ctx); does not synchronise. */
int adsb_fields_device(adsb_ctx *ctx, const adsb_packet_fields **fields_dev);

/*
 * Per-frame signal and noise power.  The reference's gate is declared to return "high value, signal power, noise
 * power" (src/adsb/demod.rs:16-17), returns zeros for the two powers (demod.rs:56) and thread 2 drops them
 * (src/adsb.rs:103).  Here: exact integer statistics of the 240 samples a frame was decoded from, one 32-byte record
 * per frame, in frame order.  Sample power is p = I^2 + Q^2 on the stored integers (i8: at most 32768; i16: at most
 * 2^31, from (-32768, -32768)).  With w = offset - first_sample_index the frame's position in its buffer and bit b
 * (0..111) of bytes[] AS RETURNED (MSB first, after any repair), the 116 PULSE samples are w+0, w+2, w+7, w+9
 * (demod.rs:20-24) and, per bit, w+16+2b if the bit is 1, else w+16+2b+1; the other 124 are the QUIET samples.
 */
#define ADSB_LEVEL_VALID 0x1u
typedef struct adsb_frame_level {   /* 32 bytes */
    uint64_t signal_sum;   /* sum of p over the 116 pulse samples                         */
    uint64_t noise_sum;    /* sum of p over the 124 quiet samples                         */
    uint32_t peak;         /* max p over all 240                                          */
    uint32_t pulse_min;    /* min p over the pulse samples                                */
    uint32_t quiet_max;    /* max p over the quiet samples                                */
    uint16_t weak_bits;    /* bits whose pulse-sample p < 2 x their quiet-sample p (u64)  */
    uint16_t flags;        /* ADSB_LEVEL_VALID (| ADSB_LEVEL_SHORT, adsb_levels_modes_of); 0: window not inside the buffer, rest 0 */
} adsb_frame_level;
/* Enqueues the levels of the last launch's list behind its ordering pass (like adsb_decode_fields_device_async; the
 * count is read on the device, the host does not wait).  Reads the launch's input again: the buffer handed to
 * adsb_demod_device_async (every channel; adsb_set_stream_base and adsb_set_result_target are honoured) or
 * adsb_demod's copy of it must still be intact, which it is until the next call that launches.  Needs cfg.max_out
 * records of ctx memory, allocated on first use; a ctx that never calls it allocates nothing and launches exactly
 * the kernels it launched before.  ADSB_E_STATE before any launch.
 * NOT for feeds: while a feed is open the older launch's input may already be overwritten (two buffers in flight
 * over two staging slots), and the one-dispatch path is one dispatch on purpose.  A feed's consumer holds the host
 * buffer: adsb_host_frame_levels (adsb_host.h) gives the same records from it. */
int adsb_levels_device_async(adsb_ctx *ctx);
/* Waits and copies min(frames of the list, max_out) records; *n_out = how many.  If the wait found the list rebuilt
 * (ADSB_FLAG_INCOMPLETE, slot-pool overflow), the levels are computed again for the rebuilt list first.
 * ADSB_E_STATE if no levels were enqueued for the last launch. */
int adsb_fetch_levels(adsb_ctx *ctx, adsb_frame_level *out, size_t max_out, size_t *n_out);
/* Device pointer to the records (valid until the next levels call on this ctx); does not synchronise. */
int adsb_levels_device(adsb_ctx *ctx, const adsb_frame_level **levels_dev);
/* Any frame list against any ONE-channel device buffer of the ctx's sample type (iq_dev aligned to one sample):
 * frame i sits at sample frames[i].offset - first_sample_index.  `frames` is host memory or device memory of the
 * ctx's device, `out` host memory of n records; blocking.  A frame whose 240-sample window is not wholly inside
 * [0, n_samples) -- offset < first_sample_index included -- gets flags = 0 and zeros, and nothing of it is read.
 * Uses scratch of its own: the last launch's levels stay as they are.  ADSB_E_CAPACITY for n >= 2^32. */
int adsb_levels_of(adsb_ctx *ctx, const void *iq_dev, size_t n_samples, uint64_t first_sample_index,
                   const adsb_frame *frames, size_t n, adsb_frame_level *out);
/*
 * Level records by frame length: what adsb_replies_of and adsb_merge_lists_of produce -- 56-bit and 112-bit frames of
 * many channels in one list -- against the samples they came from.  A frame's length is that of its DF, bytes[0] >> 3:
 * below 16 it is a SHORT frame of 56 bits, anything else (DF16..31, DF24..31 included) a long one of 112.  This is the
 * rule adsb_modes_of and the replies scan use.
 *   A long frame's record is exactly adsb_levels_of's.
 *   A short frame's window is the 128 samples [w, w + 128).  Its 60 PULSE samples are w+0, w+2, w+7, w+9 and, per bit
 *   b = 0..55 of bytes[0..7), w+16+2b if the bit is 1, else w+16+2b+1; the other 68 are the QUIET samples.  The fields
 *   are the same: the two sums, peak over all 128, pulse_min, quiet_max, and weak_bits over the 56 bits.  flags =
 *   ADSB_LEVEL_VALID | ADSB_LEVEL_SHORT.  bytes[7..14) of a short frame are never read.
 *   A short frame is valid iff [w, w + 128) lies inside its channel, [0, n_samples): one at n_samples - 128 is valid, one
 *   at n_samples - 127 gets zeros and flags = 0 -- a short frame in the last 240 samples of a buffer, which the replies
 *   scan finds on purpose, has a record.  Nothing at or past w + 128 is addressed for a short frame, and nothing at or
 *   past its channel's end for any frame.
 * The list is in channel order: counts[c] (HOST memory, n_channels entries that add up to n) frames of channel c, whose
 * sample 0 is at iq_dev + c x channel_stride samples (channel_stride >= n_samples; ignored for one channel); frame i of
 * channel c sits at sample frames[i].offset - first_sample_index of it.  `frames` is host memory or device memory of the
 * ctx's device.  `out` is host memory of n records, or NULL to leave the records on the device only.  Blocking.  Uses
 * scratch of its own, grown on demand: the last launch's levels and adsb_levels_of's scratch stay as they are, and a ctx
 * that never calls it allocates nothing and launches exactly the kernels it launched before.  n = 0 is ADSB_OK, allocates
 * and launches nothing and leaves an earlier call's records as they are.  ADSB_E_ARG for a NULL
 * ctx, iq_dev or counts, NULL frames with n > 0, iq_dev not aligned to one sample, n_channels = 0 or above 2^20,
 * channel_stride < n_samples with more than one channel, or counts that do not add up to n; ADSB_E_CAPACITY for
 * n >= 2^32.
 */
#define ADSB_LEVEL_SHORT 0x2u /* adsb_frame_level.flags: a 56-bit frame's record, sums over 60 and 68 samples */
int adsb_levels_modes_of(adsb_ctx *ctx, const void *iq_dev, uint32_t n_channels, size_t n_samples, size_t channel_stride,
                         uint64_t first_sample_index, const adsb_frame *frames, const uint64_t *counts, size_t n,
                         adsb_frame_level *out /* NULL: device only */);
/* Device pointer to the records of the last adsb_levels_modes_of, valid until the next one: what adsb_wire_of,
 * adsb_correlate_of and a table's update take as a device level list.  ADSB_E_STATE before the first call with n > 0
 * that returned ADSB_OK, and after one that failed on its way (its records are not complete). */
int adsb_levels_modes_device(adsb_ctx *ctx, const adsb_frame_level **levels_dev);

/*
 * Wire output: a frame list as Beast binary or AVR text, the formats readsb / dump1090 network inputs, tar1090,
 * Virtual Radar Server, mlat-client and feeder clients speak, encoded on the device.
 *   TIMESTAMP  t = (6 x frame.offset + tick_bias) mod 2^48: the 12 MHz multilateration clock, six ticks per 2 MSPS
 *     sample.  frame.offset is absolute across launches and ranks once adsb_set_stream_base is used.  tick_bias = 0
 *     stamps the first preamble sample (dump1090's convention for long messages is the END of the message); the
 *     caller's constant is the only configuration, nothing else is inferred.
 *   SIGNAL BYTE  s = 0 with signal == 0, with a NULL level list, or for a level record without ADSB_LEVEL_VALID.
 *     Otherwise s = 255 x sqrt(signal_sum / (116 x FS)) rounded half up, clamped to 255 and raised to 1 when
 *     signal_sum > 0, with FS the full scale of adsb_level_dbfs (32768 for ADSB_SAMPLE_I8, 2^31 for ADSB_SAMPLE_I16).
 *     Computed exactly in integers: s is the largest s in 0..255 with (2s-1)^2 x 116 x FS <= 4 x 255^2 x signal_sum
 *     (every product fits uint64: the largest left side is 509^2 x 116 x 2^31, about 6.5e16).  No floating point:
 *     device, CPU mirror and any model agree to the bit.
 *   ADSB_WIRE_BEAST     1A 33, then 6 bytes of t big-endian, then s, then the 14 frame bytes; every 0x1A among those
 *                       21 bytes is written twice.  23..44 bytes.
 *   ADSB_WIRE_AVR       '*', 28 upper-case hex digits, ';', '\n'.  31 bytes.
 *   ADSB_WIRE_AVR_MLAT  '@', 12 upper-case hex digits of t, 28 hex digits, ';', '\n'.  43 bytes.  (The AVR forms carry
 *                       no signal byte: `signal` is ignored.)
 *   ADSB_WIRE_SHORT     a bit of `format`, OR-ed onto one of the three (adsb_wire_cfg has no spare field).  With it a
 *                       frame whose length is 7 by the rule of "Level records by frame length" (bytes[0] >> 3 below 16)
 *                       leaves as a short frame:
 *                         Beast     1A 32, 6 bytes of t, s, bytes[0..7); every 0x1A of those 14 bytes doubled.  16..30 bytes.
 *                         AVR       '*', 14 upper-case hex digits, ';', '\n'.  17 bytes.
 *                         AVR_MLAT  '@', 12 digits of t, 14 digits, ';', '\n'.  29 bytes.
 *                       bytes[7..14) are neither written nor looked at for escapes.  Long frames are written as without
 *                       the bit, and t is the same 6 x offset + tick_bias.  SIGNAL BYTE with the bit: a level record with
 *                       ADSB_LEVEL_SHORT is a sum over 60 pulse samples, so s is the largest s in 0..255 with (2s-1)^2 x
 *                       60 x FS <= 4 x 255^2 x signal_sum, raised to 1 for a sum above zero and clamped as above; a record
 *                       without that flag uses 116 whatever the frame's length (wire input's records have no SHORT flag
 *                       and are built with 116, so they keep encoding to the byte they came from).  Without the bit
 *                       every byte is what it was before the bit existed: 14 frame bytes, 116.  adsb_wire_in_of with
 *                       ADSB_WIRE_IN_SHORT reads such a stream back as the same list; its own `format` does not take
 *                       this bit.
 * The output is ONE contiguous byte stream in list order (channel 0's frames in ascending offset, then channel 1's,
 * ...) and uint32 ends[n]: the exclusive end offset of each frame's bytes, so ends[i-1] .. ends[i] is frame i (from 0
 * for frame 0) and ends[n-1] is the stream's length.  With adsb_fetch's per_channel_counts a consumer cuts the stream
 * per receiver without parsing it.  The stream is byte-identical from run to run.
 */
#define ADSB_WIRE_BEAST 0u
#define ADSB_WIRE_AVR 1u
#define ADSB_WIRE_AVR_MLAT 2u
#define ADSB_WIRE_SHORT 0x100u /* a bit of adsb_wire_cfg.format: 56-bit frames leave as short frames */
#define ADSB_WIRE_MAX_BYTES 44 /* the longest encoded frame */
typedef struct adsb_wire_cfg {
    uint32_t format;     /* ADSB_WIRE_BEAST, _AVR or _AVR_MLAT, | ADSB_WIRE_SHORT     */
    uint32_t signal;     /* != 0: the Beast signal byte from the frames' level records */
    uint64_t tick_bias;  /* < 2^48                                                     */
} adsb_wire_cfg;
/* Enqueues the encoding of the last launch's list behind its ordering pass (three small dispatches; the count is read
 * on the device, the host does not wait).  A second call on the same launch replaces the first's output.  With
 * signal != 0 (Beast) and no levels enqueued for this launch it enqueues adsb_levels_device_async itself first, so
 * that call's conditions hold: like it, NOT for use while a feed is open when signal != 0 (a feed's consumer encodes
 * the popped frames with adsb_host_wire_encode, adsb_host.h).  Buffers are allocated on first use: 44 x cfg.max_out
 * bytes, cfg.max_out ends, one word per 256 frames; a ctx that never calls it allocates nothing and launches exactly
 * the kernels it launched before.  ADSB_E_ARG for a NULL ctx or cfg, an unknown format or tick_bias >= 2^48;
 * ADSB_E_STATE before any launch; ADSB_E_CAPACITY when 44 x cfg.max_out does not fit uint32. */
int adsb_wire_device_async(adsb_ctx *ctx, const adsb_wire_cfg *cfg);
/* Waits.  If the wait found the list rebuilt (ADSB_FLAG_INCOMPLETE, slot-pool overflow), the stream is encoded again
 * for the rebuilt list first, as adsb_fetch_levels does.  *n_bytes = the stream's length and *n_frames = the frames in
 * it, whatever the capacities.  `out` receives the whole stream if cap holds it, else whole frames only: the longest
 * prefix of frames that fits.  `ends` (may be NULL with max_ends 0) receives min(*n_frames, max_ends) entries.
 * ADSB_E_STATE if no wire output was enqueued for the last launch. */
int adsb_fetch_wire(adsb_ctx *ctx, uint8_t *out, size_t cap, size_t *n_bytes, uint32_t *ends, size_t max_ends,
                    size_t *n_frames);
/* For device-side consumers; does not synchronise.  The stream, ends[] and the stream's header
 * { uint64 n_bytes; uint64 n_frames } in device memory (each optional), valid until the next wire call on this ctx
 * and ordered like adsb_levels_device's records.  ADSB_E_STATE before the first adsb_wire_device_async. */
int adsb_wire_device(adsb_ctx *ctx, const uint8_t **bytes_dev, const uint32_t **ends_dev, const void **header_dev);
/* Any frame list with any level list (levels NULL: s = 0), each in host memory or in device memory of the ctx's
 * device; frames no demodulator would emit are encoded like any other.  Blocking.  out / cap / *n_bytes as
 * adsb_fetch_wire; ends (host, may be NULL) receives all n entries.  Uses scratch of its own: the last launch's wire
 * output stays as it is.  ADSB_E_CAPACITY when 44 x n does not fit uint32. */
int adsb_wire_of(adsb_ctx *ctx, const adsb_wire_cfg *cfg, const adsb_frame *frames,
                 const adsb_frame_level *levels /* NULL: s = 0 */, size_t n, uint8_t *out, size_t cap, size_t *n_bytes,
                 uint32_t *ends);
/* Frames per workgroup of the encoder's kernels and threads of its totals scan (either may be NULL): the sizes at
 * which the encoder takes another path, for tests.  The stream does not depend on them. */
int adsb_debug_wire_geometry(uint32_t *frames_per_block, uint32_t *scan_threads);

/*
 * Wire input: the inverse of the wire output.  One or many byte streams of Beast binary or AVR text, as distributed
 * receivers (readsb, dump1090, Beast splitters, mlat-client) send them over TCP, parsed on the device into the ordered
 * adsb_frame[] every consumer behind the demodulator takes, with per-frame receive records, optional level records and
 * per-stream counts[] that drop straight into adsb_correlate_of, adsb_track_bank_update(_levels) and adsb_wire_of.
 *   INPUT  bytes[n_bytes] is R streams laid end to end, 1 <= R <= 256; stream_ends[R] holds ascending exclusive ends,
 *     the last equal to n_bytes; n_bytes < 2^32.  Streams are parsed independently: a stream's first byte has no
 *     predecessor, and nothing reads past a stream's end.  Below, B[0..N) is one stream.
 *   BEAST (ADSB_WIRE_BEAST)
 *     MARKS  Take every maximal run of 0x1A bytes B[a..b) that is followed by a byte inside the stream (b < N).  If its
 *       length b - a is odd, its last byte b-1 is a MARK and B[b] is the mark's type byte.  Even runs hold no mark.  A run
 *       that reaches the end of the stream holds no mark.
 *     LENGTHS  Types '1', '2' and '3' carry 2, 7 and 14 message bytes after 6 timestamp bytes and 1 signal byte.  Any
 *       other type byte makes the mark UNKNOWN: it is counted and nothing is read for it.
 *     READING a known mark starts at b+1 and un-escapes 7 + len bytes.  A byte other than 0x1A is taken as is.  1A 1A
 *       yields one 0x1A.  A 0x1A whose next byte exists and is not 0x1A means the frame is CUT; that byte is itself a
 *       mark by the parity rule.  Needing a byte at or past N, including the partner of a final 0x1A, means the frame is
 *       INCOMPLETE.  Otherwise the frame is COMPLETE.
 *     Complete '3' frames that pass the filters are emitted.  Complete '1' and '2' frames are counted (n_other) and not
 *       emitted ('2' frames are emitted with ADSB_WIRE_IN_SHORT, see SHORT FRAMES).  Complete frames never overlap.
 *       Only the last mark of a stream can be incomplete.
 *     CONSUMED  If the stream has an incomplete mark at m, consumed = m.  Otherwise let k be the number of trailing 0x1A
 *       bytes of the stream that no complete frame consumed, and consumed = N - (k mod 2).
 *     CHUNKS  The caller's next chunk is B[consumed..) + new bytes.  Parsing a stream in chunks of any sizes this way
 *       yields exactly the frames of parsing it whole, at the same absolute positions.  The carried tail is never
 *       longer than 43 bytes.
 *   AVR (ADSB_WIRE_AVR accepts both the '*' and the '@' form; ADSB_WIRE_AVR_MLAT is the same value set)
 *     A candidate is any B[p] in {'*', '@'}; h is the number of consecutive hex digits after it, in either case,
 *     counted up to 41.  If the byte after the digits is ';': '*' with h = 28 is a long frame; '@' with h = 40 is a long
 *     frame with a 12-digit timestamp; '*' with 4 or 14 digits and '@' with 16 or 26 digits are counted as n_other;
 *     anything else is cut.  If the digits reach the end of the stream with h at most 28 for '*' or at most 40 for '@',
 *     the candidate is incomplete and consumed = p.  Otherwise consumed = N.  Bytes between frames ('\n', '\r\n',
 *     anything) are skipped.
 *   SHORT FRAMES  With ADSB_WIRE_IN_SHORT in cfg.filter the complete 56-bit frames -- Beast '2', '*' with 14 digits,
 *     '@' with 26 digits (a 12-digit timestamp first) -- are emitted like long frames: bytes[0..7) = the message,
 *     bytes[7..14) = 0, status = 0, fixed_bit = 0xFF, offset from the timestamp as for long frames, rx.kind '2', '*' or
 *     '@', the level record from the signal byte as for '3'.  n_other then counts Mode A/C only ('1'; 4 / 16 digits).
 *     These are the Mode S replies of transponders without ADS-B (DF0/4/5/11); adsb_modes_of ("Mode S replies") gives
 *     each its address.  Framing, consumed[] and the chunk rule do not depend on what is emitted.  Without the bit
 *     every output is what it was before the bit existed.
 *   OUTPUTS, all in stream order: receiver 0's frames by position, then receiver 1's, and so on.
 *     adsb_frame frames[n]: bytes = the 14 message bytes, status = 0, fixed_bit = 0xFF, offset = ((t - tick_bias) mod
 *       2^48) / 6 rounded down, the exact inverse of the encoder's timestamp for offsets below 2^48 / 6.  Plain '*'
 *       lines have t = 0.
 *     adsb_wire_rx rx[n]: the raw t, the position of the mark or lead byte inside its own stream, the signal byte, the
 *       kind ('3', '*' or '@'; '2' for a short Beast frame) and the receiver (the stream's index).
 *     adsb_frame_level levels[n] when cfg.levels != 0.  For a signal byte s > 0: flags = ADSB_LEVEL_VALID and signal_sum
 *       = the smallest sum whose signal byte is s for cfg.sample_type's full scale, ceil((2s-1)^2 x 116 x FS /
 *       (4 x 255^2)), and 1 for s = 1; every other field 0.  For s = 0 or AVR: an all-zero record.  With this,
 *       adsb_wire_of(parse(x)) reproduces x's signal bytes, and correlate's best_receiver works on network input.
 *     uint64 counts[R] (frames of each stream in the list) and uint64 consumed[R] (per stream, relative to its start).
 *     adsb_wire_in_header: n_frames (in the list), total_found, n_marks (AVR: candidates), n_cut, n_unknown, n_other,
 *       n_rejected, flags.
 *   FILTERS (cfg.filter bits).  A rejected frame is still a complete frame for framing and for consumed; it is counted
 *     in n_rejected and not emitted.  ADSB_WIRE_IN_CRC keeps a long frame only if crc24(bytes[0..11]) ^ bytes[11..14]
 *     == 0 (generator 0x1FFF409; no repair, a Beast sender has already done its own).  ADSB_WIRE_IN_DF17 keeps it only
 *     if bytes[0] >> 3 == 17.  The filters are literal on short frames too: ADSB_WIRE_IN_DF17 rejects every short frame,
 *     and ADSB_WIRE_IN_CRC keeps one only if crc24(bytes[0..4)) ^ bytes[4..7) == 0.  The address/parity formats
 *     (DF0/4/5/16/20/21: the address is overlaid on the parity field) therefore NEVER pass the CRC filter, short or
 *     long; adsb_modes_of is the check for them.
 *   CAPACITY  cfg.max_frames = 0 means n_bytes / 23 (n_bytes / 16 with ADSB_WIRE_IN_SHORT: the shortest emitted frame
 *     in both formats), which can never truncate.  Otherwise the first max_frames frames
 *     in order are kept, flags has ADSB_FLAG_TRUNCATED, counts[] are clipped to the list and total_found is the full
 *     number.
 * Nothing depends on atomics or scheduling: two runs give the same bytes.
 */
#define ADSB_WIRE_IN_CRC 0x1u
#define ADSB_WIRE_IN_DF17 0x2u
#define ADSB_WIRE_IN_SHORT 0x4u
typedef struct adsb_wire_in_cfg {
    uint32_t format;      /* ADSB_WIRE_*                                                       */
    uint32_t filter;      /* ADSB_WIRE_IN_* bits                                               */
    uint64_t tick_bias;   /* < 2^48                                                            */
    uint64_t max_frames;  /* 0: n_bytes / 23 (/ 16 with ADSB_WIRE_IN_SHORT)                    */
    int32_t  sample_type; /* ADSB_SAMPLE_*: the full scale of the level records (with levels) */
    uint32_t levels;      /* != 0: level records beside the frames                             */
} adsb_wire_in_cfg;
typedef struct adsb_wire_rx {      /* 16 bytes */
    uint64_t ticks;           /* the raw timestamp t; 0 for a plain '*' line                  */
    uint32_t pos;             /* position of the mark or lead byte inside its own stream      */
    uint8_t  signal;          /* Beast's signal byte; 0 for AVR                               */
    uint8_t  kind;            /* '3', '*' or '@'; '2' for a short Beast frame                 */
    uint16_t receiver;        /* the stream's index                                           */
} adsb_wire_rx;
typedef struct adsb_wire_in_header { /* 64 bytes */
    uint64_t n_frames, total_found, n_marks, n_cut, n_unknown, n_other, n_rejected, flags;
} adsb_wire_in_header;
/* Parses.  `bytes` is host memory or device memory of the ctx's device; stream_ends is host memory.  Asynchronous on the
 * ctx's stream once host arrays are copied.  Buffers are allocated on first use and grown when needed (may wait for
 * earlier work): per input byte about 0.01 bytes of scan words, per frame of capacity 40 bytes (72 with levels; the
 * capacity max_frames = 0 stands for is n_bytes / 16 frames with ADSB_WIRE_IN_SHORT instead of n_bytes / 23), and a
 * copy of a host input; a ctx that never calls it allocates nothing and launches exactly the kernels it launched before.
 * Replaces the result of an earlier call.  n_bytes = 0 and empty streams are ADSB_OK.  ADSB_E_ARG for a NULL ctx, cfg or
 * stream_ends, NULL bytes with n_bytes > 0, an unknown format, tick_bias >= 2^48, a bad sample_type with levels,
 * n_streams outside 1..256, or ends that are not ascending or do not end at n_bytes; ADSB_E_CAPACITY for n_bytes >= 2^32. */
int adsb_wire_in_of(adsb_ctx *ctx, const adsb_wire_in_cfg *cfg, const uint8_t *bytes, size_t n_bytes,
                    const uint64_t *stream_ends, uint32_t n_streams);
/* Waits and copies; each output may be NULL.  frames, rx and levels receive min(header.n_frames, max) entries and *n
 * that number; counts and consumed receive n_streams entries each (at most the parsed call's); *header the totals,
 * whatever the capacities.  ADSB_E_STATE before any adsb_wire_in_of, or for levels when that call had cfg.levels == 0;
 * ADSB_E_ARG for a NULL ctx or n_streams above the parsed call's. */
int adsb_fetch_wire_in(adsb_ctx *ctx, adsb_frame *frames, adsb_wire_rx *rx, adsb_frame_level *levels, size_t max,
                       size_t *n, uint64_t *counts, uint64_t *consumed, uint32_t n_streams, adsb_wire_in_header *header);
/* For device-side consumers; does not synchronise.  The arrays of the last adsb_wire_in_of in device memory (each
 * optional; *levels_dev is NULL when that call had cfg.levels == 0), valid until the next wire-input call on this ctx
 * and ordered on the ctx's stream behind it.  ADSB_E_STATE before any adsb_wire_in_of. */
int adsb_wire_in_device(adsb_ctx *ctx, const adsb_frame **frames_dev, const adsb_wire_rx **rx_dev,
                        const adsb_frame_level **levels_dev, const uint64_t **counts_dev, const uint64_t **consumed_dev,
                        const void **header_dev);
/* Bytes per workgroup span of the parser's kernels and threads of its one-workgroup scans (either may be NULL): the
 * sizes at which the parser takes another path, for tests.  The result does not depend on them. */
int adsb_debug_wire_in_geometry(uint32_t *bytes_per_block, uint32_t *scan_threads);

/*
 * Correlate: a multi-receiver frame list as ONE de-duplicated, time-ordered message list, with every message's
 * receptions (receiver and sample time) -- what an aggregator forwards once, what one track table pairs across
 * receivers, and what a multilateration solver takes as input.  Stateless; computed on the device.
 *   INPUT  frames[n] in adsb_fetch's layout: receiver 0's frames in ascending offset, then receiver 1's, ...;
 *     counts[R] summing to n, 1 <= R <= 256; sample_base[R] (NULL: all 0); optionally levels[n], the frames'
 *     adsb_frame_level records; window, in samples.  n < 2^32.  The layout is an input contract, as for
 *     adsb_track_bank_update: the result for an unordered list is defined by the same rules, not checked.
 *   RECEPTION j is list index j, heard by receiver r(j).  Its time T_j = sample_base[r] + frames[j].offset (uint64
 *     arithmetic mod 2^64; the caller keeps it from wrapping); its key K_j = the 14 frame bytes as one big-endian
 *     112-bit integer, all 112 bits taking part.
 *   GROUP ORDER  receptions ordered by (K, T, j), ascending, all unsigned.
 *   HEADS  a reception starts a new group when it is first in group order, or its K differs from its predecessor's, or
 *     T - T_pred > window.  A chain rule: a group is a maximal run of equal bytes whose consecutive gaps are all
 *     <= window (window = 0: only equal times group).  Two receptions of ONE receiver that decodes the same bytes at
 *     two nearby offsets are both in the group, which is why n_receivers and n_receptions are separate fields.
 *   MESSAGE  one per group; its time is the T of the group's first reception.  Messages are listed in ascending
 *     (time, K), a pair that is unique per group (two groups with equal K and equal time would have chained).
 *     Bytes 0..23 of an adsb_message are an adsb_frame with offset = time; the same 24 bytes are also written
 *     contiguously as adsb_frame frames_out[n_messages]: ascending offset, ties in ascending bytes, a valid argument
 *     for adsb_track_table_update(..., sample_base = 0), adsb_wire_of and adsb_levels_of.
 *   RECEPTIONS  receptions[n], message by message in message order and in (T, j) order inside a message: message m owns
 *     receptions[first .. first + n_receptions).
 * Nothing depends on atomics, hash placement or scheduling: two runs give the same bytes.
 */
typedef struct adsb_message {      /* 64 bytes */
    uint64_t time;            /* earliest reception's T                                               */
    uint8_t  bytes[14];       /* the key                                                              */
    uint8_t  status;          /* least status over the receptions                                     */
    uint8_t  fixed_bit;       /* fixed_bit of the first reception in group order with that status     */
    uint32_t first;           /* index of its first entry in receptions[]                             */
    uint32_t n_receptions;
    uint16_t n_receivers;     /* distinct receivers in the group                                      */
    uint16_t first_receiver;  /* receiver of the earliest reception (ties: lowest list index)         */
    uint16_t best_receiver;   /* receiver of the reception with the greatest signal_sum among those whose level
                                 has ADSB_LEVEL_VALID (ties: earliest in group order); 0xFFFF if none or no levels */
    uint16_t reserved;        /* 0 */
    uint32_t n_clean;         /* receptions with status == 0                                          */
    uint32_t reserved2;       /* 0 */
    uint64_t span;            /* latest T minus earliest T of the group                               */
    uint64_t best_signal_sum; /* 0 if best_receiver is 0xFFFF                                         */
} adsb_message;
typedef struct adsb_reception {    /* 16 bytes */
    uint64_t time;            /* T */
    uint32_t frame;           /* the index j in the input list */
    uint16_t receiver;
    uint16_t reserved;        /* 0 */
} adsb_reception;
typedef struct adsb_correlate_cfg {
    uint32_t window;          /* samples */
    uint32_t use_levels;      /* adsb_correlate_launch: != 0 takes the launch's levels; ignored by adsb_correlate_of */
    uint64_t reserved;
} adsb_correlate_cfg;
/* The ctx's last launch, channel k -> receiver k: the same header sync and slot-pool repair as adsb_fetch_counts (it
 * waits for the launch), then the correlate sequence enqueued on the ctx's stream.  use_levels != 0 takes the ctx's
 * levels of that launch, enqueuing adsb_levels_device_async if they are not there (and again for a rebuilt list), as
 * adsb_track_bank_update_launch_levels does; that call's conditions then hold.  sample_base[n_channels] or NULL.
 * Buffers are allocated on first use, sized by cfg.max_out: 224 bytes per frame (64 + 24 + 16 of results, 72 of group
 * aggregate, 48 of times, key words and orders) plus the sorts' temporary storage (about 16 more per frame); a ctx
 * that never calls it allocates nothing and launches exactly the kernels it launched before.  ADSB_E_ARG for a NULL ctx or cfg or a
 * launch with more than 256 channels; ADSB_E_STATE before any launch. */
int adsb_correlate_launch(adsb_ctx *ctx, const adsb_correlate_cfg *cfg, const uint64_t *sample_base);
/* Any list: frames / levels (NULL allowed) each in host memory or in device memory of the ctx's device; counts and
 * sample_base (NULL allowed) host memory.  Asynchronous on the ctx's stream once the host arrays are copied.  Grows the
 * buffers when n exceeds them (may wait for earlier work), and replaces the result of an earlier correlate call.
 * ADSB_E_ARG for a NULL ctx or cfg, n_receivers outside 1..256, NULL counts, counts not summing to n, or NULL frames
 * with n > 0; ADSB_E_CAPACITY for n >= 2^32.  n = 0 is ADSB_OK with empty results. */
int adsb_correlate_of(adsb_ctx *ctx, const adsb_correlate_cfg *cfg, const adsb_frame *frames,
                      const adsb_frame_level *levels, size_t n, const uint64_t *counts, uint32_t n_receivers,
                      const uint64_t *sample_base);
/* Waits.  *n_msgs / *n_recs (each may be NULL) are the totals, whatever the capacities; msgs receives
 * min(*n_msgs, max_msgs) messages and recs min(*n_recs, max_recs) receptions (NULL allowed with capacity 0).
 * ADSB_E_STATE before any correlate call. */
int adsb_fetch_correlated(adsb_ctx *ctx, adsb_message *msgs, size_t max_msgs, size_t *n_msgs, adsb_reception *recs,
                          size_t max_recs, size_t *n_recs);
/* For device-side consumers; does not synchronise.  messages[], frames_out[], receptions[] and the header
 * { uint64 n_messages; uint64 n_receptions } in device memory (each optional), valid until the next correlate call on
 * this ctx and ordered on the ctx's stream behind it.  ADSB_E_STATE before any correlate call. */
int adsb_correlated_device(adsb_ctx *ctx, const adsb_message **msgs_dev, const adsb_frame **frames_dev,
                           const adsb_reception **recs_dev, const void **header_dev);
/* Threads (= receptions) per workgroup of the correlate kernels: the size at which they take another path, for tests.
 * The result does not depend on it. */
int adsb_debug_correlate_geometry(uint32_t *threads_per_block);

/*
 * Mode S replies: the address of every frame of a list, and the surveillance fields of the replies a transponder
 * without ADS-B sends (DF11 all-call, DF4/5/20/21 surveillance and Comm-B, DF0/16 air-air).  Everything else in this
 * library reads the address as bytes[1..3]; that holds for DF11/17/18 only.  The other formats overlay the address on
 * the parity field, so it is recovered as crc24(payload) ^ parity and can be trusted only if the aircraft is already
 * known.  Stateless; computed on the device; the list is in adsb_fetch's layout and may be wire input's output (with
 * ADSB_WIRE_IN_SHORT), correlate's frames_out or the demodulator's own list.  correlate -> clock sync -> multilaterate
 * then place these frames unchanged (the solver does not look at the DF).
 *   PER FRAME  b = frame.bytes, DF = b[0] >> 3, length 7 bytes for DF < 16 and 14 otherwise (bytes past the length are
 *     ignored), S = crc24(b[0..len-3)) ^ b[len-3..len), generator 0x1FFF409.
 *   KIND and ADDRESS
 *     DF17, DF18: S == 0 -> SELF, address b[1..3]; else PARITY (address 0).
 *     DF11: S == 0 -> SELF, address b[1..3].  S != 0 with S & 0xFFFF80 == 0 (a reply to interrogator iid = S & 0x7F):
 *       address b[1..3], KNOWN if that address is known (below), else UNKNOWN.  Otherwise PARITY.
 *     DF0, 4, 5, 16, 20, 21, 24..31: address S, KNOWN if known, else UNKNOWN.
 *     Every other DF: UNSUPPORTED, address and all fields 0 (df is still the frame's).
 *   KNOWN (causal, in list order)  Address a is known at list index j iff a is in known_in[], or some frame i < j of
 *     this list is SELF with address a.  known_in[n_known_in] is ascending, unique and < 2^24, host or device memory
 *     (a host array that breaks this is ADSB_E_ARG; for a device array it is an unchecked input contract, as the list
 *     layout is for correlate).  known_out[] = the ascending unique union of known_in and the list's SELF addresses.
 *     So modes(L1, K) followed by modes(L2, known_out1) gives exactly the records of modes(L1 + L2, K) and the same
 *     final known_out: a feed carries known_out from call to call.  Nothing expires here; the caller prunes, for
 *     example by rebuilding known_in from a track table's ICAOs after its expire.  A garbage frame of an address/parity
 *     format is accepted as KNOWN with probability |known| / 2^24 (4096 known aircraft: 1 in 4096); consumers that
 *     cannot bear that ask for two agreeing frames.
 *   FIELDS are decoded whatever the kind, so consumers look at kind.  f = (b[2] & 0x1F) << 8 | b[3], bits 12..0 =
 *     C1 A1 C2 A2 C4 A4 M B1 Q B2 D2 B4 D4 (M and Q in the AC field; 0 and D1 in the ID field).
 *     DF4/5/20/21: fs = b[0] & 7, dr = b[1] >> 3, um = (b[1] & 7) << 3 | b[2] >> 5; GROUND for fs 1, 3; ALERT for fs
 *       2, 3, 4; SPI for fs 4, 5.  DF0/16: GROUND for vs = b[0] >> 2 & 1, ri = (b[1] & 7) << 1 | b[2] >> 7.
 *       DF11/17/18: ca = b[0] & 7; iid as above (DF11), else 0.
 *     ALTITUDE (DF0/4/16/20, f = AC): f == 0: none.  M = 1: none, ALT_METRIC.  Q = 1: n = (f & 0x1F80) >> 2 |
 *       (f & 0x20) >> 1 | (f & 0xF), altitude_ft = 25 n - 1000, ALT.  Q = 0, Gillham: h = binary of the Gray code D2 D4
 *       A1 A2 A4 B1 B2 B4, c = binary of the Gray code C1 C2 C4 with 5 and 7 exchanged; c == 0 or c > 5: none; h odd:
 *       c = 6 - c; altitude_ft = 500 h + 100 c - 1300, ALT.  1280 valid codes, -1200 .. 126700 ft.
 *     SQUAWK (DF5/21, f = ID): digits A = A4 A2 A1, B, C, D likewise; squawk = 1000 A + 100 B + 10 C + D, so 7700 reads
 *       7700; SQUAWK.
 *     CALLSIGN (DF20/21 with b[4] == 0x20, BDS 2,0): callsign[8] = the eight 6-bit characters of b[5..11) in the ICAO
 *       set as the field decode spells it ('_' for space, '#' for none); CALLSIGN only if every character is a letter,
 *       a digit or the space.  Otherwise callsign is 0.
 *   OUTPUTS  adsb_modes_rec recs[n], index for index with the list; uint32 known_out[n_known_out]; adsb_frame
 *     squitters[n_squitters]: the SELF frames with DF 17 or 18 in list order, the sub-list that is safe to hand to
 *     adsb_track_table_update / adsb_track_bank_update, which key on bytes[1..3]; uint64 squitter_counts[R] (squitters
 *     of each receiver) when the call had counts[R]; the adsb_modes_header.
 * Nothing depends on atomics or scheduling: two runs give the same bytes.
 */
#define ADSB_MODES_SELF 0u        /* the frame checks itself (S == 0): address from bytes[1..3] */
#define ADSB_MODES_KNOWN 1u       /* the address (from the parity, or DF11's with an iid) is a known aircraft's */
#define ADSB_MODES_UNKNOWN 2u     /* ... is not: a new aircraft, or garbage */
#define ADSB_MODES_PARITY 3u      /* a self-checking format whose parity fails */
#define ADSB_MODES_UNSUPPORTED 4u /* a DF this stage does not read */
#define ADSB_MODES_ALT 0x1u
#define ADSB_MODES_ALT_METRIC 0x2u
#define ADSB_MODES_SQUAWK 0x4u
#define ADSB_MODES_GROUND 0x8u
#define ADSB_MODES_ALERT 0x10u
#define ADSB_MODES_SPI 0x20u
#define ADSB_MODES_CALLSIGN 0x40u
typedef struct adsb_modes_rec {    /* 32 bytes */
    uint32_t address;         /* 24 bits; 0 for PARITY and UNSUPPORTED                                 */
    uint8_t  df;
    uint8_t  kind;            /* ADSB_MODES_SELF ...                                                   */
    uint16_t flags;           /* ADSB_MODES_ALT ...                                                    */
    int32_t  altitude_ft;     /* with ADSB_MODES_ALT                                                   */
    uint16_t squawk;          /* with ADSB_MODES_SQUAWK                                                */
    uint8_t  fs, dr, um, iid, ca, ri;
    char     callsign[8];     /* DF20/21 with BDS 2,0; trust it with ADSB_MODES_CALLSIGN               */
    uint8_t  reserved[4];     /* 0 */
} adsb_modes_rec;
typedef struct adsb_modes_header { /* 64 bytes */
    uint64_t n, n_self, n_known, n_unknown, n_parity, n_unsupported, n_known_out, n_squitters;
} adsb_modes_header;
#ifdef __cplusplus
static_assert(sizeof(adsb_modes_rec) == 32 && sizeof(adsb_modes_header) == 64, "adsb_modes_rec / adsb_modes_header layout");
#endif
/* Resolves.  frames[n] and known_in[n_known_in] each in host memory or in device memory of the ctx's device; counts
 * host memory, or NULL (then n_receivers is ignored and there are no squitter_counts).  n comes from the host, as for
 * the other _of calls.  Asynchronous on the ctx's stream once the host arrays are copied.  Buffers are allocated on first
 * use and grown when needed (may wait for earlier work): per frame 56 bytes of results, and per frame and known address
 * 36 bytes of sort entries, scan words and known_out plus the sort's temporary storage; a ctx that never calls it
 * allocates nothing and launches exactly the kernels it launched before.  Replaces the result of an earlier call.
 * n = 0 is ADSB_OK: known_out = known_in.  ADSB_E_ARG for a NULL ctx, NULL frames with n > 0, NULL known_in with
 * n_known_in > 0, n_known_in > 2^24, a host known_in that is not ascending, unique and < 2^24, or counts with
 * n_receivers outside 1..256 or not summing to n; ADSB_E_CAPACITY for n + n_known_in >= 2^32. */
int adsb_modes_of(adsb_ctx *ctx, const adsb_frame *frames, size_t n, const uint64_t *counts, uint32_t n_receivers,
                  const uint32_t *known_in, size_t n_known_in);
/* Waits and copies; each output may be NULL (with capacity 0).  recs receives min(header.n, max_recs) records, known_out
 * min(header.n_known_out, max_known) addresses, squitters min(header.n_squitters, max_squitters) frames,
 * squitter_counts n_receivers entries (at most the call's); *header the totals, whatever the capacities.
 * ADSB_E_STATE before any adsb_modes_of; ADSB_E_ARG for a NULL ctx, a NULL array with a capacity, or n_receivers above
 * the call's. */
int adsb_fetch_modes(adsb_ctx *ctx, adsb_modes_rec *recs, size_t max_recs, uint32_t *known_out, size_t max_known,
                     adsb_frame *squitters, size_t max_squitters, uint64_t *squitter_counts, uint32_t n_receivers,
                     adsb_modes_header *header);
/* For device-side consumers; does not synchronise.  The arrays of the last adsb_modes_of in device memory (each
 * optional; *squitter_counts_dev is NULL when that call had no counts), valid until the next call and ordered on the
 * ctx's stream behind it: known_out_dev is a valid known_in for the next call.  ADSB_E_STATE before any adsb_modes_of. */
int adsb_modes_device(adsb_ctx *ctx, const adsb_modes_rec **recs_dev, const uint32_t **known_out_dev,
                      const adsb_frame **squitters_dev, const uint64_t **squitter_counts_dev, const void **header_dev);
/* Threads (= frames) per workgroup of the stage's kernels: the size at which they take another path, for tests.  The
 * result does not depend on it. */
int adsb_debug_modes_geometry(uint32_t *threads_per_block);

/*
 * Comm-B registers: which transponder register the 56-bit MB field of a DF20/21 reply carries, and its values.  A
 * reply does not say which register it answers with; the interrogation did, and a receiver has not heard that.  So the
 * register is inferred from the 56 bits alone: status bits that contradict their fields, reserved bits, and values
 * outside what an aircraft can do.  Stateless, per frame, integers only; computed on the device; the list is in
 * adsb_fetch's layout, as for adsb_modes_of.
 *   BIT NUMBERING  For a frame with DF = bytes[0] >> 3 equal to 20 or 21, MB is bytes[4..11).  Bit 1 is the top bit of
 *     bytes[4], bit 56 the low bit of bytes[10].  u(a, n) is the n bits from bit a, as an unsigned number.  s(a, n) is a
 *     sign bit at a followed by n bits, two's complement: u(a+1, n) - (bit a ? 2^n : 0).  The "status rule (a; n)"
 *     reads: if bit a is 0, then u(a, n+1) == 0.
 *   STATE
 *     NOT_COMMB  DF is not 20 or 21.  Every other field of the record is 0.
 *     EMPTY      MB is all zero.
 *     NONE       No candidate register passes.
 *     ONE        Exactly one candidate passes.  bds is its code, and the values are decoded from it.
 *     AMBIGUOUS  Two or more candidates pass.  bds is 0 and the values are 0.
 *     candidates and n_candidates are filled for NONE, ONE and AMBIGUOUS alike.  The stage decides whatever the frame's
 *     parity says and does not know the address: consumers pair the record with adsb_modes_rec.kind, index for index.
 *   CANDIDATES  One bit each in candidates, in this order:
 *     1,0  u(1,8) == 0x10; u(10,5) == 0; with ovc = u(15,1) and ver = u(17,7), either ovc == 1 && ver >= 5 or
 *          ovc == 0 && ver <= 4.
 *     1,7  u(29,28) == 0 and bit 7 is set (a transponder that answers Comm-B has BDS 2,0).
 *     2,0  u(1,8) == 0x20 and each of the eight characters u(9 + 6k, 6) is a letter, a digit or the space (the rule
 *          of ADSB_MODES_CALLSIGN).
 *     3,0  u(1,8) == 0x30; u(29,2) != 3; u(16,7) < 48.
 *     4,0  status rules (1;12), (14;12), (27;12); u(40,8) == 0; u(52,2) == 0.
 *     5,0  status rules (1;10), (12;11), (24;10), (35;10), (46;10), and the limits: with bit 1, |s(2,9)| <= 284 (roll
 *          is at most 50 degrees); with bit 24, u(25,10) <= 300 (ground speed is at most 600 kt); with bit 46,
 *          u(47,10) <= 250 (true airspeed is at most 500 kt); with bits 24 and 46, |u(47,10) - u(25,10)| <= 100 (the
 *          two speeds differ by at most 200 kt).
 *     6,0  status rules (1;11), (13;10), (24;10), (35;10), (46;10), and the limits: with bit 13, u(14,10) <= 500;
 *          with bit 24, u(25,10) <= 250 (Mach is at most 1.0); with bit 35, |s(36,9)| <= 187; with bit 46,
 *          |s(47,9)| <= 187 (vertical rates are at most 6000 ft/min).
 *     The limits are written as integers on the raw fields, so device, mirror and model cannot disagree at a boundary.
 *   VALUES (state ONE)  value[0..5) are int32, bit k of status says that value[k] holds a value (it is 0 otherwise),
 *     word is a uint32.  All are integers; the Python interface converts to physical units.
 *     4,0  value[0] = 16 u(2,12): MCP/FCU selected altitude in feet, with bit 1.  value[1] = 16 u(15,12): FMS selected
 *          altitude in feet, with bit 14.  value[2] = 8000 + u(28,12): barometric setting in 0.1 mb, with bit 27.
 *          value[3] = u(49,3): VNAV, ALT HOLD, APPROACH, with bit 48.  value[4] = u(55,2): target altitude source,
 *          with bit 54.
 *     5,0  value[0] = s(2,9): roll, LSB 45/256 degrees, with bit 1.  value[1] = s(13,10) mod 2048: true track, LSB
 *          90/512 degrees, 0..2047, with bit 12.  value[2] = 2 u(25,10): ground speed in kt, with bit 24.  value[3] =
 *          s(36,9): track rate, LSB 8/256 degrees per second, with bit 35.  value[4] = 2 u(47,10): true airspeed in kt,
 *          with bit 46.
 *     6,0  value[0] = s(2,10) mod 2048: magnetic heading, LSB 90/512 degrees, with bit 1.  value[1] = u(14,10): IAS in
 *          kt, with bit 13.  value[2] = u(25,10): Mach, LSB 0.004, with bit 24.  value[3] = 32 s(36,9): barometric
 *          vertical rate in ft/min, with bit 35.  value[4] = 32 s(47,9): inertial vertical rate in ft/min, with bit 46.
 *     3,0  status is 0x1F.  value[0] = u(9,14): ARA.  value[1] = u(23,4): RAC.  value[2] = u(27,2): RAT and MTE.
 *          value[3] = u(29,2): TTI.  value[4] = u(31,26): TID.  word = u(1,32).
 *     1,0  status is 0x3.  value[0] = u(17,7): subnetwork version.  value[1] = u(15,1): overlay capability.  word =
 *          u(1,32).
 *     1,7  status is 0.  word = u(1,28): bit 27 - k of word is MB bit k + 1.  MB bits 1 to 24 stand for these
 *          registers, in this order: bits 1-6: 0,5 0,6 0,7 0,8 0,9 0,A; bits 7-8: 2,0 2,1; bits 9-15: 4,0 4,1 4,2 4,3
 *          4,4 4,5 4,8; bits 16-23: 5,0 5,1 5,2 5,3 5,4 5,5 5,6 5,F; bit 24: 6,0.
 *     2,0  status 0 and word 0.  The callsign is already in adsb_modes_rec.
 *   OUTPUTS  adsb_commb_rec recs[n], index for index with the list, every byte of every record written; the
 *     adsb_commb_header.
 * Nothing depends on atomics or scheduling: two runs give the same bytes.
 */
#define ADSB_COMMB_NOT_COMMB 0u
#define ADSB_COMMB_EMPTY 1u
#define ADSB_COMMB_NONE 2u
#define ADSB_COMMB_ONE 3u
#define ADSB_COMMB_AMBIGUOUS 4u
#define ADSB_COMMB_C10 0x1u
#define ADSB_COMMB_C17 0x2u
#define ADSB_COMMB_C20 0x4u
#define ADSB_COMMB_C30 0x8u
#define ADSB_COMMB_C40 0x10u
#define ADSB_COMMB_C50 0x20u
#define ADSB_COMMB_C60 0x40u
typedef struct adsb_commb_rec {   /* 32 bytes */
    uint8_t  state;               /* ADSB_COMMB_NOT_COMMB ...                                          */
    uint8_t  bds;                 /* 0x10, 0x17, 0x20, 0x30, 0x40, 0x50, 0x60 with ONE; else 0         */
    uint8_t  candidates;          /* ADSB_COMMB_C10 ...                                                */
    uint8_t  n_candidates;
    uint16_t status;
    uint16_t reserved;            /* 0 */
    int32_t  value[5];
    uint32_t word;
} adsb_commb_rec;
typedef struct adsb_commb_header { /* 128 bytes */
    uint64_t n, n_commb, n_empty, n_none, n_one, n_ambiguous;
    uint64_t n_bds[7];            /* ONE records per register, in the order of the candidate bits */
    uint64_t reserved[3];         /* 0 */
} adsb_commb_header;
#ifdef __cplusplus
static_assert(sizeof(adsb_commb_rec) == 32 && sizeof(adsb_commb_header) == 128, "adsb_commb_rec / adsb_commb_header layout");
#endif
/* Infers and decodes.  frames[n] in host memory or in device memory of the ctx's device; n comes from the host, as for
 * the other _of calls.  Asynchronous on the ctx's stream once a host list is copied.  Buffers are allocated on first
 * use and grown when needed (may wait for earlier work): per frame 32 bytes of results, and 48 bytes per 256 frames of
 * partial counts; a ctx that never calls it allocates nothing and launches exactly the kernels it launched before.
 * Replaces the result of an earlier call; shares no buffer with another stage's result.  n = 0 is ADSB_OK.  ADSB_E_ARG
 * for a NULL ctx or NULL frames with n > 0; ADSB_E_CAPACITY for n >= 2^32. */
int adsb_commb_of(adsb_ctx *ctx, const adsb_frame *frames, size_t n);
/* Waits and copies; recs may be NULL (with capacity 0) and receives min(header.n, max_recs) records; *header
 * (optional) the totals, whatever the capacity.  ADSB_E_STATE before any adsb_commb_of; ADSB_E_ARG for a NULL ctx or
 * NULL recs with a capacity. */
int adsb_fetch_commb(adsb_ctx *ctx, adsb_commb_rec *recs, size_t max_recs, adsb_commb_header *header);
/* For device-side consumers; does not synchronise.  The records and the header of the last adsb_commb_of in device
 * memory (each optional), valid until the next call and ordered on the ctx's stream behind it.  ADSB_E_STATE before
 * any adsb_commb_of. */
int adsb_commb_device(adsb_ctx *ctx, const adsb_commb_rec **recs_dev, const void **header_dev);
/* Threads (= frames) per workgroup of the stage's kernel: the size at which it takes another path, for tests.  The
 * result does not depend on it. */
int adsb_debug_commb_geometry(uint32_t *threads_per_block);

/*
 * Extended squitter status: what a DF17/18 frame says about the aircraft beside identity, position and velocity: the
 * emitter category (TC 1-4), the emergency state and squawk and the ACAS RA broadcast (TC 28), the target state (TC 29),
 * the operational status with the ADS-B version and the integrity and accuracy categories (TC 31), NACv of a velocity
 * (TC 19), NIC supplement B and the stand-alone containment radius of a position (TC 5-18, 20-22).  Stateless, per
 * frame, integers only, no inference (an extended squitter says what it is); computed on the device; the list is in
 * adsb_fetch's layout, as for adsb_modes_of and adsb_commb_of.  The stage decides whatever the frame's parity says:
 * consumers pair the record with adsb_modes_rec.kind, index for index.
 *   BIT NUMBERING  ME is bytes[4..11).  Bit 1 is the top bit of bytes[4], bit 56 the low bit of bytes[10]; u(a, n) is
 *     the n bits from bit a as an unsigned number (the numbering of MB in "Comm-B registers").  DF = bytes[0] >> 3,
 *     TC = u(1,5), ST = u(6,3).
 *   STATE  the first rule that applies:
 *     NOT_ES        DF is not 17 or 18.  Every other byte of the record is 0.
 *     FOREIGN       DF 18 with bytes[0] & 7 not 0 or 1 (TIS-B, ADS-R and the rest: other ME layouts).  Every other
 *                   byte is 0.
 *     CATEGORY      TC 1-4.
 *     POSITION      TC 0, 5-8, 9-18, 20-22.
 *     VELOCITY      TC 19 with ST 1-4.
 *     EMERGENCY     TC 28 with ST 1.
 *     ACAS_RA       TC 28 with ST 2.
 *     TARGET_STATE  TC 29 with u(6,2) == 1 (DO-260B; the DO-260A form, u(6,2) == 0, is counted as RESERVED).
 *     OPERATIONAL   TC 31 with ST 0 (airborne) or 1 (surface).
 *     RESERVED      everything else: type_code and subtype and nothing more.
 *     type_code is set in every state from CATEGORY on.  subtype is u(6,3) in VELOCITY, EMERGENCY, ACAS_RA,
 *     OPERATIONAL and RESERVED, u(6,2) for TC 29 (TARGET_STATE, or RESERVED), and 0 in CATEGORY and POSITION, whose
 *     bits 6-8 are no subtype.
 *   FIELDS  Bit ADSB_ES_HAS_x of `present` says that field x holds a value; a field whose bit is off is 0.
 *     CATEGORY      category = (0xE - TC) << 4 | u(6,3): set A to D in the high nibble, so TC 4 with CA 0 is 0xA0.
 *     POSITION      nic_b = u(8,1) for TC 9-18.  value = the containment radius Rc in decimetres that the type code
 *                   alone gives (the version-0 reading of adsb_host_es_integrity's table), with HAS_RC where it gives
 *                   one.  A consumer that knows the aircraft's version and supplements replaces it.
 *     VELOCITY      nac_v = u(11,3); flags INTENT_CHANGE = u(9,1) and IFR = u(10,1), with HAS_VELOCITY_FLAGS.
 *     EMERGENCY     emergency = u(9,3).  half[0] = the squawk of the 13 bits u(12,13), C1 A1 C2 A2 C4 A4 X B1 D1 B2 D2
 *                   B4 D4, as adsb_modes_rec.squawk spells it: 7700 reads 7700, X is ignored.
 *     ACAS_RA       value = u(9,32), half[0] = u(41,16): ARA 14, RAC 4, RAT 1, MTE 1, TTI 2, TID 26 bits, what BDS 3,0
 *                   carries at MB 9-56.
 *     TARGET_STATE  version = 2.  sil_supplement = u(8,1).  Flag ALT_FMS = u(9,1) (0: MCP/FCU) and flag TCAS = u(53,1),
 *                   always.  value = 32 (n - 1) feet with n = u(10,11) != 0: the selected altitude.  half[0] = 8000 +
 *                   8 (n - 1) tenths of a millibar with n = u(21,9) != 0: the barometric setting, in the unit of BDS
 *                   4,0's value[2].  half[1] = u(31,9) with u(30,1) set: the selected heading, LSB 180/256 degrees.
 *                   nac_p = u(40,4), nic_baro = u(44,1), sil = u(45,2).  With u(47,1) set, HAS_MODES and the flags
 *                   AUTOPILOT = u(48,1), VNAV = u(49,1), ALT_HOLD = u(50,1), APPROACH = u(52,1), LNAV = u(54,1).
 *     OPERATIONAL   version = u(41,3).  Version 0, 1, 2: half[0] = cc = u(9,16) and half[1] = om = u(25,16), raw.
 *                   Version 1 and 2: nic_a = u(44,1), nac_p = u(45,4), sil = u(51,2), flag HRD = u(54,1); ST 0:
 *                   nic_baro = u(53,1); ST 1: flag TRACK_HEADING = u(53,1) and length_width = u(21,4).  Version 2 also:
 *                   sil_supplement = u(55,1), sda = u(31,2); ST 0: gva = u(49,2); ST 1: nic_c = u(20,1) and the
 *                   surface nac_v = u(17,3).  Version 3-7: the version and nothing more.
 *   OUTPUTS  adsb_es_rec recs[n], index for index with the list, every byte of every record written; the
 *     adsb_es_header.
 * Nothing depends on atomics or scheduling: two runs give the same bytes.
 */
#define ADSB_ES_NOT_ES 0u
#define ADSB_ES_FOREIGN 1u
#define ADSB_ES_CATEGORY 2u
#define ADSB_ES_POSITION 3u
#define ADSB_ES_VELOCITY 4u
#define ADSB_ES_EMERGENCY 5u
#define ADSB_ES_ACAS_RA 6u
#define ADSB_ES_TARGET_STATE 7u
#define ADSB_ES_OPERATIONAL 8u
#define ADSB_ES_RESERVED 9u
#define ADSB_ES_STATES 10u
/* adsb_es_rec.present */
#define ADSB_ES_HAS_CATEGORY 0x1u
#define ADSB_ES_HAS_NIC_B 0x2u
#define ADSB_ES_HAS_RC 0x4u
#define ADSB_ES_HAS_NAC_V 0x8u
#define ADSB_ES_HAS_VELOCITY_FLAGS 0x10u
#define ADSB_ES_HAS_EMERGENCY 0x20u
#define ADSB_ES_HAS_SQUAWK 0x40u
#define ADSB_ES_HAS_RA 0x80u
#define ADSB_ES_HAS_SIL_SUPPLEMENT 0x100u
#define ADSB_ES_HAS_ALT_SOURCE 0x200u
#define ADSB_ES_HAS_SELECTED_ALT 0x400u
#define ADSB_ES_HAS_BARO 0x800u
#define ADSB_ES_HAS_HEADING 0x1000u
#define ADSB_ES_HAS_NAC_P 0x2000u
#define ADSB_ES_HAS_NIC_BARO 0x4000u
#define ADSB_ES_HAS_SIL 0x8000u
#define ADSB_ES_HAS_MODES 0x10000u
#define ADSB_ES_HAS_TCAS 0x20000u
#define ADSB_ES_HAS_VERSION 0x40000u
#define ADSB_ES_HAS_CC_OM 0x80000u
#define ADSB_ES_HAS_NIC_A 0x100000u
#define ADSB_ES_HAS_HRD 0x200000u
#define ADSB_ES_HAS_TRACK_HEADING 0x400000u
#define ADSB_ES_HAS_LENGTH_WIDTH 0x800000u
#define ADSB_ES_HAS_SDA 0x1000000u
#define ADSB_ES_HAS_GVA 0x2000000u
#define ADSB_ES_HAS_NIC_C 0x4000000u
/* adsb_es_rec.flags */
#define ADSB_ES_INTENT_CHANGE 0x1u
#define ADSB_ES_IFR 0x2u
#define ADSB_ES_ALT_FMS 0x4u
#define ADSB_ES_AUTOPILOT 0x8u
#define ADSB_ES_VNAV 0x10u
#define ADSB_ES_ALT_HOLD 0x20u
#define ADSB_ES_APPROACH 0x40u
#define ADSB_ES_LNAV 0x80u
#define ADSB_ES_TCAS 0x100u
#define ADSB_ES_HRD 0x200u
#define ADSB_ES_TRACK_HEADING 0x400u
/* the version argument of adsb_host_es_integrity for an aircraft whose operational status has not been heard */
#define ADSB_ES_VERSION_UNKNOWN 0xFFu
typedef struct adsb_es_rec {      /* 32 bytes */
    uint8_t  state;               /* ADSB_ES_NOT_ES ...                                                */
    uint8_t  type_code;
    uint8_t  subtype;
    uint8_t  version;
    uint32_t present;             /* ADSB_ES_HAS_...                                                   */
    uint8_t  nic_a, nic_b, nic_c;
    uint8_t  nac_p, nac_v;
    uint8_t  sil, sil_supplement;
    uint8_t  gva, sda, nic_baro;
    uint8_t  category;
    uint8_t  emergency;
    uint8_t  length_width;
    uint8_t  reserved;            /* 0 */
    uint16_t flags;               /* ADSB_ES_INTENT_CHANGE ...                                         */
    uint32_t value;               /* Rc in dm / selected altitude in ft / u(9,32) of an RA             */
    uint16_t half[2];             /* squawk, - / baro setting, heading / cc, om / u(41,16) of an RA, -  */
} adsb_es_rec;
typedef struct adsb_es_header {   /* 128 bytes */
    uint64_t n;
    uint64_t n_state[10];         /* records per state, n_state[ADSB_ES_NOT_ES] ...                    */
    uint64_t n_version[4];        /* OPERATIONAL records of version 0, 1, 2 and 3-7                    */
    uint64_t reserved;            /* 0 */
} adsb_es_header;
#ifdef __cplusplus
static_assert(sizeof(adsb_es_rec) == 32 && sizeof(adsb_es_header) == 128, "adsb_es_rec / adsb_es_header layout");
#endif
/* Reads every frame.  frames[n] in host memory or in device memory of the ctx's device; n comes from the host, as for
 * the other _of calls.  Asynchronous on the ctx's stream once a host list is copied.  Buffers are allocated on first
 * use and grown when needed (may wait for earlier work): per frame 32 bytes of results, and 56 bytes per 256 frames of
 * partial counts; a ctx that never calls it allocates nothing and launches exactly the kernels it launched before.
 * Replaces the result of an earlier call; shares no buffer with another stage's result.  n = 0 is ADSB_OK.  ADSB_E_ARG
 * for a NULL ctx or NULL frames with n > 0; ADSB_E_CAPACITY for n >= 2^32. */
int adsb_es_of(adsb_ctx *ctx, const adsb_frame *frames, size_t n);
/* Waits and copies; recs may be NULL (with capacity 0) and receives min(header.n, max_recs) records; *header
 * (optional) the totals, whatever the capacity.  ADSB_E_STATE before any adsb_es_of; ADSB_E_ARG for a NULL ctx or NULL
 * recs with a capacity. */
int adsb_fetch_es(adsb_ctx *ctx, adsb_es_rec *recs, size_t max_recs, adsb_es_header *header);
/* For device-side consumers; does not synchronise.  The records and the header of the last adsb_es_of in device memory
 * (each optional), valid until the next call and ordered on the ctx's stream behind it.  ADSB_E_STATE before any
 * adsb_es_of. */
int adsb_es_device(adsb_ctx *ctx, const adsb_es_rec **recs_dev, const void **header_dev);
/* Threads (= frames) per workgroup of the stage's kernel: the size at which it takes another path, for tests.  The
 * result does not depend on it. */
int adsb_debug_es_geometry(uint32_t *threads_per_block);

/*
 * Mode S replies from samples: a second scan of the sample buffer, beside the demodulator's, that finds the replies of
 * transponders without ADS-B (DF11 all-call, DF4/5/20/21 surveillance and Comm-B, DF0/16 air-air) and DF18.  The
 * demodulator keeps the reference's gate (preamble and the DF17 ordering test) and its list does not change; this scan
 * is opt-in, has a definition of its own (the reference has none) and never emits DF17.  Computed on the device; the
 * list is in adsb_fetch's layout and drops into adsb_modes_of, adsb_commb_of, adsb_correlate_of and
 * adsb_track_table_update_modes unchanged; adsb_merge_lists_of puts it and the demodulator's list into one.
 *   DEFINITION  On sample power, not on the floored magnitude: exact in integers, and no root.
 *     p[k]    = I[k]^2 + Q[k]^2      (ADSB_SAMPLE_I8: <= 32768; ADSB_SAMPLE_I16: <= 2^31, from (-32768, -32768); uint32)
 *     pre(i)  = min p[i+{0,2,7,9}] > max p[i+{1,3,4,5,6,8,10,11,12,13,14,15}]
 *               STRICT: a tie fails, so constant and all-zero input give nothing.
 *     bit_k   = p[i+16+2k] > p[i+17+2k], MSB first; a tie gives 0.
 *     DF      = bits 0..4;  L = 56 bits for DF < 16, 112 otherwise.
 *     WINDOW  offset i of a channel is examined iff i + 26 <= n_samples (the DF can be read), and can be emitted iff
 *             i + 16 + 2 L <= n_samples.  Short frames in the last 240 samples ARE found.  No window crosses a channel
 *             edge: every channel is a buffer of its own.
 *     S       = crc24(first L - 24 bits) ^ last 24 bits, generator 0x1FFF409.
 *     ACCEPT  DF11 iff S < 128 (a reply to interrogator S; adsb_modes_of's own rule).
 *             DF18 iff S == 0 (no repair here).
 *             DF0, 4, 5, 16, 20, 21 (address/parity, address = S): always; with ADSB_REPLIES_AP_KNOWN iff S is in
 *             known[].
 *             Every other DF, DF17 and DF24..31 included: never.  (DF24..31, first two bits 11, is a quarter of all
 *             noise candidates and is left out on purpose.)
 *     EMIT    per channel in ascending offset; every offset is independent of every other (nothing is skipped behind a
 *             frame); frame.offset = cfg.first_sample_index + i.  A frame has wire input's short-frame convention:
 *             bytes[0..7) the message and bytes[7..14) = 0 for a 56-bit frame; status = 0 and fixed_bit = 0xFF.
 *   KNOWN  known[n_known] is ascending, distinct and < 2^24, host or device memory: adsb_modes_of's known_out, or a
 *     table's ICAOs (a host array that breaks this is ADSB_E_ARG; for a device array it is an unchecked input
 *     contract).  The filter is WHOLE-CALL, NOT CAUSAL: an address first heard as DF11 in this very buffer is not yet
 *     known to the filter.  Without the filter every address/parity candidate is emitted and adsb_modes_of decides,
 *     causally, as it does for wire input; pure noise then yields about one frame per 10 000 offsets.
 *   RESULT  EXACT: every accepted frame is in the list, however many a tile holds, up to the capacity; there is no
 *     per-tile quota and no host re-run.  Capacity = cfg.max_frames, 0 meaning the ctx's cfg.max_out.  Past it the first
 *     frames in order are kept, header.flags has ADSB_FLAG_TRUNCATED, counts[] (frames per channel) are clipped to the
 *     list and total_found is the full number, as for wire input.
 *   HEADER  n_out frames in the list; total_found = n_all_call + n_df18 + n_address_parity, the accepted frames of each
 *     sort; n_preamble the examined offsets with pre(i); n_not_known the address/parity frames the filter turned away;
 *     n_parity the DF11 / DF18 candidates whose check failed.  The last four count only candidates that can be emitted
 *     (the window rule), n_preamble all that are examined.  flags = ADSB_FLAG_*; reserved = 0.
 * Nothing depends on atomics or scheduling: two runs give the same bytes.
 * MERGE  adsb_merge_lists_of merges two lists in adsb_fetch's layout with the same n_channels, each channel's frames
 *   in ascending offset, into one such list: out has counts_a[c] + counts_b[c] = counts_out[c] frames of channel c, in
 *   ascending offset; on equal offsets list A's frame goes first; frames of one list keep their order.  src[k] = the
 *   index of out[k] in its own list, with the top bit (ADSB_MERGE_FROM_B) set for list B, so a caller can carry side
 *   arrays such as level records along.
 */
#define ADSB_REPLIES_AP_KNOWN 0x1u
#define ADSB_MERGE_FROM_B 0x80000000u
typedef struct adsb_replies_cfg {      /* 32 bytes */
    uint32_t flags;               /* ADSB_REPLIES_AP_KNOWN or 0                                        */
    uint32_t reserved;            /* 0 */
    uint64_t max_frames;          /* 0: cfg.max_out of the ctx                                         */
    uint64_t first_sample_index;  /* added to every offset, every channel                              */
    uint64_t reserved2;           /* 0 */
} adsb_replies_cfg;
typedef struct adsb_replies_header {   /* 80 bytes */
    uint64_t n_out, total_found, n_preamble, n_all_call, n_df18, n_address_parity, n_not_known, n_parity, flags, reserved;
} adsb_replies_header;
#ifdef __cplusplus
static_assert(sizeof(adsb_replies_cfg) == 32 && sizeof(adsb_replies_header) == 80, "adsb_replies_cfg / adsb_replies_header layout");
#endif
/* Scans.  iq_dev, n_channels, n_samples and channel_stride as for adsb_demod_device_async (samples of the ctx's
 * sample_type in device memory, 16-byte aligned, channel_stride a multiple of 8 and >= n_samples when n_channels > 1);
 * known in host or device memory.  Asynchronous on the ctx's stream once a host known[] is copied; reads the samples
 * only, so it may follow or precede a launch on the same buffer.  Buffers are allocated on first use and grown when
 * needed (may wait for earlier work): 24 bytes per frame of capacity, and per tile of 8192 (i8) or 4096 (CS16) offsets
 * 1 KiB of bitmap and 36 bytes of counts; a ctx that never calls it allocates nothing and launches exactly the kernels
 * it launched before.  Replaces the result of an earlier call.  Not for use while a feed is open: a feed's consumer has
 * the host buffer and adsb_host_replies.  ADSB_E_ARG for a NULL ctx, cfg or iq_dev, n_channels == 0, unknown flags or
 * non-zero reserved words, a misaligned iq_dev or stride, a stride below n_samples, NULL known with n_known > 0,
 * n_known > 2^24, or a host known[] that is not ascending, distinct and < 2^24; ADSB_E_SHORT for n_samples < 26;
 * ADSB_E_CAPACITY for n_channels or n_samples above the ctx's, or max_frames >= 2^32.  A rejected call writes nothing
 * and leaves an earlier result as it was. */
int adsb_replies_of(adsb_ctx *ctx, const adsb_replies_cfg *cfg, const void *iq_dev, uint32_t n_channels, size_t n_samples,
                    size_t channel_stride, const uint32_t *known, size_t n_known);
/* Waits and copies; each output may be NULL.  out receives min(header.n_out, max_out) frames and *n_out that number;
 * counts the call's n_channels entries (clipped to the list of header.n_out frames, not to max_out); *header the totals,
 * whatever the capacity.  ADSB_E_STATE before any adsb_replies_of; ADSB_E_ARG for a NULL ctx or NULL out with a
 * capacity. */
int adsb_fetch_replies(adsb_ctx *ctx, adsb_frame *out, size_t max_out, size_t *n_out, uint64_t *counts,
                       adsb_replies_header *header);
/* For device-side consumers; does not synchronise.  The list, the per-channel counts and the header of the last
 * adsb_replies_of in device memory (each optional), valid until the next call and ordered on the ctx's stream behind
 * it.  ADSB_E_STATE before any adsb_replies_of. */
int adsb_replies_device(adsb_ctx *ctx, const adsb_frame **frames_dev, const uint64_t **counts_dev, const void **header_dev);
/* Offsets per tile (= per workgroup) of the scan for each sample type (either may be NULL): the sizes at which the scan
 * takes another path, for tests.  The result does not depend on them. */
int adsb_debug_replies_geometry(uint32_t *tile_offsets_i8, uint32_t *tile_offsets_i16);
/* MERGE above.  a, b, counts_a, counts_b, out, src and counts_out each in host memory or in device memory of the ctx's
 * device; out and src hold the sum of all counts, counts_out n_channels entries; src and counts_out may be NULL.
 * Blocking.  ADSB_E_ARG for a NULL ctx, NULL counts, n_channels outside 1..2^20, or a NULL list or out with frames to
 * read or write; ADSB_E_CAPACITY for 2^31 frames or more in either list. */
int adsb_merge_lists_of(adsb_ctx *ctx, const adsb_frame *a, const uint64_t *counts_a, const adsb_frame *b,
                        const uint64_t *counts_b, uint32_t n_channels, adsb_frame *out, uint32_t *src, uint64_t *counts_out);

/*
 * Multilaterate: where each correlated message was sent from, solved from the times its receivers heard it.  One small
 * non-linear least-squares problem per message, all messages of a list in one kernel; f64; stateless.
 *   INPUT  a correlate result msgs[M] / recs[N]; adsb_mlat_receiver receivers[R], 1 <= R <= 256, WGS84 degrees and
 *     metres above the ellipsoid, with each receiver's clock offset in seconds (what its clock shows minus true time);
 *     optionally adsb_wire_rx rx[n_rx], the wire-input records of the list that was correlated, indexed by
 *     adsb_reception.frame; an adsb_mlat_cfg.
 *   TIME  cfg.time_source = ADSB_MLAT_TIME_RECEPTION takes adsb_reception.time, in units of cfg.seconds_per_tick (> 0;
 *     for this project's own channels the sample period).  ADSB_MLAT_TIME_TICKS takes rx[frame].ticks, the raw 48-bit
 *     timestamp that wire input keeps at full resolution, in units of cfg.seconds_per_tick (0: 1 / 12e6).  Only
 *     differences against the first used reception are taken, as integers before anything becomes a double:
 *     RECEPTION: (int64)(t_i - t_0) of the uint64 difference; TICKS: (t_i - t_0) mod 2^48, sign-extended into
 *     [-2^47, 2^47).  The measured range difference of reception i is
 *       rho_i = c x ((double)dticks_i x seconds_per_tick - (clock_offset_s[r_i] - clock_offset_s[r_0]))
 *     with c = ADSB_MLAT_C, light in air.
 *   USED  Inside a message (receptions are in (T, j) order) reception k = 0, 1, ... is USED iff no reception k' < k of
 *     the message has the same receiver: one time per receiver, the earliest.  Reception 0 is always used and is "the
 *     first used reception" above.  A message with more than ADSB_MLAT_MAX_RECEPTIONS receptions is not attempted
 *     (TOO_MANY).  need = max(cfg.min_receivers, floor) with floor = 3 for a message with an altitude and 4 without
 *     (min_receivers = 0: the floor alone); fewer used receptions than need: not attempted (TOO_FEW).
 *   ALTITUDE  With ADSB_MLAT_USE_ALTITUDE in cfg.flags, a message with bytes[0] >> 3 in {17, 18}, type code (ME bits
 *     0-4) 9..18, a non-zero 12-bit altitude code (ME bits 8-19) and its Q bit (ME bit 15) set HAS AN ALTITUDE:
 *     (25 N - 1000) ft x 0.3048 m, N = the code's other 11 bits.  It adds one equation, h(p) - altitude = 0.
 *   MODEL  Unknowns (x, y, z, d): ECEF metres and d = c x (emission time - time of the first used reception).  Residual
 *     of used reception i at station s_i: |p - s_i| + d - rho_i; its Jacobian row is ((p - s_i) / |p - s_i|, 1), the
 *     unit vector taken as 0 when |p - s_i| = 0.  h(p) is Bowring's closed form with TWO refinement steps:
 *     P = sqrt(x^2 + y^2), beta = atan2(a z, b P); twice: phi = atan2(z + e'^2 b sin^3 beta, P - e^2 a cos^3 beta),
 *     beta = atan2(b sin phi, a cos phi); h = P cos phi + z sin phi - a sqrt(1 - e^2 sin^2 phi); lambda from x / P and
 *     y / P (P = 0: cos lambda = 1).  The altitude row's Jacobian is the ellipsoid normal (cos phi cos lambda,
 *     cos phi sin lambda, sin phi, 0).  a = 6378137, f = 1 / 298.257223563.
 *   SUMS  The cost is the sum of squared residuals.  Every sum over receptions (the 10 entries of JtJ, the 4 of Jtr,
 *     the cost; the 3 coordinate sums of the centroid) is 16 partial sums folded in a butterfly: partial l adds the
 *     terms of the used receptions k = l (mod 16) in ascending k, starting from 0; then four rounds v[l] = v[l] +
 *     v[l ^ m] for m = 8, 4, 2, 1.  The altitude row is added to the folded sums last.  All f64, contraction off.
 *   SOLVER  Levenberg-Marquardt on the 4 x 4 normal equations: (JtJ + lambda diag(JtJ)) delta = -Jtr, lambda from 1e-3,
 *     divided by 10 after an accepted step and multiplied by 10 after a rejected one, kept inside [1e-12, 1e12].  A
 *     step is accepted iff the cost at p + delta is <= the cost at p.  A stage is converged when a step's position part
 *     is shorter than cfg.step_tol_m (0: 0.01 m), accepted or not; it takes at most cfg.max_iterations steps (0: 24; at
 *     most 1000).  The linear solve is an L D Lt factorisation in the order x, y, z, d without pivoting; a pivot that
 *     is not greater than 1e-12 x its diagonal entry gives SINGULAR and ends the solve.
 *     Stage 1 holds the height: the altitude equation with the message's altitude, or with cfg.default_altitude_m
 *     (0: 10000 m) when it has none.  It starts from the centroid of the used receivers' ECEF positions moved along its
 *     own ellipsoid normal to that height, with d = -|p - s_0|.  Stage 2 starts from stage 1's result (converged or
 *     not) and solves the message's real equations; lambda starts again.  A message with an altitude runs stage 1 only.
 *     Ground receivers are nearly coplanar, and a free solve started from the centroid falls through their plane into
 *     the mirror solution for one emitter in seven; started from the height-held solution it does not.
 *   OUTPUT  adsb_mlat_fix fixes[M], index for index with msgs[].  latitude / longitude in degrees, height_m above the
 *     ellipsoid, time_s = d / c (emission relative to the first used reception's true time), residual_rms_m =
 *     sqrt(cost / equations) of the last stage, n_used, iterations (steps of both stages), and the dilutions from the
 *     position block of the inverse of the last stage's undamped JtJ at the solution (the same factorisation and pivot
 *     rule; SINGULAR leaves them 0): pdop = sqrt(trace), hdop / vdop after rotating the block to local east / north / up.
 *     flags: ATTEMPTED; ALTITUDE (the message's altitude was used); CONVERGED (the last stage converged);
 *     REJECTED_RESIDUAL (residual_rms_m > cfg.max_residual_m; 0: no limit); REJECTED_RANGE (farther from the used
 *     receivers' centroid than cfg.max_range_m; 0: 500 km); VALID = CONVERGED and neither SINGULAR nor rejected.  A
 *     fix that was not attempted holds its reason (TOO_FEW, TOO_MANY, BAD_INDEX), n_used where known, and zeros.
 *     BAD_INDEX: a reception's receiver >= R, a message's receptions past recs[N], or with TICKS a frame >= n_rx; found
 *     on the device, never read.  adsb_mlat_header { n_messages, n_attempted, n_valid, flags } comes from a reduction
 *     over the fixes; flags has ADSB_MLAT_HDR_BAD_INDEX if any fix has BAD_INDEX.
 * No atomics, nothing depends on scheduling: two runs give the same bytes.  The CPU mirror (adsb_host_multilaterate)
 * evaluates the same text in the same order; what may differ is the last bit of the math library (atan2, sin, cos) in
 * the height formula and the output conversion, and whatever device and host sqrt and division differ by.
 */
#define ADSB_MLAT_C (299792458.0 / 1.0003) /* m/s */
#define ADSB_MLAT_MAX_RECEPTIONS 256
#define ADSB_MLAT_TIME_RECEPTION 0u
#define ADSB_MLAT_TIME_TICKS 1u
#define ADSB_MLAT_USE_ALTITUDE 0x1u        /* adsb_mlat_cfg.flags */
#define ADSB_MLAT_ATTEMPTED 0x1u           /* adsb_mlat_fix.flags */
#define ADSB_MLAT_CONVERGED 0x2u
#define ADSB_MLAT_ALTITUDE 0x4u
#define ADSB_MLAT_TOO_FEW 0x8u
#define ADSB_MLAT_TOO_MANY 0x10u
#define ADSB_MLAT_SINGULAR 0x20u
#define ADSB_MLAT_REJECTED_RESIDUAL 0x40u
#define ADSB_MLAT_REJECTED_RANGE 0x80u
#define ADSB_MLAT_VALID 0x100u
#define ADSB_MLAT_BAD_INDEX 0x200u
#define ADSB_MLAT_HDR_BAD_INDEX 0x1u       /* adsb_mlat_header.flags */
typedef struct adsb_mlat_receiver { /* 32 bytes */
    double latitude, longitude;   /* degrees, [-90, 90] and [-180, 180]                           */
    double height_m;              /* above the ellipsoid, [-1000, 100000]                         */
    double clock_offset_s;        /* what this receiver's clock shows minus true time, |.| <= 1e6 */
} adsb_mlat_receiver;
typedef struct adsb_mlat_cfg {      /* 64 bytes */
    uint32_t time_source;         /* ADSB_MLAT_TIME_*                                             */
    uint32_t flags;               /* ADSB_MLAT_USE_ALTITUDE                                       */
    uint32_t min_receivers;       /* 0: the floor (3 with an altitude, 4 without); at most 256    */
    uint32_t max_iterations;      /* per stage; 0: 24; at most 1000                               */
    double   seconds_per_tick;    /* RECEPTION: > 0; TICKS: 0 = 1 / 12e6                          */
    double   step_tol_m;          /* 0: 0.01                                                      */
    double   max_residual_m;      /* 0: no limit                                                  */
    double   max_range_m;         /* 0: 500e3                                                     */
    double   default_altitude_m;  /* 0: 10000                                                     */
    uint64_t reserved;            /* 0 */
} adsb_mlat_cfg;
typedef struct adsb_mlat_fix {      /* 64 bytes */
    double   latitude, longitude; /* degrees */
    double   height_m;
    double   time_s;
    float    residual_rms_m, pdop, hdop, vdop;
    uint16_t n_used, iterations;
    uint32_t flags;               /* ADSB_MLAT_* */
    uint64_t reserved;            /* 0 */
} adsb_mlat_fix;
typedef struct adsb_mlat_header {   /* 32 bytes */
    uint64_t n_messages, n_attempted, n_valid, flags;
} adsb_mlat_header;
/* The ctx's last correlate result (adsb_correlate_launch or adsb_correlate_of), solved where it lies: enqueued on the
 * ctx's stream behind it, nothing read back.  receivers is host memory; rx (NULL with TIME_RECEPTION) is host memory or
 * device memory of the ctx's device and holds one record per frame of the correlated list, e.g. adsb_wire_in_device's.
 * Buffers are allocated on first use and grown when needed (may wait for earlier work): 64 bytes per message of
 * capacity, 8 KiB of stations, the reduction's temporary storage, and copies of host lists; a ctx that never calls it
 * allocates nothing and launches exactly the kernels it launched before.  Replaces the result of an earlier
 * multilaterate call.  ADSB_E_ARG for a NULL ctx, cfg or receivers, n_receivers outside 1..256, a receiver or cfg value
 * that is not finite or out of the ranges above, an unknown time_source or flag, TICKS without rx; ADSB_E_STATE before
 * any correlate call. */
int adsb_multilaterate(adsb_ctx *ctx, const adsb_mlat_cfg *cfg, const adsb_mlat_receiver *receivers, uint32_t n_receivers,
                       const adsb_wire_rx *rx);
/* Any lists: msgs[n_msgs], recs[n_recs] and rx[n_rx] (NULL / 0 with TIME_RECEPTION), each in host memory or in device
 * memory of the ctx's device.  Asynchronous on the ctx's stream once host arrays are copied.  The errors above, and
 * ADSB_E_ARG for NULL msgs or recs with a count > 0; ADSB_E_CAPACITY for a count >= 2^32. */
int adsb_multilaterate_of(adsb_ctx *ctx, const adsb_mlat_cfg *cfg, const adsb_mlat_receiver *receivers,
                          uint32_t n_receivers, const adsb_message *msgs, size_t n_msgs, const adsb_reception *recs,
                          size_t n_recs, const adsb_wire_rx *rx, size_t n_rx);
/* Waits and copies: fixes receives min(header.n_messages, max) records and *n (optional) that number; *header
 * (optional) the totals whatever max.  ADSB_E_STATE before any multilaterate call; ADSB_E_ARG for a NULL ctx, NULL
 * fixes with max > 0, or, after copying, when the header has ADSB_MLAT_HDR_BAD_INDEX. */
int adsb_fetch_mlat(adsb_ctx *ctx, adsb_mlat_fix *fixes, size_t max, size_t *n, adsb_mlat_header *header);
/* For device-side consumers; does not synchronise.  fixes[] and the header in device memory (each optional), valid until
 * the next multilaterate call on this ctx and ordered on the ctx's stream behind it.  ADSB_E_STATE before any. */
int adsb_mlat_device(adsb_ctx *ctx, const adsb_mlat_fix **fixes_dev, const void **header_dev);
/* Lanes that share one message and messages per workgroup of the solver kernel (either may be NULL): the sizes at which
 * it takes another path, for tests.  The result does not depend on them. */
int adsb_debug_mlat_geometry(uint32_t *lanes_per_message, uint32_t *messages_per_block);

/*
 * Clock sync: every receiver's clock offset and drift against one reference receiver, from the position messages of a
 * correlated list.  An airborne position message says where it was sent from, so a message heard by two receivers
 * measures the difference of their clocks; all such messages of a list are one linear least-squares problem.  f64;
 * stateless; computed on the device.  adsb_clock_apply then writes the receptions with corrected times, which
 * multilaterate takes through its TIME_RECEPTION input.
 *   INPUT  a correlate result msgs[M] / recs[N]; adsb_mlat_receiver receivers[R], 1 <= R <= 256, positions as for
 *     multilaterate; clock_offset_s is the caller's PRIOR, the coarse alignment it already used to make correlate group
 *     the receptions (0 if none; |.| <= 1e6); optionally adsb_wire_rx rx[n_rx]; an adsb_clock_cfg.
 *   TIMES  Multilaterate's, by the same functions: time_source (RECEPTION or TICKS), seconds_per_tick (spt; TICKS: 0 =
 *     1 / 12e6), the integer difference dticks_k of used reception k against the message's first used reception (TICKS:
 *     mod 2^48, sign-extended), and the USED rule (the earliest reception per receiver; reception 0 is always used).  A
 *     message's own time is tau_m = (double)(int64)(msgs[m].time - msgs[0].time) x cfg.seconds_per_time, the unit of
 *     adsb_message.time (RECEPTION: 0 = seconds_per_tick; TICKS: 0 is ADSB_E_ARG).
 *   ELIGIBLE  The single-message position decode ("Positions from single messages") is applied to the message bytes
 *     with the site { latitude, longitude of the first used reception's receiver, cfg.max_range_nm (0: 180) }.  The
 *     message is eligible when the decode gives ADSB_FIX_VALID without ADSB_FIX_SURFACE, gives ADSB_FIX_ALT, the altitude
 *     has its Q bit set and a non-zero code (multilaterate's ALTITUDE rule), it has at most ADSB_MLAT_MAX_RECEPTIONS
 *     receptions and at least two of them are used.  Its position p is the ECEF point of (latitude, longitude,
 *     altitude ft x 0.3048), by the conversion multilaterate uses for its stations.  Barometric altitude is taken as
 *     height above the ellipsoid: a known approximation, tens of metres of height, which a receiver's offset absorbs
 *     only in part.
 *   ROWS  Each used reception k >= 1 of an eligible message gives one row (i = r_0, j = r_k, tau_m, y) with
 *       y = (double)dticks_k x spt - (prior_j - prior_i) - (|p - s_j| - |p - s_i|) / ADSB_MLAT_C
 *     in the slot of its reception index, msgs[m].first + k.  Every other slot is empty.  No compaction, no atomics.
 *   MODEL  Receiver r's clock shows true time plus prior_r + a_r + b_r x tau.  A row says y = (a_j + b_j tau) -
 *     (a_i + b_i tau).  cfg.reference (< R) has a = b = 0.
 *   PAIRS  A row's pair is (lo, hi) = (min, max) of (i, j); its y' = y if j = hi, else -y.  Rows are ordered by (pair,
 *     slot) with a stable radix sort whose key puts empty slots last.  A pair's sums are n and the five f64 sums of tau,
 *     tau^2, y', tau y', y'^2: 64 partial sums folded in a butterfly.  Partial l adds the pair's rows q = l (mod 64), q
 *     counting the pair's rows in that order, in ascending q, starting from 0; then v[l] = v[l] + v[l ^ m] for m = 32,
 *     16, 8, 4, 2, 1.  Contraction off.
 *   REACHED  Pairs with n >= cfg.min_rows (0: 1) are EDGES.  Receivers connected to the reference through edges are
 *     REACHED; every other receiver gets a = b = 0.  Rows of pairs that are not edges take no part in the solve.
 *   SOLVE  Unknowns (a_r, b_r) per reached receiver other than the reference, in ascending r, interleaved; without
 *     ADSB_CLOCK_DRIFT in cfg.flags, a_r only.  The normal equations come from the edges' sums: the entry of (a_u, a_u)
 *     is the sum of n over u's edges, (b_u, a_u) of the tau sums, (b_u, b_u) of the tau^2 sums, each added in ascending
 *     partner index starting from 0; between receivers u != v joined by an edge the entries are minus that edge's sums;
 *     the right-hand side of a_u adds +(sum of y') for each partner below u and -(sum of y') for each partner above,
 *     of b_u likewise with the sums of tau y', in ascending partner index.  L D Lt without pivoting, left-looking: entry
 *     (i, j) is A_ij - sum over k < j of (L_ik x D_k) x L_jk, ascending k.  Then v = the right-hand side; for k
 *     ascending, v_i = v_i - L_ik x v_k for every i > k; v_i = v_i / D_i; for k descending, v_i = v_i - L_ki x v_k
 *     for every i < k.  A pivot that is not greater than 1e-12 x its diagonal entry ends the solve with drift: the
 *     whole solve is repeated for offsets only and the header gets ADSB_CLOCK_HDR_DRIFT_DROPPED.  If that fails too,
 *     the header gets ADSB_CLOCK_HDR_SINGULAR and every a and b is 0.
 *   SECOND PASS  With cfg.max_residual_s > 0, the residual y' - ((a_hi + b_hi tau) - (a_lo + b_lo tau)) of every row
 *     under the first solution is computed; rows with |residual| > max_residual_s are DROPPED (their slots become
 *     empty), and order, sums, reached set and solve are redone over the kept rows.  0: one pass.
 *   OUTPUT  adsb_clock clocks[R]: offset_s = prior + a, fine_offset_s = a, drift = b; n_rows the kept rows the receiver
 *     takes part in (edges or not), n_dropped the dropped ones, n_partners its edges; residual_rms_s =
 *     sqrt(max(S, 0) / n_rows) with S the sum over its pairs, in ascending partner index, of the pair's
 *     sum(y'^2) - 2 da sum(y') - 2 db sum(tau y') + da^2 n + 2 da db sum(tau) + db^2 sum(tau^2), da and db the pair's
 *     hi minus lo solution (0 when n_rows = 0; a closed form, exact to about 1e-7 of the largest |y'|).  flags: REFERENCE, REACHED (the reference is), DRIFT (b was solved).
 *     adsb_clock_header: n_messages; n_eligible; n_rows (before dropping); n_dropped; n_reached (the reference
 *     included); flags: ADSB_CLOCK_HDR_BAD_INDEX as multilaterate defines BAD_INDEX (the message is skipped, its
 *     stations and ticks never read), DRIFT_DROPPED, SINGULAR.
 *   APPLY  adsb_clock_apply writes adsb_reception corrected[N]: order, frame and receiver as in recs, and for every
 *     reception that a message owns inside recs[N] and whose own receiver (and, with TICKS, frame) the lists have
 *       time' = (uint64)(256 x d - llrint(256 x (offset_s[r] + drift[r] x tau_m) / spt))        (mod 2^64)
 *     d the reception's raw time as a signed integer difference against the raw time of recs[msgs[0].first] (TICKS:
 *     mod 2^48, sign-extended; 0 is taken for that raw time if the lists do not have it), m the reception's message.  The
 *     unit of time' is spt / 256: pass `corrected` to adsb_multilaterate_of with TIME_RECEPTION, seconds_per_tick =
 *     spt / 256 and every clock_offset_s = 0.  An unreached receiver's receptions get offset = prior, drift = 0 (see
 *     its clock's flags).  Messages without a position are corrected like every other: they are what this is for.
 *     Every other reception keeps its raw time.
 * No atomics, no library scan or reduce-by-key for the float sums, nothing depends on scheduling: two runs give the same
 * bytes.  The CPU mirror (adsb_host_clock_sync / adsb_host_clock_apply) evaluates the same text in the same order; what
 * may differ is the last bit of the math libraries' sin / cos / sqrt in the decode, the ECEF conversion and the ranges.
 */
#define ADSB_CLOCK_DRIFT 0x1u              /* adsb_clock_cfg.flags: solve a drift per receiver */
#define ADSB_CLOCK_REFERENCE 0x1u          /* adsb_clock.flags */
#define ADSB_CLOCK_REACHED 0x2u
#define ADSB_CLOCK_HAS_DRIFT 0x4u          /* DRIFT: b was solved for this receiver */
#define ADSB_CLOCK_HDR_BAD_INDEX 0x1u      /* adsb_clock_header.flags */
#define ADSB_CLOCK_HDR_DRIFT_DROPPED 0x2u
#define ADSB_CLOCK_HDR_SINGULAR 0x4u
typedef struct adsb_clock_cfg {     /* 64 bytes */
    uint32_t time_source;         /* ADSB_MLAT_TIME_*                                             */
    uint32_t flags;               /* ADSB_CLOCK_DRIFT                                             */
    uint32_t reference;           /* < n_receivers                                                */
    uint32_t min_rows;            /* rows that make a pair an edge; 0: 1                          */
    double   seconds_per_tick;    /* RECEPTION: > 0; TICKS: 0 = 1 / 12e6; at most 1               */
    double   seconds_per_time;    /* unit of adsb_message.time; RECEPTION: 0 = seconds_per_tick   */
    double   max_residual_s;      /* 0: one pass                                                  */
    double   max_range_nm;        /* 0: 180; at most 180                                          */
    uint64_t reserved[2];         /* 0 */
} adsb_clock_cfg;
typedef struct adsb_clock {         /* 64 bytes */
    double   offset_s;            /* prior + a */
    double   fine_offset_s;       /* a */
    double   drift;               /* b, s/s */
    float    residual_rms_s;      /* over the kept rows the receiver takes part in */
    uint32_t n_rows;
    uint32_t n_dropped;
    uint32_t n_partners;          /* edges */
    uint32_t flags;               /* ADSB_CLOCK_REFERENCE, REACHED, HAS_DRIFT */
    uint32_t reserved[5];         /* 0 */
} adsb_clock;
typedef struct adsb_clock_header {  /* 64 bytes */
    uint64_t n_messages, n_eligible, n_rows, n_dropped, n_reached, flags;
    uint64_t reserved[2];         /* 0 */
} adsb_clock_header;
/* The ctx's last correlate result, where it lies: enqueued on the ctx's stream behind it, nothing read back.  receivers
 * is host memory; rx (NULL with TIME_RECEPTION) as for adsb_multilaterate.  Buffers are allocated on first use and grown
 * when needed (may wait for earlier work): 44 bytes per reception of capacity (rows, keys and orders, the corrected
 * list), 1 byte per message, the sorts' temporary storage, 6 MiB of pair sums (48 bytes per pair and pass), the 2 MiB of
 * the normal equations, and copies of host lists; a ctx that never calls it allocates nothing and launches exactly the kernels it
 * launched before.  Replaces the result of an earlier clock-sync call.  ADSB_E_ARG for a NULL ctx, cfg or receivers,
 * n_receivers outside 1..256, a receiver or cfg value that is negative where it may not be, not finite or out of the
 * ranges above, an unknown time_source or flag, reference >= n_receivers, TICKS without rx or with seconds_per_time = 0;
 * ADSB_E_STATE before any correlate call. */
int adsb_clock_sync(adsb_ctx *ctx, const adsb_clock_cfg *cfg, const adsb_mlat_receiver *receivers, uint32_t n_receivers,
                    const adsb_wire_rx *rx);
/* Any lists, as for adsb_multilaterate_of, with its errors.  Device lists must stay as they are until adsb_clock_apply
 * has run, if it is called. */
int adsb_clock_sync_of(adsb_ctx *ctx, const adsb_clock_cfg *cfg, const adsb_mlat_receiver *receivers,
                       uint32_t n_receivers, const adsb_message *msgs, size_t n_msgs, const adsb_reception *recs,
                       size_t n_recs, const adsb_wire_rx *rx, size_t n_rx);
/* Waits and copies: clocks receives min(n_receivers, max) records and *n (optional) that number; *header (optional) the
 * totals.  ADSB_E_STATE before any clock-sync call; ADSB_E_ARG for a NULL ctx, NULL clocks with max > 0, or, after
 * copying, when the header has ADSB_CLOCK_HDR_BAD_INDEX. */
int adsb_fetch_clocks(adsb_ctx *ctx, adsb_clock *clocks, size_t max, size_t *n, adsb_clock_header *header);
/* For device-side consumers; does not synchronise.  clocks[] and the header in device memory (each optional), valid until
 * the next clock-sync call on this ctx and ordered on the ctx's stream behind it.  ADSB_E_STATE before any. */
int adsb_clocks_device(adsb_ctx *ctx, const adsb_clock **clocks_dev, const void **header_dev);
/* Corrects the receptions of the lists the last clock-sync call worked on, by its clocks, on the ctx's stream behind it.
 * Replaces the result of an earlier apply.  After adsb_clock_sync those lists are the ctx's correlate result: call this
 * before the next correlate call replaces it.  ADSB_E_STATE without a clock-sync call. */
int adsb_clock_apply(adsb_ctx *ctx);
/* Waits and copies min(N, max) corrected receptions; *n (optional) that number, *n_total (optional) N.  ADSB_E_STATE
 * before any adsb_clock_apply. */
int adsb_fetch_clock_receptions(adsb_ctx *ctx, adsb_reception *corrected, size_t max, size_t *n, size_t *n_total);
/* For device-side consumers; does not synchronise: corrected[] in device memory, an argument for adsb_multilaterate_of,
 * and its length's upper bound (the list's N as the host knows it).  ADSB_E_STATE before any adsb_clock_apply. */
int adsb_clock_receptions_device(adsb_ctx *ctx, const adsb_reception **corrected_dev, size_t *n);
/* Messages per workgroup of the rows kernel and the partial sums of a pair (a pair's partial sum holds every 64th of its
 * rows), either may be NULL: the sizes at which the kernels take another path, for tests.  The result does not depend
 * on the first. */
int adsb_debug_clock_geometry(uint32_t *messages_per_block, uint32_t *pair_partials);

/*
 * Tracker + global CPR position decode on the device: what the reference's display
 * threads do with every AdsbPacket, `handle_aircraft_update` (src/adsb/aircraft.rs:158-165 ->
 * Aircraft::handle_packet, aircraft.rs:48-111 -> cpr::calculate_geographic_position, cpr.rs:135-147),
 * applied to the ordered frame list of the last single-channel launch, starting from an empty aircraft
 * map (like the demodulation itself, no state is carried between launches; adsb_track_table_* below keeps
 * one aircraft map across launches, as the reference's display threads do).  Packet time = frame offset
 * x seconds_per_sample (the reference stamps the wall clock; excluded from parity).  f64 arithmetic;
 * parity with the reference is by tolerance (its own tests use 1e-4 degrees).
 */
#define ADSB_TRACK_NEW_POSITION 0x1u /* this frame completed an even/odd pair: latitude/longitude valid */
typedef struct adsb_track_point {   /* one per frame, in frame order */
    double   latitude, longitude;   /* degrees; 0 unless ADSB_TRACK_NEW_POSITION */
    uint32_t icao;
    uint32_t flags;
} adsb_track_point;
typedef struct adsb_aircraft_record { /* AircraftSummary (aircraft.rs:14-23), one per ICAO, ascending ICAO */
    double   latitude, longitude;   /* geo_position, valid if has_position */
    double   last_contact;          /* seconds: time of the last position message (aircraft.rs:56); NaN if none */
    uint32_t icao;
    int32_t  altitude;              /* feet, of the last position message; 0 if none */
    uint32_t has_position;
    uint32_t n_frames;              /* frames of this aircraft in the list */
    char     callsign[8];           /* of the last identification message; zeros if none (not NUL terminated) */
} adsb_aircraft_record;
/* Runs adsb_decode_fields_device_async if needed, waits for the list's length, then enqueues the tracker
 * on the ctx stream.  ADSB_E_ARG for multi-channel launches. */
int adsb_track_device(adsb_ctx *ctx, double seconds_per_sample);
/* Waits and copies: up to max_points per-frame points (frame order) and up to max_aircraft records
 * (ascending ICAO); either array may be NULL with a zero count.  *n_aircraft is the number of distinct
 * ICAO addresses in the list even if fewer records were copied. */
int adsb_fetch_track(adsb_ctx *ctx, adsb_track_point *points, size_t max_points, size_t *n_points,
                     adsb_aircraft_record *aircraft, size_t max_aircraft, size_t *n_aircraft);

/*
 * Persistent aircraft table on the device: the reference keeps ONE HashMap<u32, Aircraft> for the life of its
 * display thread (src/adsb/tui.rs:22-42, src/adsb/web.rs:115) and pairs an even and an odd position message up to
 * 10 s apart (aircraft.rs:62-95) -- far longer than one 20 000-sample buffer (10 ms at 2 MSPS).  A table applies
 * ordered frame lists one after the other with handle_aircraft_update semantics (aircraft.rs:48-111,158-165):
 * cutting one list into any sequence of updates gives the same points and the same final table, and one update
 * on an empty table gives what adsb_track_device gives on the same list.  Packet time = (sample_base + frame
 * offset) x seconds_per_sample: with a feed in per-buffer mode (carry = 0) sample_base is adsb_feed_pop's
 * *first_sample; with carry = 1 (absolute offsets) it is 0.  That time is ONE f64 value, the u64 sum converted to
 * f64 and multiplied once, each step rounded to nearest; the 10 s window compares two such rounded times
 * (too old iff |t_i - t_j| > 10.0, aircraft.rs:68-70), whether the partner is in the same update or in the table
 * from an earlier one, so at any sample period (0.5e-6 as well as 2^-20) partners exactly round(10 /
 * seconds_per_sample) samples apart pair wherever that difference of rounded products is not above 10.0, and every
 * cut of a list gives the same bytes at that boundary too.  Frames with equal offsets are applied in list order.
 * One table per receiver (an update takes one ordered list).  Aircraft stay until adsb_track_table_expire evicts them (the reference's map is unbounded and never does;
 * this one has max_aircraft places) or until reset.  The table costs 64 MiB of device memory for its ICAO index plus
 * 136 bytes per aircraft of max_aircraft (a 128-byte record and 8 bytes of expire scratch) and about 100 bytes per
 * frame of max_frames.  The ctx must outlive the table; like the ctx, a table is not thread-safe.
 */
#define ADSB_TRACK_UNTRACKED 0x2u  /* point flag: this frame's aircraft was not admitted (table full); only icao valid */
#define ADSB_TRACK_TABLE_FULL 0x1u /* table flag: some aircraft was turned away since create / reset                  */
typedef struct adsb_track_table adsb_track_table;
typedef struct adsb_track_table_cfg {
    uint32_t abi_version;        /* ADSB_ABI_VERSION                                                           */
    uint32_t max_aircraft;       /* distinct ICAO addresses kept until reset; 0: 65536; at most 2^24            */
    uint64_t max_frames;         /* longest frame list one update accepts (1 .. 2^32 - 1)                       */
    double   seconds_per_sample; /* packet time = (sample_base + frame.offset) x this; 0.5e-6 at 2 MSPS         */
} adsb_track_table_cfg;
int adsb_track_table_create(adsb_ctx *ctx, const adsb_track_table_cfg *cfg, adsb_track_table **out_table);
void adsb_track_table_destroy(adsb_track_table *table);
/* Empties the map and clears the flags (ordered after the table's last update). */
int adsb_track_table_reset(adsb_track_table *table);
/*
 * Applies one ordered frame list (ascending offset).  `frames` is host memory or device memory of the ctx's
 * device (e.g. adsb_result_device after adsb_fetch_counts).  Host frames have been copied when this returns; the
 * kernels run asynchronously on the ctx stream, ordered after the ctx's last launch.  New ICAO addresses of one
 * update are admitted in ascending order while the table has room; the frames of the others get
 * ADSB_TRACK_UNTRACKED and the table ADSB_TRACK_TABLE_FULL.  ADSB_E_CAPACITY for n > max_frames.
 */
int adsb_track_table_update(adsb_track_table *table, const adsb_frame *frames, size_t n, uint64_t sample_base);
/* Waits; one point per frame of the LAST update, in its order (ADSB_E_STATE before any update). */
int adsb_track_table_fetch_points(adsb_track_table *table, adsb_track_point *points, size_t max_points,
                                  size_t *n_points);
/* Waits; the whole table in ascending ICAO (n_frames = frames since create / reset); *n_aircraft = table size even
 * if it exceeds max_aircraft; *flags (optional) = ADSB_TRACK_TABLE_FULL or 0. */
int adsb_track_table_fetch(adsb_track_table *table, adsb_aircraft_record *aircraft, size_t max_aircraft,
                           size_t *n_aircraft, uint32_t *flags);
/*
 * Expiry.  An aircraft's LAST HEARD time is (sample_base + offset) x seconds_per_sample of the last frame of ANY kind
 * that an update applied to it (UNTRACKED frames do not count); unlike last_contact (position messages only, NaN
 * without one) every admitted aircraft has one.
 * adsb_track_table_expire evicts every aircraft with last_heard < before (strictly older).  An evicted aircraft is
 * gone as if it had never been admitted: heard again, it is admitted as a new aircraft (ascending-ICAO rule) with no
 * CPR halves, callsign or altitude, n_frames = 0 and last_contact NaN, so a frame no longer pairs with a CPR half
 * held from before the eviction.  The freed places are room again: afterwards the table size is the survivors.
 * Asynchronous: it runs on the ctx stream after the table's last update, the next update sees its result, and it
 * never waits for the device.  It does not clear ADSB_TRACK_TABLE_FULL (that means "since create / reset"; only reset
 * clears it) and does not change what fetch_points returns for the last update.  -INFINITY evicts nothing, INFINITY
 * everything.  ADSB_E_ARG for a NULL table or a NaN before.
 */
int adsb_track_table_expire(adsb_track_table *table, double before);
/* Waits; one last-heard time (seconds) per record, in exactly the order adsb_track_table_fetch returns the records;
 * *n = table size even if it exceeds max.  ADSB_E_ARG for a NULL table, or NULL last_heard with max > 0. */
int adsb_track_table_fetch_last_heard(adsb_track_table *table, double *last_heard, size_t max, size_t *n);
/*
 * Airborne velocity.  Every record also keeps its aircraft's last airborne-velocity message (DF17 TC 19, subtype
 * 1-4; the reference decodes none and prints "n/a" in its Velocity column).  ME bit 0 is the top bit of frame byte
 * 4 (TC = ME bits 0-4, ST = 5-7); k = 4 for ST 2 and 4 (supersonic), else 1.
 *   ST 1-2: Dew 13, Vew 14-23, Dns 24, Vns 25-34.  Vew != 0 and Vns != 0: v_ew = +-(Vew - 1) k (- if Dew), v_ns
 *           likewise, speed = sqrt(v_ew^2 + v_ns^2) (SPEED); if speed > 0 also direction = atan2(v_ew, v_ns) in
 *           degrees, [0, 360) (DIRECTION).
 *   ST 3-4: status 13, heading 14-23, type 24, airspeed 25-34.  status = 1: direction = heading x 360 / 1024
 *           (DIRECTION); airspeed != 0: speed = (airspeed - 1) k, airspeed_tas = type (SPEED).
 *   ST 1-4: VrSrc 35, Svr 36, Vr 37-45.  Vr != 0: vertical_rate = +-(Vr - 1) x 64 (- if Svr), vrate_baro = VrSrc
 *           (VRATE).
 * ST 0 and 5-7 are no velocity message: the record keeps what it had.  f64 arithmetic, rounded once to f32.  The
 * newest such message of an update wins; an admitted (or re-admitted, after expire) aircraft starts with none.
 */
#define ADSB_VELOCITY_SPEED     0x1u /* speed_kt holds a value          */
#define ADSB_VELOCITY_DIRECTION 0x2u /* direction_deg holds a value     */
#define ADSB_VELOCITY_VRATE     0x4u /* vertical_rate_fpm holds a value */
typedef struct adsb_velocity {  /* an aircraft's last airborne-velocity message (DF17 TC 19, subtype 1-4), 32 bytes */
    double   time;              /* seconds: the table's frame time of that message; NaN if none yet            */
    float    speed_kt;          /* ST 1-2: ground speed; ST 3-4: airspeed; 0 unless ADSB_VELOCITY_SPEED        */
    float    direction_deg;     /* ST 1-2: track over ground [0, 360); ST 3-4: heading; 0 unless ..._DIRECTION  */
    int32_t  vertical_rate_fpm; /* positive = climbing; 0 unless ADSB_VELOCITY_VRATE                            */
    int16_t  v_ew_kt, v_ns_kt;  /* ST 1-2 with SPEED: signed components, east and north positive; else 0          */
    uint8_t  subtype;           /* 1-4; 0 = no velocity message since admission                                */
    uint8_t  flags;             /* ADSB_VELOCITY_*                                                              */
    uint8_t  vrate_baro;        /* 1 = barometric vertical rate, 0 = GNSS (only with VRATE)                     */
    uint8_t  airspeed_tas;      /* ST 3-4 with SPEED: 1 = true airspeed, 0 = indicated                          */
    uint32_t reserved;          /* 0 */
} adsb_velocity;
/* Waits; one velocity per record, in exactly the order adsb_track_table_fetch returns the records; *n = table size
 * even if it exceeds max.  ADSB_E_ARG for a NULL table, or NULL velocity with max > 0. */
int adsb_track_table_fetch_velocity(adsb_track_table *table, adsb_velocity *velocity, size_t max, size_t *n);

/*
 * A bank of persistent tables, one per receiver: what N display threads hold, one HashMap<u32, Aircraft> each
 * (src/adsb/tui.rs:22-42, web.rs:115), for a ctx that batches N receivers into one multi-channel launch.  Receiver r
 * behaves exactly like an adsb_track_table of its own with the bank's max_aircraft and seconds_per_sample, fed
 * receiver r's part of every update with sample_base[r]: its points and records are bit-identical to that table's,
 * also when the same ICAO is active on several receivers at once.  One update applies every receiver's part with one
 * dispatch sequence (the table's: field decode, sort by receiver << 24 | icao, lookup, admission, pairs, merge).
 * New ICAO addresses are admitted per receiver in ascending order while that receiver has room; a full receiver sets
 * ADSB_TRACK_TABLE_FULL for itself and marks its turned-away frames ADSB_TRACK_UNTRACKED.  Device memory: 136 bytes
 * per record of n_receivers x max_aircraft (128 of record, 8 of expire scratch), 8 bytes per entry of a hash of
 * (receiver, ICAO) with the next power of two >= 2 x n_receivers x max_aircraft entries, about 120 bytes per frame of
 * max_frames (64 receivers x 65536 aircraft: 512 MiB of records + 32 MiB of expire scratch + 64 MiB of hash).  The
 * ctx must outlive the bank; a bank is not thread-safe.
 */
typedef struct adsb_track_bank adsb_track_bank;
typedef struct adsb_track_bank_cfg {
    uint32_t abi_version;        /* ADSB_ABI_VERSION                                                           */
    uint32_t n_receivers;        /* 1 .. 256                                                                   */
    uint32_t max_aircraft;       /* PER RECEIVER, kept until reset; 0: 65536; at most 2^24                     */
    uint32_t reserved;           /* 0                                                                          */
    uint64_t max_frames;         /* longest list one update accepts, all receivers together (1 .. 2^32 - 1)   */
    double   seconds_per_sample; /* frame time of receiver r = (sample_base[r] + offset) x this                */
} adsb_track_bank_cfg;
int adsb_track_bank_create(adsb_ctx *ctx, const adsb_track_bank_cfg *cfg, adsb_track_bank **out_bank);
void adsb_track_bank_destroy(adsb_track_bank *bank);
/* Empties every receiver and clears the flags (ordered after the bank's last update). */
int adsb_track_bank_reset(adsb_track_bank *bank);
/*
 * Applies one multi-receiver list: receiver 0's frames in ascending offset, then receiver 1's, ... (adsb_fetch's
 * layout).  counts[n_receivers] (host) must sum to n (NULL only with n = 0); sample_base[n_receivers] (host, NULL: all
 * 0) times receiver r's frames.  `frames` in host memory (copied when this returns) or on the ctx's device; kernels
 * run asynchronously on the ctx stream.  ADSB_E_CAPACITY for n > max_frames.
 */
int adsb_track_bank_update(adsb_track_bank *bank, const adsb_frame *frames, size_t n, const uint64_t *counts,
                           const uint64_t *sample_base);
/*
 * Applies the ctx's last launch, channel k -> receiver k (receivers at or above its channel count get no frames):
 * exactly the frames and per-channel split adsb_fetch / per_channel_counts would return for max_out = the ctx's
 * (same header sync and slot-pool repair as adsb_fetch_counts), read in device memory.  sample_base as for update.
 * ADSB_E_ARG if the launch had more channels than the bank has receivers; ADSB_E_STATE before any launch.
 */
int adsb_track_bank_update_launch(adsb_track_bank *bank, const uint64_t *sample_base);
/* Waits; one point per frame of the LAST update, in its list order (ADSB_E_STATE before any update). */
int adsb_track_bank_fetch_points(adsb_track_bank *bank, adsb_track_point *points, size_t max_points,
                                 size_t *n_points);
/* Waits; every receiver's records, receiver 0 first, each in ascending ICAO, up to max_aircraft in all;
 * per_receiver_counts[n_receivers] (optional) = records of each receiver in `aircraft`; *n_aircraft = records held
 * in total even if more than max_aircraft; flags[n_receivers] (optional) = ADSB_TRACK_TABLE_FULL or 0 each. */
int adsb_track_bank_fetch(adsb_track_bank *bank, adsb_aircraft_record *aircraft, size_t max_aircraft,
                          size_t *n_aircraft, uint64_t *per_receiver_counts, uint32_t *flags);
/* adsb_track_table_expire for every receiver r with its own cut before[n_receivers] (host; -INFINITY: keep all):
 * receiver r stays bit-identical to a table of its own given the same updates and the same expire calls.  Per
 * receiver, the size becomes the survivors and the flag is kept.  ADSB_E_ARG for a NULL bank or before array, or a NaN
 * in it. */
int adsb_track_bank_expire(adsb_track_bank *bank, const double *before);
/* Waits; one last-heard time per record, in exactly the order adsb_track_bank_fetch returns the records; *n = records
 * held in total even if more than max.  ADSB_E_ARG for a NULL bank, or NULL last_heard with max > 0. */
int adsb_track_bank_fetch_last_heard(adsb_track_bank *bank, double *last_heard, size_t max, size_t *n);
/* Waits; one velocity (adsb_track_table_fetch_velocity) per record, in exactly the order adsb_track_bank_fetch
 * returns the records; *n = records held in total even if more than max.  ADSB_E_ARG for a NULL bank, or NULL
 * velocity with max > 0. */
int adsb_track_bank_fetch_velocity(adsb_track_bank *bank, adsb_velocity *velocity, size_t max, size_t *n);

/*
 * The fused view of a bank: ONE picture of what all receivers hear, each aircraft (ICAO address) once, in ascending
 * ICAO, computed and kept on the device.  A record of receiver r CONTRIBUTES iff it is held (what adsb_track_bank_fetch
 * would return) and its last_heard >= since (the complement of expire's last_heard < before: fuse(since = t) is
 * fuse(-INFINITY) after an expire with before[r] = t for every r).  Every quantity of a fused record comes whole from
 * ONE contributing record, copied bit for bit, never averaged or recomputed; the *_receiver fields name that receiver:
 *   last_heard:                          the greatest last_heard;
 *   last_contact, altitude:              the greatest last_contact among records whose last_contact is not NaN;
 *   latitude, longitude, position_time:  the greatest last_contact among records with has_position.  A record keeps no
 *                                        time of its fix (its position can be older than its last_contact, when its
 *                                        newest position message completed no pair), so position_time is that record's
 *                                        last_contact and is named for what it is;
 *   callsign:                            among records whose callsign has a non-zero byte, the greatest last_heard (a
 *                                        record keeps no time of its identification message);
 *   velocity (the eleven fields from velocity_time to velocity_reserved: an adsb_velocity bit for bit, in its order):
 *                                        among records with subtype != 0, the greatest time.
 * Every tie goes to the lowest receiver index; nothing depends on hash placement, atomics or scheduling, so two calls
 * on the same bank give the same bytes.  n_frames is the sum and n_receivers the count over the contributing records
 * (n_frames counts receptions: a message heard by three receivers counts three times).  Times of different receivers
 * are compared as stored, (sample_base[r] + offset) x seconds_per_sample: they are on one clock only if the caller's
 * sample_base values are.  An even message of one receiver is never paired with an odd one of another.
 * The bank is only read: no record, size, flag or point changes.  Device memory, all of it allocated by
 * adsb_track_bank_fuse_reserve and none before: per place of n_receivers x max_aircraft 16 bytes of sort keys and
 * values (24 with more than 128 receivers) plus rocPRIM's sort scratch (about 8 more), and 132 bytes per record of
 * max_fused (64 receivers x 65536 aircraft: 64 MiB + 33.75 MiB, and 8.25 MiB for max_fused = 65536: 106 MiB measured;
 * 626 MiB with max_fused = 0).
 */
#define ADSB_FUSED_NONE 0xFFFFu            /* a *_receiver field: no contributing record has that quantity           */
#define ADSB_TRACK_FUSED_TRUNCATED 0x1u    /* more distinct ICAOs than max_fused: the lowest max_fused ICAOs are kept */
typedef struct adsb_fused_aircraft {  /* 128 bytes, one per distinct ICAO, ascending ICAO */
    double   latitude, longitude;     /* of position_receiver's record; 0 unless has_position                        */
    double   position_time;           /* last_contact of position_receiver's record; NaN unless has_position         */
    double   last_contact;            /* of contact_receiver's record; NaN if none                                    */
    double   last_heard;              /* of heard_receiver's record                                                   */
    uint64_t n_frames;                /* sum of the contributing records' n_frames                                    */
    uint32_t icao;
    int32_t  altitude;                /* of contact_receiver's record; 0 if none                                      */
    uint16_t n_receivers;             /* contributing receivers, 1 .. 256                                             */
    uint16_t heard_receiver;          /* whose last_heard that is                                                     */
    uint16_t contact_receiver;        /* whose last_contact and altitude; ADSB_FUSED_NONE                             */
    uint16_t position_receiver;       /* whose latitude, longitude and position_time; ADSB_FUSED_NONE                 */
    uint16_t callsign_receiver;       /* whose callsign; ADSB_FUSED_NONE                                              */
    uint16_t velocity_receiver;       /* whose velocity; ADSB_FUSED_NONE                                              */
    uint32_t has_position;
    char     callsign[8];             /* zeros if none                                                                */
    double   velocity_time;           /* offset 80: adsb_velocity.time (NaN if none) ...                              */
    float    speed_kt;
    float    direction_deg;
    int32_t  vertical_rate_fpm;
    int16_t  v_ew_kt, v_ns_kt;
    uint8_t  velocity_subtype;        /* adsb_velocity.subtype; 0 if none (then the flags are 0 and the rest 0 too)   */
    uint8_t  velocity_flags;          /* adsb_velocity.flags: ADSB_VELOCITY_*                                         */
    uint8_t  vrate_baro;
    uint8_t  airspeed_tas;
    uint32_t velocity_reserved;       /* ... adsb_velocity.reserved, offset 108                                       */
    uint64_t reserved[2];             /* 0 */
} adsb_fused_aircraft;
/* Allocates (or, called again, resizes) what adsb_track_bank_fuse needs for up to max_fused fused records; 0: the worst
 * case n_receivers x max_aircraft (every record a different ICAO: 512 MiB of output for 64 x 65536, so name a figure).
 * May wait for the device.  A bank that never reserves allocates nothing and behaves exactly as before.  ADSB_E_ARG for
 * a NULL bank, ADSB_E_NOMEM if the memory is not to be had (an earlier reserve is then gone too). */
int adsb_track_bank_fuse_reserve(adsb_track_bank *bank, size_t max_fused);
/* Computes the fused view of the records with last_heard >= since (-INFINITY: all held records; INFINITY: none).
 * Asynchronous: one dispatch sequence on the ctx stream after the bank's last update / expire / reset (keys, rocPRIM
 * radix sort by ICAO then receiver, scan of the ICAO changes, one reduction per ICAO); it never waits for the device
 * and copies nothing from or to the host.  ADSB_E_ARG for a NULL bank or a NaN since, ADSB_E_STATE without a reserve. */
int adsb_track_bank_fuse(adsb_track_bank *bank, double since);
/* Waits; copies min(records written, max) records of the last fuse, ascending ICAO; *n (optional) = records copied,
 * *n_total (optional) = distinct ICAOs even when they exceed max_fused, *flags (optional) then has
 * ADSB_TRACK_FUSED_TRUNCATED.  ADSB_E_ARG for a NULL bank, or NULL out with max > 0; ADSB_E_STATE before any fuse
 * (since the last reserve). */
int adsb_track_bank_fetch_fused(adsb_track_bank *bank, adsb_fused_aircraft *out, size_t max, size_t *n,
                                size_t *n_total, uint32_t *flags);
/* Does not synchronise: device pointers to the fused records and to two words, counts_dev[0] = records written,
 * counts_dev[1] = distinct ICAOs, both valid on the ctx stream after the last fuse, until the next fuse or reserve.
 * Either pointer argument may be NULL.  ADSB_E_STATE before any fuse. */
int adsb_track_bank_fused_device(adsb_track_bank *bank, const adsb_fused_aircraft **fused_dev,
                                 const uint64_t **counts_dev);

/*
 * Per-frame summaries and the changed list: what the reference's web thread emits.  It calls handle_aircraft_update for
 * every packet and broadcasts that aircraft's AircraftSummary as it stands right after that packet (src/adsb/web.rs:
 * 117-128, aircraft.rs:141-149,158-165).  With a reserve, every update of a table or bank also leaves, on the device,
 *   (1) one adsb_aircraft_record per frame of that update, in its list order (the order of fetch_points): the frame's
 *       aircraft as Aircraft::handle_packet (aircraft.rs:48-111) leaves it after that frame, starting from the record
 *       the table held before the update (an empty one for an aircraft this update admits, also after an expire):
 *         callsign:                of the last identification message at or before the frame, else the record's;
 *         altitude, last_contact:  of the last position message at or before it, else the record's;
 *         latitude, longitude, has_position: of the last frame at or before it whose point has
 *                                  ADSB_TRACK_NEW_POSITION, else the record's;
 *         n_frames:                the record's count plus the aircraft's frames of this update up to and including it;
 *       a frame whose point is ADSB_TRACK_UNTRACKED gets its icao and otherwise an empty record (zeros, last_contact
 *       NaN, n_frames 0).  The expressions are the merge's, so bit for bit: the summary at an aircraft's last frame of
 *       an update is its record as fetch returns it after the update; a list cut into any sequence of updates gives,
 *       concatenated, the summaries of one update; receiver r's part of a bank's equals a table's of its own;
 *   (2) the changed list: the record slots of the distinct aircraft the update applied at least one frame to (UNTRACKED
 *       ones excluded), in ascending ICAO (bank: receiver 0's, then receiver 1's, ...), and their number.
 * Both come from one more scan over the sorted list (a segmented maximum of "sorted position of the last writer" per
 * quantity, rocPRIM) and one kernel with a thread per frame, between the pairs step and the merge: linear in the list
 * however long one aircraft's part is, no atomics, two runs give the same bytes.  Asynchronous on the ctx stream like
 * the rest of the update.  Device memory, all of it allocated by the reserve and none before: 72 bytes per frame of
 * max_frames (48 of summary, 20 of scan values, 4 of changed list) plus rocPRIM's scan scratch, and 128 bytes per
 * record of min(max_frames, max_aircraft x receivers) for fetch_changed's gather.  A table or bank that never reserves
 * allocates nothing, launches exactly the kernels it launched before and behaves as before.
 */
/* Allocates the above; from then on every update also computes the summaries and the changed list.  May wait for the
 * device.  A second reserve changes nothing.  ADSB_E_ARG for a NULL table, ADSB_E_NOMEM if the memory is not to be
 * had. */
int adsb_track_table_summaries_reserve(adsb_track_table *table);
/* Waits; copies min(*n, max) summaries of the LAST update, *n (optional) = its frames.  ADSB_E_STATE without a reserve,
 * or before any update since the reserve or the last reset; ADSB_E_ARG for a NULL table, or NULL out with max > 0.
 * Like fetch_points, a later expire does not change what it returns. */
int adsb_track_table_fetch_summaries(adsb_track_table *table, adsb_aircraft_record *out, size_t max, size_t *n);
/* Does not synchronise: the device address of the summaries, valid on the ctx stream after the last update until the
 * next one (as many as that update had frames).  Same ADSB_E_STATE / ADSB_E_ARG rules; dev may be NULL. */
int adsb_track_table_summaries_device(adsb_track_table *table, const adsb_aircraft_record **dev);
/* Waits; the aircraft the last update touched, ascending ICAO, each with its record, last-heard time and velocity
 * exactly as adsb_track_table_fetch, _fetch_last_heard and _fetch_velocity would return for it now, byte for byte; any
 * of the three arrays may be NULL; min(*n, max) entries are written, *n (optional) = how many there are.  The records
 * are gathered on the device and only they are copied (the table is neither copied nor sorted).  Valid while the last
 * operation on the table was that update: ADSB_E_STATE after an expire or reset (slots move) until the next update,
 * and without a reserve or an update since it.  ADSB_E_ARG for a NULL table. */
int adsb_track_table_fetch_changed(adsb_track_table *table, adsb_aircraft_record *rec, double *last_heard,
                                   adsb_velocity *velocity, size_t max, size_t *n);
/* The same for a bank: summaries in the update's list order (receiver 0's frames, then receiver 1's, ...), the changed
 * list receiver by receiver, each in ascending ICAO; per_receiver_counts[n_receivers] (optional) = entries of each
 * receiver among those written. */
int adsb_track_bank_summaries_reserve(adsb_track_bank *bank);
int adsb_track_bank_fetch_summaries(adsb_track_bank *bank, adsb_aircraft_record *out, size_t max, size_t *n);
int adsb_track_bank_summaries_device(adsb_track_bank *bank, const adsb_aircraft_record **dev);
int adsb_track_bank_fetch_changed(adsb_track_bank *bank, adsb_aircraft_record *rec, double *last_heard,
                                  adsb_velocity *velocity, size_t max, size_t *n, uint64_t *per_receiver_counts);

/*
 * Per-aircraft signal levels: the per-frame power statistics (adsb_frame_level) kept per aircraft, beside its record.
 * With a levels reserve a table or bank holds one 64-byte adsb_aircraft_level per record place, and the *_levels
 * forms of update merge a list's level records into them.  Frame j of an update is COUNTED for its aircraft iff its
 * point is not ADSB_TRACK_UNTRACKED and levels[j].flags has ADSB_LEVEL_VALID.  Over an aircraft's counted frames:
 *   signal_total, noise_total, weak_bits_total, n_levels: sums that SATURATE at the field's maximum (2^64 - 1,
 *       2^32 - 1) and stay there;
 *   max_signal_sum, peak: maxima (exact, also once a total has saturated);
 *   last_signal_sum, last_noise_sum, last_time: of the NEWEST counted frame, the last one in list order (frames with
 *       equal offsets are applied in list order, as for the merge); last_time is the store's frame time of that frame,
 *       (sample_base + offset) x seconds_per_sample, the same single rounded product as every other time of the store.
 * An EMPTY level record is all zeros with last_time NaN.  An aircraft's is empty at admission, at re-admission after
 * an expire, after a reset, and while the store held the aircraft from before the reserve, until its next counted
 * frame.  Expire moves a survivor's level record with its record.  Every field combines by an associative,
 * commutative rule (saturating add, max, newest by position), so the records are bit-exact whatever shape the
 * reduction takes: one list (frames and levels alike) cut into any sequence of updates gives the same 64 bytes per
 * aircraft, receiver r of a bank equals a table of its own, and two runs give the same bytes.  The mean signal power
 * of an aircraft is signal_total / (116 x n_levels); once signal_total has saturated that mean is a LOWER BOUND.
 * On the device: after the pairs step, one segmented inclusive scan over the sorted list (rocPRIM, a 48-byte tuple
 * computed where the scan loads it) and one thread per segment tail that merges into the side record: linear in the
 * list however long one aircraft's part is, no atomics.  Device memory, all of it allocated by the reserve and none
 * before: 64 bytes per place of n_receivers x max_aircraft, and per frame of max_frames 32 bytes of device staging
 * for a host levels array, 48 bytes of scan values plus rocPRIM's scan scratch; 32 bytes per frame of pinned host
 * memory (64 receivers x 65536 aircraft: 256 MiB of level records).  A table or bank that never reserves allocates
 * nothing, launches exactly the kernels it launched before and returns the same bytes; the plain update of a store
 * that did reserve behaves as before too and leaves the level records alone (apart from admission emptying a place).
 * fetch_changed and the per-frame summaries carry no levels.
 */
typedef struct adsb_aircraft_level {  /* 64 bytes, one per record place, beside the 128-byte record */
    uint64_t signal_total;     /* saturating sum of signal_sum over the counted frames            */
    uint64_t noise_total;      /* saturating sum of noise_sum                                     */
    uint64_t last_signal_sum;  /* of the newest counted frame                                     */
    uint64_t last_noise_sum;
    uint64_t max_signal_sum;   /* greatest signal_sum of a counted frame                          */
    double   last_time;        /* the store's frame time of the newest counted frame; NaN if none */
    uint32_t n_levels;         /* counted frames, saturating                                      */
    uint32_t peak;             /* max of peak over the counted frames                             */
    uint32_t weak_bits_total;  /* saturating sum of weak_bits                                     */
    uint32_t reserved;         /* 0 */
} adsb_aircraft_level;
/* Allocates the above and empties every level record.  May wait for the device.  A second reserve changes nothing.
 * ADSB_E_ARG for a NULL table, ADSB_E_NOMEM if the memory is not to be had. */
int adsb_track_table_levels_reserve(adsb_track_table *table);
/* adsb_track_table_update plus the level merge: points, records, summaries and the changed list are byte for byte what
 * update gives on the same frames.  levels[n] is the frames' level records in list order; `frames` and `levels` may
 * each be host memory or memory of the ctx's device, independently; host arrays have been copied when this returns.
 * A table's path from a launch: adsb_result_device (after adsb_fetch_counts) and adsb_levels_device (after
 * adsb_levels_device_async) give the two device arrays.  A feed's consumer passes adsb_host_frame_levels output as a
 * host array.  ADSB_E_ARG for a NULL table, or NULL frames or levels with n > 0; ADSB_E_STATE without a reserve;
 * ADSB_E_CAPACITY for n > max_frames; n = 0 is ADSB_OK. */
int adsb_track_table_update_levels(adsb_track_table *table, const adsb_frame *frames, const adsb_frame_level *levels,
                                   size_t n, uint64_t sample_base);
/* Waits; one level record per aircraft, in exactly the order adsb_track_table_fetch returns the records (ascending
 * ICAO); *n = records held even if more than max.  ADSB_E_ARG for a NULL table, or NULL out with max > 0;
 * ADSB_E_STATE without a reserve. */
int adsb_track_table_fetch_levels(adsb_track_table *table, adsb_aircraft_level *out, size_t max, size_t *n);
/* Does not synchronise: the device address of the level records, one per record PLACE (max_aircraft of them; a bank:
 * receiver r's at [r x max_aircraft, (r + 1) x max_aircraft)), in slot order, which is admission order and not ICAO
 * order, for consumers that stay on the GPU; valid on the ctx stream for the life of the store.  dev may be NULL.
 * ADSB_E_ARG for a NULL table, ADSB_E_STATE without a reserve. */
int adsb_track_table_levels_device(adsb_track_table *table, const adsb_aircraft_level **dev);
/* The same for a bank; fetch_levels receiver by receiver, each in ascending ICAO, as adsb_track_bank_fetch. */
int adsb_track_bank_levels_reserve(adsb_track_bank *bank);
int adsb_track_bank_update_levels(adsb_track_bank *bank, const adsb_frame *frames, const adsb_frame_level *levels,
                                  size_t n, const uint64_t *counts, const uint64_t *sample_base);
/* adsb_track_bank_update_launch with the ctx's levels of the same launch: enqueues adsb_levels_device_async itself if
 * the ctx's levels are not those of the last launch, and again for the rebuilt list when the header sync rebuilt it
 * (slot-pool overflow), as adsb_fetch_levels does.  Errors of the levels call are passed through.  ADSB_E_STATE
 * without a reserve or before any launch. */
int adsb_track_bank_update_launch_levels(adsb_track_bank *bank, const uint64_t *sample_base);
int adsb_track_bank_fetch_levels(adsb_track_bank *bank, adsb_aircraft_level *out, size_t max, size_t *n);
int adsb_track_bank_levels_device(adsb_track_bank *bank, const adsb_aircraft_level **dev);
/*
 * Fused levels.  A bank with both a fuse reserve and a levels reserve also computes, in adsb_track_bank_fuse, one
 * adsb_fused_level per fused record, in the same order (under truncation: for the written records only), over the same
 * contributing records.  The STRONGEST receiver is the one with the greatest mean signal signal_total / n_levels among
 * the contributing records with n_levels > 0, compared exactly by cross-multiplication (a.signal_total x b.n_levels
 * against b.signal_total x a.n_levels, 96-bit integer products, no floating point); ties go to the lowest receiver.  A
 * saturated signal_total makes that record's mean a lower bound, and it is compared as such.  The array of max_fused
 * records (96 bytes each) is allocated by whichever of the two reserves comes second; a repeated fuse_reserve resizes
 * it.  The 128-byte fused records are what they are without a levels reserve.  A kernel of its own after the fuse's
 * reduction, one thread per fused record over the sorted places.
 */
typedef struct adsb_fused_level {     /* 96 bytes, one per fused record, same order */
    /* the first ten fields are strongest_receiver's adsb_aircraft_level, bit for bit and in its order (offset 0); an
     * empty one if none */
    uint64_t strongest_signal_total;
    uint64_t strongest_noise_total;
    uint64_t strongest_last_signal_sum;
    uint64_t strongest_last_noise_sum;
    uint64_t strongest_max_signal_sum;
    double   strongest_last_time;
    uint32_t strongest_n_levels;
    uint32_t strongest_peak;
    uint32_t strongest_weak_bits_total;
    uint32_t strongest_reserved;
    uint64_t signal_total, noise_total; /* saturating sums over the contributing records               */
    uint64_t n_levels;                /* sum of their n_levels                                         */
    uint16_t strongest_receiver;      /* ADSB_FUSED_NONE if no contributing record has n_levels > 0    */
    uint16_t level_receivers;         /* contributing records with n_levels > 0                        */
    uint32_t reserved;                /* 0 */
} adsb_fused_level;
/* Waits; copies min(records written, max) level records of the last fuse; *n (optional) = records written by that fuse
 * even if more than max.  ADSB_E_ARG for a NULL bank, or NULL out with max > 0; ADSB_E_STATE if the last fuse computed
 * no levels: no fuse yet (since the last fuse reserve), or one of the two reserves was missing when it ran. */
int adsb_track_bank_fetch_fused_levels(adsb_track_bank *bank, adsb_fused_level *out, size_t max, size_t *n);

/*
 * Positions from single messages, relative to the receiver site.  The records' position needs an even and an odd
 * airborne message within 10 s (the reference's calculate_geographic_position).  With a fixes reserve a table or bank
 * also decodes every position message ON ITS OWN against the site of the receiver that heard it (the locally
 * unambiguous CPR decode), and keeps the newest such fix per aircraft in one 64-byte adsb_fix beside its record, with
 * range and bearing from the site.  That also covers what the pair decode never reports: aircraft heard with one CPR
 * format only, surface messages (TC 5-8, with ground speed and track) and airborne messages with GNSS height (TC 20-22).
 *
 * A frame is a POSITION MESSAGE if DF = 17 and TC is 5-8 (surface), 9-18 or 20-22 (airborne).  With ME bit 0 the top
 * bit of frame byte 4: F (odd) = ME bit 21, lat_cpr = ME bits 22-38, lon_cpr = ME bits 39-55.  y = lat_cpr / 2^17,
 * x = lon_cpr / 2^17, span = 360 (airborne) or 90 (surface), i = F, mod(a, b) = a - b floor(a / b), site (lat_s, lon_s):
 *     dLat = span / (60 - i)
 *     j    = floor(lat_s / dLat) + floor(0.5 + mod(lat_s, dLat) / dLat - y)
 *     lat  = dLat (j + y)
 *     dLon = span / max(NL(lat) - i, 1)                NL: the number of longitude zones (cpr.rs:39-54)
 *     m    = floor(lon_s / dLon) + floor(0.5 + mod(lon_s, dLon) / dLon - x)
 *     lon  = dLon (m + x), brought into [-180, 180] (cpr.rs:27-31)
 * range = haversine distance from the site in nautical miles (R = 3440.065 NM), bearing = the initial bearing
 * atan2(sin dl cos p2, cos p1 sin p2 - sin p1 cos p2 cos dl) in degrees in [0, 360); all of it f64, each rounded to
 * f32 once.  A bearing whose rounding to f32 gives 360 is returned as 0, so bearing_deg itself lies in [0, 360).  The
 * range limit is tested on the f64 range: the f32 range_nm of an accepted frame may round up past a fractional limit
 * by half an f32 step (7.6e-6 NM at 180 NM).  The frame is REJECTED (counted in n_rejected, the fix stays) if |lat| > 90 or the range exceeds the
 * site's limit: max_range_nm for an airborne message, min(max_range_nm, 45) for a surface one.  The decode picks the
 * position nearest the site among those half a zone apart, so it is right only for aircraft within half a zone: 180 NM
 * airborne, 45 NM surface; hence max_range_nm must lie in (0, 180].
 * Surface messages: movement = ME bits 5-11: 0 and 125-127 no speed; 1: 0 kt; 2-8: 0.125 + (m - 2) 0.125; 9-12:
 * 1 + (m - 9) 0.25; 13-38: 2 + (m - 13) 0.5; 39-93: 15 + (m - 39); 94-108: 70 + (m - 94) 2; 109-123:
 * 100 + (m - 109) 5; 124: 175 kt.  ME bit 12 set: track = ME bits 13-19 x 360 / 128 degrees.  TC 9-18 carry the
 * altitude of the field decode (adsb_packet_fields.altitude); TC 20-22 carry none here (ADSB_FIX_ALT clear).
 *
 * The NEWEST accepted position message wins (the last one in list order); n_fixes and n_rejected are saturating sums
 * over the aircraft's frames since admission.  An aircraft's fix is EMPTY (time NaN, all else zero) at admission, at
 * re-admission after an expire and after a reset; expire moves a survivor's fix with its record.  A frame's decode
 * depends on the frame and the site only and the merge is associative, so one list cut into any sequence of updates
 * gives the same 64 bytes per aircraft, and receiver r of a bank equals a table with receiver r's site.
 * With a reserve every form of update (update, update_levels, update_launch*, host or device lists) also merges the
 * fixes.  On the device, after the pairs step: one thread per frame decodes from the frame bytes into one
 * adsb_frame_fix (and 16 bytes more), one segmented inclusive scan over the sorted list (rocPRIM, a 16-byte tuple:
 * head mark, later accepted position, saturating counts) and one thread per segment tail that merges into the side
 * record: linear in the list however long one aircraft's part is, no atomics.  Device memory, all of it allocated by
 * the reserve: 64 bytes per place of n_receivers x max_aircraft, 24 bytes per receiver, and 64 bytes per frame of
 * max_frames plus rocPRIM's scan scratch.  A store that never reserves allocates nothing, launches exactly the
 * kernels it launched before, and records, points, velocity, levels and summaries are the same bytes either way.  The
 * fused view carries no fixes.
 */
typedef struct adsb_site {           /* a receiver's position and how far it trusts a local decode */
    double latitude, longitude;      /* degrees, [-90, 90] and [-180, 180] */
    double max_range_nm;             /* (0, 180] */
} adsb_site;
#define ADSB_FIX_VALID    0x1u  /* the record holds a fix                          */
#define ADSB_FIX_SURFACE  0x2u  /* from a surface message (TC 5-8)                 */
#define ADSB_FIX_ALT      0x4u  /* altitude holds a value (TC 9-18)                */
#define ADSB_FIX_SPEED    0x8u  /* ground_speed_kt holds a value (surface)         */
#define ADSB_FIX_TRACK    0x10u /* track_deg holds a value (surface)               */
#define ADSB_FIX_REJECTED 0x20u /* adsb_frame_fix only: a position message turned away (then nothing else is set but
                                   ADSB_FIX_SURFACE, and the position fields are 0) */
typedef struct adsb_fix {            /* 64 bytes, one per record place, beside the 128-byte record */
    double   time;                   /* table frame time of the message this fix came from; NaN if none yet */
    double   latitude, longitude;    /* degrees */
    float    range_nm, bearing_deg;  /* from the site */
    float    ground_speed_kt, track_deg; /* surface only; 0 unless flagged */
    int32_t  altitude;               /* feet; 0 unless ADSB_FIX_ALT */
    uint32_t n_fixes, n_rejected;    /* saturating, since admission */
    uint8_t  type_code, flags, cpr_odd, reserved8;
    uint32_t reserved;               /* 0; the four bytes of padding after it are 0 too */
} adsb_fix;
typedef struct adsb_frame_fix {      /* 32 bytes, one per frame of the last update, in its order */
    double   latitude, longitude;
    float    range_nm, bearing_deg;
    uint32_t icao;
    uint32_t flags;                  /* ADSB_FIX_*; 0: no position message, or an aircraft the full table turned away */
} adsb_frame_fix;
/* Allocates the above, keeps the site and empties every fix.  Waits for the device.  On a store that holds no aircraft
 * (new, or after a reset) a repeated reserve replaces the site.  ADSB_E_ARG for a NULL table or site, a NaN in the
 * site, a latitude outside [-90, 90], a longitude outside [-180, 180] or a range outside (0, 180] (all checked before
 * the table is touched); ADSB_E_STATE if the table holds aircraft; ADSB_E_NOMEM if the memory is not to be had. */
int adsb_track_table_fixes_reserve(adsb_track_table *table, const adsb_site *site);
/* Waits; one fix per aircraft, in exactly the order adsb_track_table_fetch returns the records (ascending ICAO);
 * *n = records held even if more than max.  ADSB_E_ARG for a NULL table, or NULL out with max > 0; ADSB_E_STATE
 * without a reserve. */
int adsb_track_table_fetch_fixes(adsb_track_table *table, adsb_fix *out, size_t max, size_t *n);
/* Does not synchronise: the device address of the fixes, one per record PLACE in slot order (as
 * adsb_track_table_levels_device); dev may be NULL.  ADSB_E_ARG for a NULL table, ADSB_E_STATE without a reserve. */
int adsb_track_table_fixes_device(adsb_track_table *table, const adsb_fix **dev);
/* Waits; one adsb_frame_fix per frame of the last update, in its list order, as adsb_track_table_fetch_points: copies
 * min(frames, max), *n = copied.  ADSB_E_STATE without a reserve or before the first update. */
int adsb_track_table_fetch_frame_fixes(adsb_track_table *table, adsb_frame_fix *out, size_t max, size_t *n);
/* The same for a bank: sites[n_receivers], receiver r's frames decode against sites[r]; fetch_fixes receiver by
 * receiver, each in ascending ICAO, as adsb_track_bank_fetch. */
int adsb_track_bank_fixes_reserve(adsb_track_bank *bank, const adsb_site *sites);
int adsb_track_bank_fetch_fixes(adsb_track_bank *bank, adsb_fix *out, size_t max, size_t *n);
int adsb_track_bank_fixes_device(adsb_track_bank *bank, const adsb_fix **dev);
int adsb_track_bank_fetch_frame_fixes(adsb_track_bank *bank, adsb_frame_fix *out, size_t max, size_t *n);

/*
 * Multilaterated positions per aircraft.  adsb_multilaterate leaves one adsb_mlat_fix per correlated message; with an
 * mlat reserve a TABLE keeps them per aircraft, one 64-byte adsb_aircraft_mlat per record place beside its record, and
 * checks every position an aircraft reports against where its signal came from.  Correlate's messages as a plain
 * adsb_frame[] (adsb_correlated_device's frames_dev) and fixes[] line up index for index, and both lie in device memory.  A
 * correlated list is one merged stream, so this is for tables only: a bank has no such entry points and behaves as
 * before.
 *
 * COUNTED  Frame j of an update_mlat is counted for its aircraft iff its point is not ADSB_TRACK_UNTRACKED.  A counted
 *   frame whose fix has ADSB_MLAT_ATTEMPTED adds 1 to n_attempted, one whose fix has ADSB_MLAT_VALID adds 1 to n_valid
 *   (both saturate at 2^32 - 1 and stay there).  The NEWEST counted frame with a VALID fix is kept: the last such frame
 *   in list order (frames with equal offsets are applied in list order, as for the fix merge).  From it come latitude,
 *   longitude, height_m (rounded to f32 once), residual_rms_m, pdop, n_used, ADSB_TRACK_MLAT_ALTITUDE (the fix has
 *   ADSB_MLAT_ALTITUDE) and time, the store's frame time of that frame: (sample_base + offset) x seconds_per_sample,
 *   the same single rounded product as every other time of the store.  A fix that is not valid (TOO_FEW, SINGULAR,
 *   rejected, BAD_INDEX, ...) leaves the kept fix alone.
 * THE CHECK  A counted frame is CHECKED iff its fix is VALID, the frame is an AIRBORNE position message (DF 17, TC 9-18
 *   or 20-22; surface frames are not checked) and (fix.latitude, fix.longitude, 180 NM) is a site that
 *   adsb_track_table_fixes_reserve accepts (a NaN or a position off the globe is none).  The frame is then decoded ON
 *   ITS OWN with the solved position as the site, by "Positions from single messages" above, and disagreement_m is that
 *   decode's f64 range x 1852, rounded to f32 once.  If the decode turns the frame away (|lat| > 90, or farther than
 *   180 NM) the frame is CHECKED and FAR, its disagreement_m is 333360 (180 NM) and it disagrees.  A checked frame
 *   DISAGREES iff it is FAR or the f64 distance in metres exceeds the reserve's max_disagreement_m.  A local decode
 *   picks the position nearest its site among those a whole zone apart, so the check measures a displacement modulo
 *   the zone size (360 NM in latitude): one of a whole number of zones is not seen.  last_disagreement_m is the newest checked frame's value, max_disagreement_m (the field) the
 *   maximum over the checked frames, n_checked and n_disagree saturating sums.
 * Every field combines by an associative rule (saturating add, max, newest by position), so one list (frames and
 * fixes alike) cut into any sequence of update_mlat calls gives the same 64 bytes per aircraft, and two runs give the
 * same bytes.  An EMPTY record is all zeros with time NaN.  An aircraft's is empty at admission, at re-admission after
 * an expire, after a reset, and while the store held the aircraft from before the reserve, until its next counted
 * frame that changes it.  Expire moves a survivor's mlat record with its record.
 * On the device, after the pairs step: one thread per frame reads the frame, its fix and its slot and writes one
 * adsb_frame_mlat in list order and a 32-byte scan operand in sorted order (the f64 CPR decode and the haversine are
 * the only arithmetic), one segmented inclusive scan over the sorted list (rocPRIM; head mark, newest valid frame,
 * newest checked frame, maximum disagreement, four saturating counts: integers and one float max, no float sums) and
 * one thread per segment tail that merges into the side record: linear in the list however long one aircraft's part
 * is, no atomics.  Device memory, all of it allocated by the reserve and none before: 64 bytes per place of
 * max_aircraft, and per frame of max_frames 16 + 32 + 32 bytes plus 64 bytes of device staging for a host fixes array
 * and rocPRIM's scan scratch; 64 bytes per frame of pinned host memory.  A table that never reserves allocates
 * nothing, launches exactly the kernels it launched before and returns the same bytes; adsb_track_table_update and
 * update_levels of a table that did reserve behave as before and leave the mlat records alone (apart from admission
 * emptying a place).  fetch_changed, the per-frame summaries and a bank's fused view carry no mlat records.
 */
#define ADSB_TRACK_MLAT_VALID    0x1u  /* the record holds a fix                                     */
#define ADSB_TRACK_MLAT_ALTITUDE 0x2u  /* that fix used the message's own altitude (ADSB_MLAT_ALTITUDE) */
#define ADSB_TRACK_MLAT_CHECKED  0x4u  /* last_disagreement_m holds a value                          */
#define ADSB_TRACK_MLAT_DISAGREE 0x8u  /* adsb_frame_mlat only: this frame's disagreement exceeds the limit */
#define ADSB_TRACK_MLAT_FAR      0x10u /* adsb_frame_mlat only: the local decode was turned away (see above) */
typedef struct adsb_aircraft_mlat {   /* 64 bytes, one per record place, beside the 128-byte record */
    double   time;                  /* table frame time of the message the kept fix belongs to; NaN if none */
    double   latitude, longitude;   /* degrees, the fix's */
    float    height_m, residual_rms_m, pdop;   /* the fix's (height rounded to f32 once) */
    float    last_disagreement_m;   /* of the newest CHECKED frame; 0 unless ADSB_TRACK_MLAT_CHECKED */
    float    max_disagreement_m;    /* maximum over the checked frames since admission */
    uint32_t n_attempted, n_valid;  /* counted frames whose fix has ADSB_MLAT_ATTEMPTED / ADSB_MLAT_VALID; saturating */
    uint32_t n_checked, n_disagree; /* checked frames / those beyond the limit; saturating */
    uint16_t n_used;                /* the kept fix's */
    uint8_t  flags, reserved;       /* ADSB_TRACK_MLAT_*; 0 */
} adsb_aircraft_mlat;
typedef struct adsb_frame_mlat {      /* 16 bytes, one per frame of the last update_mlat, in its list order */
    float    disagreement_m;        /* 0 unless CHECKED */
    uint32_t icao;
    uint32_t flags;                 /* VALID (this frame's fix was valid and counted), CHECKED, DISAGREE, FAR */
    uint32_t reserved;              /* 0 */
} adsb_frame_mlat;
/* Allocates the above, keeps the limit and empties every mlat record.  May wait for the device.  A second reserve
 * changes nothing (the first limit stays).  ADSB_E_ARG for a NULL table or a max_disagreement_m that is not finite and
 * > 0 (checked before the table is touched); ADSB_E_NOMEM if the memory is not to be had. */
int adsb_track_table_mlat_reserve(adsb_track_table *table, double max_disagreement_m);
/* adsb_track_table_update plus the merge above: points, records, summaries, changed list, velocity and single-message
 * fixes are byte for byte what update gives on the same frames.  fixes[n] is the frames' fixes in list order.  With
 * levels not NULL it is also adsb_track_table_update_levels and needs the levels reserve.  frames, fixes and levels may
 * each be host memory or memory of the ctx's device, independently; host arrays have been copied when this returns.
 * ADSB_E_ARG for a NULL table, or NULL frames or fixes with n > 0; ADSB_E_STATE without an mlat reserve, or with levels
 * and no levels reserve; ADSB_E_CAPACITY for n > max_frames; n = 0 is ADSB_OK. */
int adsb_track_table_update_mlat(adsb_track_table *table, const adsb_frame *frames, const adsb_mlat_fix *fixes,
                                 const adsb_frame_level *levels /* may be NULL */, size_t n, uint64_t sample_base);
/* Waits; one mlat record per aircraft, in exactly the order adsb_track_table_fetch returns the records (ascending
 * ICAO); *n = records held even if more than max.  ADSB_E_ARG for a NULL table, or NULL out with max > 0;
 * ADSB_E_STATE without a reserve. */
int adsb_track_table_fetch_mlat(adsb_track_table *table, adsb_aircraft_mlat *out, size_t max, size_t *n);
/* Does not synchronise: the device address of the mlat records, one per record PLACE in slot order (as
 * adsb_track_table_levels_device); dev may be NULL.  ADSB_E_ARG for a NULL table, ADSB_E_STATE without a reserve. */
int adsb_track_table_mlat_device(adsb_track_table *table, const adsb_aircraft_mlat **dev);
/* Waits; one adsb_frame_mlat per frame of the last update_mlat, in its list order: copies min(frames, max), *n =
 * copied.  A frame of an aircraft the full table turned away has its icao and nothing else.  ADSB_E_ARG for a NULL
 * table, or NULL out with max > 0; ADSB_E_STATE without a reserve or before the first update_mlat (since a reset). */
int adsb_track_table_fetch_frame_mlat(adsb_track_table *table, adsb_frame_mlat *out, size_t max, size_t *n);

/*
 * Filtered mlat track per aircraft.  A single multilaterated fix scatters by hdop x 30..100 m, one wild fix would be the
 * aircraft's position until the next, and an aircraft without ADS-B has no velocity at all.  With a FILTER reserve
 * (beside the mlat reserve it needs) every update that merges fixes (update_mlat, and update_modes / update_commb /
 * update_es given fixes) also runs each aircraft's fixes, in list order, through a small Kalman filter whose state is one
 * 192-byte adsb_aircraft_filter per record place.  Tables only.  The definition is this project's own.
 *
 * PER FRAME, THE OPERAND (adsb_filter_operand, 64 bytes).  A frame is USABLE iff it is counted (its point is not
 *   ADSB_TRACK_UNTRACKED, and for update_modes its address is an aircraft's), its fix has ADSB_MLAT_VALID, latitude,
 *   longitude and height_m are finite with |latitude| <= 89 and height_m in [-1000, 100000], hdop is finite and in
 *   (0, max_hdop], and var_h below is finite.  Every other frame's operand is 64 zero bytes.  A usable frame's holds
 *     time      the store's frame time (sample_base + offset) x seconds_per_sample, the one rounded product
 *     latitude, longitude  the fix's;  height_m  the fix's, rounded to f32 once (as adsb_aircraft_mlat's)
 *     rn, re    metres per degree of latitude / of longitude at the fix: with s = sin(lat), w2 = 1 - e2 s^2, w = sqrt(w2),
 *               M = a (1 - e2) / (w2 w), N = a / w (WGS84 a, e2):  rn = (M + h) x pi/180,  re = (N + h) x cos(lat) x pi/180
 *     sr        = residual_rms_m if that is greater than range_sigma_m, else range_sigma_m (a NaN residual gives the latter)
 *     var_h     = (hdop x sr)^2
 *     var_v     = altitude_sigma_m^2 if the fix has ADSB_MLAT_ALTITUDE, else (vdop x sr)^2
 *     HEIGHT    the vertical axis is measured: var_v is finite and, without ADSB_MLAT_ALTITUDE, vdop is in (0, max_vdop].
 *               Without HEIGHT the var_v field holds (max_vdop x sr)^2 instead, what a start gives the up axis.
 *   All trigonometry and every root of the feature is here; the walk has only + - x / and compares.
 * PER AIRCRAFT, THE WALK over its usable frames in list order.  Three independent 2-state filters (position, velocity;
 *   symmetric covariance Ppp, Ppv, Pvv) on north, east and up metres, white-acceleration model with q = accel_h^2 for
 *   north and east and accel_v^2 for up.  For a usable frame with operand o and the aircraft's record r:
 *     START  latitude, longitude, height_m = o's; velocities 0; P = (var, 0, init_speed_sigma^2) per axis (var_h and
 *       init_speed_sigma_h for north and east, o.var_v and init_speed_sigma_v for up); time = o.time; run = 1,
 *       outliers_run = 0; RUNNING set, HEIGHT as o's.  The frame is INIT and its nis is 0.  A record that is not
 *       RUNNING starts at its first usable frame.
 *     dt = o.time - r.time.  !(dt >= 0) (out of order, or NaN): the frame is SKIPPED, n_skipped + 1, nothing else
 *       changes.  dt > reset_gap_s: n_reset + 1 and START (RESET | INIT).
 *     PREDICT per axis:  p = v dt;  P'pp = Ppp + 2 dt Ppv + dt^2 Pvv + q dt^4 / 4;  P'pv = Ppv + dt Pvv + q dt^3 / 2;
 *       P'vv = Pvv + q dt^2.
 *     MEASURED displacement from the estimate:  zn = (o.latitude - r.latitude) rn;  ze = wrap(o.longitude - r.longitude)
 *       re;  zu = o.height_m - r.height_m.  wrap adds or subtracts 360 once, to land in [-180, 180].
 *     INNOVATION  y = z - p,  S = P'pp + var;  nis = yn^2 / Sn + ye^2 / Se (horizontal only, two degrees of freedom).
 *     nis > gate^2: the frame is an OUTLIER, n_outlier + 1, outliers_run + 1, last_nis = nis; state and time are
 *       untouched, so the next fix predicts from the last applied state.  If outliers_run has now reached max_outliers
 *       the aircraft really is elsewhere: n_reset + 1 and START (OUTLIER | RESET | INIT; the frame keeps its nis).
 *     Otherwise the frame is APPLIED, per measured axis:  Kp = P'pp / S, Kv = P'pv / S;  d = p + Kp y;  v += Kv y;
 *       P = ((1 - Kp) P'pp, (1 - Kp) P'pv, P'vv - Kv P'pv).  An up axis without HEIGHT takes d = p, P = P'; with it
 *       the record's HEIGHT is set.  Then latitude += dn / rn, longitude = wrap(longitude + de / re), height_m += du,
 *       time = o.time, n_applied + 1, run + 1, outliers_run = 0, last_nis = nis.
 *     VELOCITY is set in the record exactly while run >= min_run.
 *   f64 throughout with contraction off; the four counts and run saturate at 2^32 - 1.
 * The state is in the record and each frame's operand is its own, so one list (frames and fixes alike) cut into any
 * sequence of updates gives the same 192 bytes per aircraft and the same per-frame outputs, and two runs give the same
 * bytes.  An EMPTY record is all zeros with time NaN.  A place is emptied at admission, at re-admission after an expire,
 * and at a reset; expire moves a survivor's filter record with its record.
 * On the device, behind the mlat merge: one thread per sorted frame writes the operand at its sorted position (and 32
 * zero bytes of output for a frame that is not usable), then one thread per segment HEAD loads the record once, steps
 * through its segment's operands, which lie consecutively, writes one adsb_frame_filter per usable frame at the frame's
 * list index and the record once at the end.  No atomics, no LDS, nothing read back.  The critical path of that walk is
 * the LONGEST aircraft's part of the list, not the list: nothing here is linear however long one aircraft's part is.  It
 * is cheap because a step is some sixty f64 operations on registers and one 64-byte load.  Device memory, all of it
 * allocated by the reserve and none before: 192 bytes per place of max_aircraft and 64 + 32 bytes per frame of
 * max_frames.  A table that never reserves allocates nothing, launches exactly the kernels it launched before and
 * returns the same bytes; with the reserve every other array of the table is byte for byte what it is without.
 * fetch_changed, the per-frame summaries and a bank's fused view carry no filter records.
 */
#define ADSB_TRACK_FILTER_RUNNING  0x1u   /* adsb_aircraft_filter.flags: the record holds a state           */
#define ADSB_TRACK_FILTER_VELOCITY 0x2u   /* run >= min_run: the velocities are worth showing               */
#define ADSB_TRACK_FILTER_HEIGHT   0x4u   /* record: the up axis has been measured since the start; operand: it is */
#define ADSB_TRACK_FILTER_USABLE   0x100u /* adsb_frame_filter.flags and adsb_filter_operand.flags          */
#define ADSB_TRACK_FILTER_APPLIED  0x200u /* adsb_frame_filter.flags only, as are the next four             */
#define ADSB_TRACK_FILTER_INIT     0x400u
#define ADSB_TRACK_FILTER_RESET    0x800u
#define ADSB_TRACK_FILTER_OUTLIER  0x1000u
#define ADSB_TRACK_FILTER_SKIPPED  0x2000u
typedef struct adsb_track_filter_cfg { /* 96 bytes; every field is policy, not a measurement; 0 takes the default */
    double   accel_h, accel_v;          /* m/s^2, 1-sigma of the white acceleration; 3, 1.5              */
    double   range_sigma_m;             /* floor of the range error a dilution multiplies; 30            */
    double   altitude_sigma_m;          /* of a message's own altitude; 15                               */
    double   gate;                      /* sigmas; 4                                                     */
    double   reset_gap_s;               /* 30                                                            */
    double   init_speed_sigma_h, init_speed_sigma_v; /* m/s; 300, 30                                     */
    double   max_hdop, max_vdop;        /* 20, 50                                                        */
    uint32_t max_outliers, min_run;     /* 3, 4                                                          */
    uint64_t reserved;                  /* 0 */
} adsb_track_filter_cfg;
typedef struct adsb_aircraft_filter {  /* 192 bytes, one per record place, beside the 128-byte record */
    double   time;                      /* frame time of the last START or APPLIED frame; NaN if none    */
    double   latitude, longitude;       /* degrees, filtered                                             */
    double   height_m;
    double   v_north, v_east, v_up;     /* m/s                                                           */
    double   p_north[3], p_east[3], p_up[3]; /* Ppp (m^2), Ppv (m^2/s), Pvv (m^2/s^2) of each axis       */
    uint32_t n_applied, n_outlier, n_reset, n_skipped; /* saturating                                     */
    uint32_t run;                       /* START and APPLIED frames since the last START; saturating     */
    uint32_t outliers_run;              /* OUTLIER frames since the last START or APPLIED one            */
    float    last_nis;                  /* of the newest APPLIED or OUTLIER frame (rounded to f32 once)  */
    uint32_t flags;                     /* ADSB_TRACK_FILTER_RUNNING / VELOCITY / HEIGHT                 */
    uint32_t reserved[8];               /* 0 */
} adsb_aircraft_filter;
typedef struct adsb_frame_filter {     /* 32 bytes, one per frame of the last update given fixes, in its list order */
    double   latitude, longitude;       /* the aircraft's filtered position right after this frame       */
    float    height_m, nis;             /* each rounded to f32 once                                      */
    uint32_t flags;                     /* USABLE, and APPLIED / INIT / RESET / OUTLIER / SKIPPED; 0: not usable, all else 0 */
    uint32_t reserved;                  /* 0 */
} adsb_frame_filter;
typedef struct adsb_filter_operand {   /* 64 bytes per frame, in SORTED order: what the walk reads (see above) */
    double   time, latitude, longitude;
    double   rn, re, var_h, var_v;
    float    height_m;
    uint32_t flags;                     /* USABLE, HEIGHT; 0: not usable, all else 0 */
} adsb_filter_operand;
/* Allocates the above, keeps the cfg (NULL: every default) and empties every filter record.  May wait for the device.
 * A second reserve changes nothing (the first cfg stays).  ADSB_E_ARG for a NULL table, or a cfg field that is neither
 * 0 nor finite and > 0, or a reserved that is not 0 (checked before the table is touched); ADSB_E_STATE without an mlat
 * reserve; ADSB_E_NOMEM if the memory is not to be had. */
int adsb_track_table_filter_reserve(adsb_track_table *table, const adsb_track_filter_cfg *cfg);
/* Waits; one filter record per aircraft, in exactly the order adsb_track_table_fetch returns the records (ascending
 * ICAO); *n = records held even if more than max.  ADSB_E_ARG for a NULL table, or NULL out with max > 0;
 * ADSB_E_STATE without a reserve. */
int adsb_track_table_fetch_filter(adsb_track_table *table, adsb_aircraft_filter *out, size_t max, size_t *n);
/* Does not synchronise: the device address of the filter records, one per record PLACE in slot order (as
 * adsb_track_table_mlat_device); dev may be NULL.  ADSB_E_ARG for a NULL table, ADSB_E_STATE without a reserve. */
int adsb_track_table_filter_device(adsb_track_table *table, const adsb_aircraft_filter **dev);
/* Waits; one adsb_frame_filter per frame of the last update given fixes, in its list order: copies min(frames, max),
 * *n = copied.  ADSB_E_ARG for a NULL table, or NULL out with max > 0; ADSB_E_STATE without a reserve or before the
 * first such update since the reserve (and since a reset). */
int adsb_track_table_fetch_frame_filter(adsb_track_table *table, adsb_frame_filter *out, size_t max, size_t *n);
/* For tests.  Waits; the operands of the last update given fixes, in SORTED order (ascending address, list order within
 * one): copies min(frames, max), *n = copied.  Errors as fetch_frame_filter. */
int adsb_debug_track_filter_operands(adsb_track_table *table, adsb_filter_operand *out, size_t max, size_t *n);

/*
 * Mode S replies per aircraft.  adsb_modes_of gives every frame of a list its address and kind; with a modes reserve a
 * TABLE takes the whole list, keyed by that address instead of bytes[1..3], so an aircraft that only answers
 * interrogations (DF0/4/5/11/16/20/21) gets a record, a place for its multilaterated fix, and one 64-byte
 * adsb_aircraft_modes beside its record with what its replies say.  Correlate's frames, adsb_modes_of's records and the
 * solver's fixes line up index for index in device memory; update_modes takes the three.  Tables only: a bank has no
 * such entry point and behaves as before (its 32-bit sort key, receiver << 24 | icao, has no spare bit for "no address"
 * at 256 receivers).
 *
 * ACCEPTED  Frame j is accepted iff recs[j].kind is ADSB_MODES_SELF or ADSB_MODES_KNOWN; its aircraft is
 *   recs[j].address & 0xFFFFFF.  The decision is by kind, never by the address value: address 0 from known_in is an
 *   aircraft, a PARITY record (whose address is 0 too) is none.
 * NOT ACCEPTED (UNKNOWN, PARITY, UNSUPPORTED)  The frame touches no record, no side record, no count, no last_heard and
 *   no changed-list entry, never admits an aircraft and never sets ADSB_TRACK_TABLE_FULL.  Its point has icao =
 *   recs[j].address and flags exactly ADSB_TRACK_UNADDRESSED; its per-frame summary, frame fix and frame mlat are what
 *   an UNTRACKED frame's are, with that icao.  Garbage cannot create aircraft.
 * MAIN RECORD  An accepted frame with DF 17 or 18 is exactly what adsb_track_table_update makes of it (for a SELF frame
 *   the address is bytes[1..3]).  An accepted frame of any other DF is keyed by its address and is a frame of kind
 *   "other": n_frames + 1 and last_heard, nothing else, whatever bytes[4..] look like: no identification, position or
 *   velocity message to the pair walk, the summaries, the single-message fix (its adsb_frame_fix carries the address as
 *   icao and nothing else) or the mlat check.  With fixes, its valid fix becomes the aircraft's kept mlat fix, as for
 *   any counted frame.
 * ADMISSION  An accepted frame of an address the table does not hold is admitted by the ascending-address rule together
 *   with the list's other new addresses; turned away by a full table it is ADSB_TRACK_UNTRACKED (not UNADDRESSED).
 * COUNTED  A frame is counted for the side record iff it is accepted and its point is not UNTRACKED.  Per counted
 *   frame: DF17/18 sets SQUITTER; any other DF adds 1 to n_replies and also to n_allcall (DF11), n_surveillance
 *   (DF4/5/20/21) or n_airair (DF0/16), all saturating at 2^32 - 1.  last_df is the newest counted frame's df.
 *   altitude_ft, altitude_time and ALT come from the newest counted frame with ADSB_MODES_ALT; squawk, squawk_time and
 *   SQUAWK likewise with ADSB_MODES_SQUAWK; callsign, callsign_time and CALLSIGN likewise with ADSB_MODES_CALLSIGN; fs,
 *   ALERT, SPI and STATUS from the newest counted DF4/5/20/21 frame; GROUND from the newest counted frame among
 *   DF0/4/5/16/20/21.  Newest = the last in list order (equal offsets apply in list order, as everywhere in the store).
 *   Times are the store's frame time, the single rounded product (sample_base + offset) x seconds_per_sample.
 * Every field combines associatively (saturating add, "later position wins", OR), so one list with its recs, fixes and
 * levels cut into any sequence of update_modes calls gives the same 64 bytes per aircraft and the same main, mlat and
 * level records, and two runs give the same bytes.  An EMPTY record is all zeros with the three times NaN: at
 * admission, at re-admission after an expire, after a reset, and for aircraft held from before the reserve until a
 * counted frame changes it.  Expire moves a survivor's record with it.
 * On the device: a key kernel after the field decode (one thread per frame) makes every frame that is not an accepted
 * DF17/18 one of kind "other" in the table's own fields and writes the sort key, the address or 1 << 24 for a frame
 * that is not accepted, so the sort covers 25 bits and the rejected frames form one last segment that the lookup gives
 * no slot.  After the pairs step one thread per frame writes a 48-byte scan operand at its sorted position (and the
 * UNADDRESSED point), one segmented inclusive scan (rocPRIM; head mark, six "newest position" words, four saturating
 * counts, the squitter bit) runs over the sorted list, and one thread per segment tail reads the winning frames'
 * records and times and merges into the side record: no atomics, linear in the list.  Device memory, all of it
 * allocated by the reserve and none before: 64 bytes per place of max_aircraft, and per frame of max_frames 48 + 48
 * bytes plus 32 bytes of device staging for a host recs array, the 25-bit sort's and the scan's scratch; 32 bytes per
 * frame of pinned host memory.  A table that never reserves allocates nothing, launches exactly the kernels it launched
 * before and returns the same bytes; update, update_levels and update_mlat of a table that did reserve behave as before
 * and leave the modes records alone (apart from admission emptying a place).
 */
#define ADSB_TRACK_UNADDRESSED 0x4u /* point flag: the frame's address is not an aircraft's; nothing was touched */
#define ADSB_TRACK_MODES_ALT      0x1u   /* altitude_ft, altitude_time hold a value (ADSB_MODES_ALT's bit)   */
#define ADSB_TRACK_MODES_SQUAWK   0x4u   /* squawk, squawk_time hold a value                                 */
#define ADSB_TRACK_MODES_GROUND   0x8u   /* the newest DF0/4/5/16/20/21 frame said: on the ground            */
#define ADSB_TRACK_MODES_ALERT    0x10u  /* with STATUS: the newest DF4/5/20/21 frame's alert                */
#define ADSB_TRACK_MODES_SPI      0x20u  /* with STATUS: ... its special position identification             */
#define ADSB_TRACK_MODES_CALLSIGN 0x40u  /* callsign, callsign_time hold a value (BDS 2,0)                   */
#define ADSB_TRACK_MODES_STATUS   0x100u /* fs, ALERT and SPI hold a value                                   */
#define ADSB_TRACK_MODES_SQUITTER 0x200u /* the aircraft has sent an accepted DF17/18 frame: it has ADS-B    */
typedef struct adsb_aircraft_modes {   /* 64 bytes, one per record place, beside the 128-byte record */
    double   altitude_time, squawk_time, callsign_time; /* store frame time of the frame each came from; NaN if none */
    int32_t  altitude_ft;
    uint16_t squawk;
    uint16_t flags;                 /* ADSB_TRACK_MODES_* */
    char     callsign[8];
    uint32_t n_replies, n_allcall, n_surveillance, n_airair; /* saturating at 2^32 - 1 */
    uint8_t  fs;                    /* of the newest DF4/5/20/21 frame */
    uint8_t  last_df;               /* of the newest counted frame */
    uint8_t  reserved[6];           /* 0 */
} adsb_aircraft_modes;
#ifdef __cplusplus
static_assert(sizeof(adsb_aircraft_modes) == 64, "adsb_aircraft_modes layout");
#endif
/* Allocates the above and empties every modes record.  May wait for the device.  A second reserve changes nothing.
 * ADSB_E_ARG for a NULL table; ADSB_E_NOMEM if the memory is not to be had. */
int adsb_track_table_modes_reserve(adsb_track_table *table);
/* The update described above.  recs[n] and, if given, fixes[n] and levels[n] are the frames' in list order.  frames,
 * recs, fixes and levels may each be host memory or memory of the ctx's device, independently; host arrays have been
 * copied when this returns.  recs may be adsb_modes_device's pointer (the ctx's scratch, ordered on the same stream).
 * ADSB_E_ARG for a NULL table, or NULL frames or recs with n > 0; ADSB_E_STATE without a modes reserve, for fixes
 * without an mlat reserve, or for levels without a levels reserve; ADSB_E_CAPACITY for n > max_frames; n = 0 is
 * ADSB_OK. */
int adsb_track_table_update_modes(adsb_track_table *table, const adsb_frame *frames, const adsb_modes_rec *recs,
                                  const adsb_mlat_fix *fixes /* may be NULL */,
                                  const adsb_frame_level *levels /* may be NULL */, size_t n, uint64_t sample_base);
/* Waits; one modes record per aircraft, in exactly the order adsb_track_table_fetch returns the records (ascending
 * ICAO); *n = records held even if more than max.  ADSB_E_ARG for a NULL table, or NULL out with max > 0;
 * ADSB_E_STATE without a reserve. */
int adsb_track_table_fetch_modes(adsb_track_table *table, adsb_aircraft_modes *out, size_t max, size_t *n);
/* Does not synchronise: the device address of the modes records, one per record PLACE in slot order; dev may be NULL.
 * ADSB_E_ARG for a NULL table, ADSB_E_STATE without a reserve. */
int adsb_track_table_modes_device(adsb_track_table *table, const adsb_aircraft_modes **dev);

/*
 * Comm-B registers per aircraft.  adsb_commb_of decodes BDS 1,0 to 6,0 of every DF20/21 reply and is stateless; with a
 * commb reserve (beside the modes reserve) a TABLE keeps, per aircraft, the newest 4,0, 5,0 and 6,0 values, the newest
 * 1,7 capability word and 3,0 word, and four counts, in one 128-byte adsb_aircraft_commb beside its record.  It also
 * settles what the stateless stage cannot: a payload that passes as 5,0 and as 6,0 is read against the aircraft's own
 * ADS-B airborne velocity, which the table holds.  update_commb is update_modes plus the frames' adsb_commb_rec[]:
 * everything update_modes does it does, with the same results; what follows is what it adds.  Tables only.
 *
 * COUNTED  A frame is counted iff update_modes counts it (accepted by kind, its point not UNTRACKED) and its commb
 *   state is not NOT_COMMB.  Per counted frame, by its PER-FRAME OUTPUT (below):
 *     n_commb + 1.
 *     NONE: n_none + 1.
 *     ONE or SETTLED with bds 0x40 / 0x50 / 0x60: that block becomes { frame time, value[5], status, settled = 1 for
 *       SETTLED and 0 for ONE }.  SETTLED also adds 1 to n_settled.
 *     ONE with bds 0x17: capability = word (a 1,7 word is never 0, bit 7 is set; a record with word 0 writes nothing).
 *     ONE with bds 0x30: ra_word = word, ra_time = frame time.
 *     AMBIGUOUS (it stayed ambiguous): n_ambiguous + 1.
 *     EMPTY, ONE with bds 0x10 or 0x20, and any other state or bds: only n_commb.
 *   Counts saturate at 2^32 - 1.  Every combine is a saturating add or "the later list position wins", so it is
 *   associative.  The EMPTY record has every time NaN and everything else 0 and is the identity of the merge: at
 *   admission, at re-admission after an expire, after a reset, and for aircraft held from before the reserve.  Times
 *   are the store's frame time, the single rounded product (sample_base + offset) x seconds_per_sample.
 * PER-FRAME OUTPUT  frame_commb[j] is commb[j] byte for byte, except for a settled frame: state ADSB_COMMB_SETTLED and
 *   the bds, status, value and word that the decode of the frame's MB as the settled register gives (what
 *   adsb_host_commb_as gives); candidates, n_candidates and reserved stay.  A frame that is not counted is never settled.
 * WHICH FRAMES  Only a counted frame whose record is AMBIGUOUS with candidates == ADSB_COMMB_C50 | ADSB_COMMB_C60.
 *   Every other candidate set stays ambiguous.
 * REFERENCE R  The aircraft's newest airborne-velocity message that precedes the frame in list order, over the table's
 *   whole history since the aircraft's admission: an accepted DF17/18 frame with TC 19 and ST 1-4 (exactly what the
 *   record's adsb_velocity takes).  In the current list it is the newest such frame of the aircraft before the frame
 *   being settled; if the list has none before it, R is the record's adsb_velocity as it stood before this update.  R
 *   is usable iff 0 <= t_frame - R.time <= max_age_s, computed in f64 with one subtraction (NaN: not usable).  Without
 *   a usable R nothing is settled.
 * EXACT FIELDS  The rule reads v_ew_kt, v_ns_kt, vertical_rate_fpm, subtype, flags and airspeed_tas; for ST 3-4 also
 *   speed_kt (an integer value, "airspeed" below) and h10 = direction_deg x 128 / 45 (an exact integer, the 10-bit
 *   heading).  It never reads direction_deg or speed_kt of ST 1-2.  SPEED, DIRECTION, VRATE: R's flags.
 * DEFINITIONS  S = max_speed_diff_kt, V = max_vrate_diff_fpm, s2 = v_ew^2 + v_ns^2, vr = vertical_rate_fpm.
 *   sector16(ew, ns), with a = |ew| and b = |ns|: k = 0 if 985 a < 408 b, else k = 1 if a < b, else k = 2 if
 *   408 a < 985 b, else k = 3; the sector is k for ew >= 0 and ns > 0, 7 - k for ew > 0 and ns <= 0, 8 + k for ew <= 0
 *   and ns < 0, and 15 - k otherwise.  Sector distance is circular over 16.  value[] and status are those of the
 *   reading in question (VALUES above).
 * CHECKS ON THE READING AS 5,0
 *   status bit 2, R ST 1-2 with SPEED: passes iff max(g - S, 0)^2 <= s2 <= (g + S)^2 with g = value[2].
 *   status bit 1, R ST 1-2 with SPEED and s2 > 0: passes iff the distance of value[1] >> 7 and sector16 is <= 1.
 *   status bit 4, R ST 3-4 with SPEED and airspeed_tas = 1: passes iff |value[4] - airspeed| <= S.
 * CHECKS ON THE READING AS 6,0
 *   status bit 0, R ST 1-2 with SPEED and s2 > 0: passes iff the distance of value[0] >> 7 and sector16 is <= 2
 *     (heading differs from track by drift and magnetic variation).
 *   status bit 0, R ST 3-4 with DIRECTION: passes iff the circular |value[0] - 2 h10| over 2048 is <= 128.
 *   status bit 1, R ST 3-4 with SPEED and airspeed_tas = 0: passes iff |value[1] - airspeed| <= S.
 *   status bit 3, R with VRATE: passes iff |value[3] - vr| <= V.
 *   status bit 4, R with VRATE: passes iff |value[4] - vr| <= V.
 * DECISION  A reading is supported iff at least one check applies and none fails, contradicted iff at least one fails.
 *   The frame is settled to X iff X is supported and the other reading is contradicted.
 * CUT INVARIANCE  The rule depends only on the frame sequence: one list cut into any sequence of update_commb calls
 *   gives the same 128 bytes per aircraft, and the concatenated frame_commb is the uncut call's.
 * On the device, after everything update_modes launches and before the merge into the main records (so the held
 * velocity is still the one from before this update): one segmented scan over the sorted list gives every frame the
 * sorted position of its aircraft's newest earlier velocity frame; one thread per frame resolves R, settles, writes
 * frame_commb[j] and a 40-byte scan operand at its sorted position; one segmented inclusive scan (head mark, five
 * "newest position" words, four saturating counts); one thread per segment tail reads the winners' frame_commb and
 * times and merges into the side record.  No atomics, integers only, linear in the list.  Device memory, all of it
 * allocated by the reserve: 128 bytes per place of max_aircraft, and per frame of max_frames 8 + 32 + 40 + 40 bytes
 * plus 32 bytes of device staging for a host commb array and the scans' scratch; 32 bytes per frame of pinned host
 * memory.  A table that never reserves allocates nothing and launches exactly the kernels it launched before; update,
 * update_levels, update_mlat and update_modes of a table that did reserve behave as before and leave the commb
 * records alone (apart from admission emptying a place).
 */
#define ADSB_COMMB_SETTLED 5u     /* only in a table's per-frame output, never from adsb_commb_of */
typedef struct adsb_commb_settle_cfg { /* 16 bytes */
    double   max_age_s;           /* R is usable up to this age; 10.0 is the store's own CPR pairing window */
    uint32_t max_speed_diff_kt;   /* S */
    uint32_t max_vrate_diff_fpm;  /* V */
} adsb_commb_settle_cfg;
typedef struct adsb_commb_block { /* 32 bytes */
    double   time;                /* store frame time of the frame it came from; NaN = none */
    int32_t  value[5];            /* as in adsb_commb_rec */
    uint16_t status;
    uint16_t settled;             /* 1: the frame was settled by the table, 0: adsb_commb_of found it unambiguous */
} adsb_commb_block;
/* (tag first, typedef after: the one record of this header with members of a struct type) */
struct adsb_aircraft_commb {          /* 128 bytes, one per record place */
    adsb_commb_block bds40, bds50, bds60;               /* newest of each; time NaN = none */
    uint32_t n_commb, n_settled, n_ambiguous, n_none;   /* saturating at 2^32 - 1 */
    uint32_t capability;          /* newest 1,7 word; 0 = none */
    uint32_t ra_word;             /* newest 3,0 word */
    double   ra_time;             /* its frame time; NaN = none */
};
typedef struct adsb_aircraft_commb adsb_aircraft_commb;
#ifdef __cplusplus
static_assert(sizeof(adsb_commb_settle_cfg) == 16 && sizeof(adsb_commb_block) == 32 && sizeof(adsb_aircraft_commb) == 128,
              "adsb_aircraft_commb layout");
#endif
/* Allocates the above and empties every commb record.  cfg NULL: 10.0 s, 40 kt, 1000 ft/min (policy, not
 * measurements).  May wait for the device.  A second reserve changes nothing, its cfg neither.  ADSB_E_ARG for a NULL
 * table or a max_age_s that is NaN or negative; ADSB_E_NOMEM if the memory is not to be had. */
int adsb_track_table_commb_reserve(adsb_track_table *table, const adsb_commb_settle_cfg *cfg);
/* The update described above.  recs[n], commb[n] and, if given, fixes[n] and levels[n] are the frames' in list order.
 * Each may be host memory or memory of the ctx's device, independently; host arrays have been copied when this returns.
 * recs may be adsb_modes_device's pointer and commb adsb_commb_device's (the ctx's scratch, ordered on the same
 * stream).  ADSB_E_ARG for a NULL table, or NULL frames, recs or commb with n > 0; ADSB_E_STATE without a modes reserve
 * or without a commb reserve, for fixes without an mlat reserve, or for levels without a levels reserve;
 * ADSB_E_CAPACITY for n > max_frames; n = 0 is ADSB_OK. */
int adsb_track_table_update_commb(adsb_track_table *table, const adsb_frame *frames, const adsb_modes_rec *recs,
                                  const adsb_commb_rec *commb, const adsb_mlat_fix *fixes /* may be NULL */,
                                  const adsb_frame_level *levels /* may be NULL */, size_t n, uint64_t sample_base);
/* Waits; one commb record per aircraft, in exactly the order adsb_track_table_fetch returns the records (ascending
 * ICAO); *n = records held even if more than max.  ADSB_E_ARG for a NULL table, or NULL out with max > 0;
 * ADSB_E_STATE without a reserve. */
int adsb_track_table_fetch_commb(adsb_track_table *table, adsb_aircraft_commb *out, size_t max, size_t *n);
/* Waits; the per-frame output of the last update_commb, in list order (another update in between leaves it alone);
 * *n = min(frames of that update, max).  ADSB_E_ARG for a NULL table, or NULL out with max > 0; ADSB_E_STATE without a
 * reserve or before any update_commb since the reserve or the last reset. */
int adsb_track_table_fetch_frame_commb(adsb_track_table *table, adsb_commb_rec *out, size_t max, size_t *n);
/* Does not synchronise: the device address of the commb records, one per record PLACE in slot order; dev may be NULL.
 * ADSB_E_ARG for a NULL table, ADSB_E_STATE without a reserve. */
int adsb_track_table_commb_device(adsb_track_table *table, const adsb_aircraft_commb **dev);

/*
 * Extended squitter status per aircraft.  adsb_es_of reads what every DF17/18 frame says beside identity, position and
 * velocity and is stateless; with an es reserve a TABLE keeps, per aircraft, the newest operational status (airborne
 * and surface), target state, emergency / squawk and ACAS RA records, the ADS-B version, NIC supplements A and C, the
 * category, NACv, and two counts, in one 256-byte adsb_aircraft_es beside its record.  It also resolves what the
 * stateless stage cannot: NIC and the containment radius Rc of a position message depend on the aircraft's version and
 * on supplements that arrive in OTHER messages of the same aircraft, which the table holds.  update_es is one of the
 * existing updates plus the frames' adsb_es_rec[]: with recs NULL it is update (update_levels / update_mlat with those
 * arrays), keyed by bytes[1..3]; with recs it is update_modes, keyed by the resolved address; with recs and commb it is
 * update_commb.  Everything the chosen update does it does, with the same results; what follows is what it adds.
 * Tables only.
 *
 * COUNTED  A frame is counted iff its sort key is an aircraft's (any key without recs; with recs, a frame update_modes
 *   accepts by kind), its point is not UNTRACKED, and es[j].state is neither NOT_ES nor FOREIGN.  A frame that is not
 *   counted gets an all-zero adsb_frame_integrity and touches nothing.  Per counted frame, by es[j] and its PER-FRAME
 *   OUTPUT (below), each line on its own:
 *     n_es + 1.
 *     OPERATIONAL with subtype 0 / subtype 1, TARGET_STATE, EMERGENCY, ACAS_RA: operational_airborne /
 *       operational_surface / target_state / emergency / acas_ra = es[j], all 32 bytes, and its time[] = frame time.
 *     present has HAS_VERSION: version = es[j].version, version_time = frame time.
 *     present has HAS_NIC_A: nic_a and nic_a_time.  present has HAS_NIC_C: nic_c and nic_c_time.
 *     CATEGORY: category = es[j].category (never 0: a real one is >= 0xA0).
 *     present has HAS_NAC_V (a VELOCITY, or a version-2 surface OPERATIONAL): nac_v = es[j].nac_v, and as ONE group
 *       with it velocity_flags = the low byte of es[j].flags for a VELOCITY and 0 otherwise, has = 3 for a VELOCITY and
 *       1 otherwise (bit 0: nac_v holds a value; bit 1: velocity_flags came from a velocity message).
 *     POSITION: n_position + 1; rc_dm and nic = the per-frame output's; position_supp = its supp in bits 0-2 and its
 *       VERSIONED, STALE_A and STALE_C flags in bits 3, 4 and 5 (the flag's value << 1), so the record says how its
 *       newest position was resolved; position_tc = the type code; nic_b = es[j].nic_b with HAS_NIC_B and 0 without;
 *       position_time = frame time.
 *   Counts saturate at 2^32 - 1.  Every combine is a saturating add or "the later list position wins" per block and per
 *   version / A / C / position / category / NACv group, so it is associative.  The EMPTY record has every time NaN and
 *   everything else 0 and is the identity of the merge: at admission, at re-admission after an expire, after a reset,
 *   and for aircraft held from before the reserve.  Times are the store's frame time, the single rounded product
 *   (sample_base + offset) x seconds_per_sample.
 * RESOLUTION of a counted frame heard at t.  V, A and C are the aircraft's newest counted frames BEFORE it in list
 *   order with HAS_VERSION, HAS_NIC_A and HAS_NIC_C respectively, over the table's history since the aircraft's
 *   admission: the newest such frame earlier in the current list, else what the record held before this update.  A
 *   frame never uses itself or a later frame: an operational status that follows a position in the same list does not
 *   reach it.  The version never expires.  A and C are usable iff 0 <= t - time <= max_age_s, computed in f64 with one
 *   subtraction (NaN: not usable; a negative age, from a smaller sample_base in a later update, is not usable).  A
 *   supplement the aircraft has but that is not usable sets STALE_A / STALE_C and enters as 0.  B is the frame's own
 *   nic_b if it has HAS_NIC_B, else 0.
 * PER-FRAME OUTPUT  For a counted POSITION frame: (nic, rc_dm) = what adsb_host_es_integrity gives for (type code, V's
 *   version or ADSB_ES_VERSION_UNKNOWN, supp) with supp = A | B << 1 | C << 2; version = V's or UNKNOWN; flags =
 *   COUNTED | POSITION, VERSIONED iff V exists, STALE_A, STALE_C.  That table decides which supplements a version and a
 *   type code read; a version-2 supplement A held when a version-0 status arrives is handed over and ignored there.
 *   For a counted frame that is no position: flags = COUNTED, version = V's or UNKNOWN, all else 0.
 * CUT INVARIANCE  The rule depends only on the frame sequence: one list cut into any sequence of update_es calls gives
 *   the same 256 bytes per aircraft, and the concatenated frame_es is the uncut call's.
 * max_age_s is policy, not a measurement: 60.0 by default; +inf keeps a supplement for ever.
 * On the device, beside the levels / fix / mlat merges (the step needs the sort, the record slots and its own side array
 * only): one segmented inclusive scan whose operand is computed where it is loaded, from es[]: a head mark and the
 * sorted position + 1 of the newest frame with HAS_VERSION, HAS_NIC_A and HAS_NIC_C; one thread per sorted frame reads
 * its predecessor's scan words, resolves V / A / C from those frames or from the held record, writes frame_es[j] and a
 * 56-byte scan operand at its sorted position; one segmented inclusive scan (head mark, eleven "newest position" words,
 * two saturating counts); one thread per segment tail reads the winners' es[], frame_es and times and merges into the
 * side record.  No atomics, no workgroup waits for another, nothing is read back, linear in the list.  Device memory,
 * all of it allocated by the reserve: 256 bytes per place of max_aircraft, and per frame of max_frames 16 + 8 + 56 + 56
 * bytes plus 32 bytes of device staging for a host es array and the scans' scratch; 32 bytes per frame of pinned host
 * memory.  A table that never reserves allocates nothing and launches exactly the kernels it launched before; update,
 * update_levels, update_mlat, update_modes and update_commb of a table that did reserve behave as before and leave the
 * es records alone (apart from admission emptying a place).
 */
#define ADSB_TRACK_ES_COUNTED   0x1u  /* adsb_frame_integrity.flags: the frame was counted                          */
#define ADSB_TRACK_ES_POSITION  0x2u  /* it is a position message: rc_dm, nic and supp hold the resolved values     */
#define ADSB_TRACK_ES_VERSIONED 0x4u  /* with POSITION: the aircraft's version was known                            */
#define ADSB_TRACK_ES_STALE_A   0x8u  /* with POSITION: the aircraft has a supplement A, too old (or from later)    */
#define ADSB_TRACK_ES_STALE_C   0x10u /* likewise supplement C                                                      */
typedef struct adsb_es_track_cfg { /* 16 bytes */
    double   max_age_s;           /* supplements A and C are usable up to this age; policy, not a measurement */
    uint32_t reserved[2];         /* 0 */
} adsb_es_track_cfg;
typedef struct adsb_frame_integrity { /* 8 bytes, one per frame of the last update_es */
    uint32_t rc_dm;               /* resolved Rc in decimetres, 0 unknown */
    uint8_t  nic;
    uint8_t  version;             /* the aircraft's version as known BEFORE this frame; ADSB_ES_VERSION_UNKNOWN if none */
    uint8_t  supp;                /* what was handed to the integrity table: bit 0 A, bit 1 B, bit 2 C */
    uint8_t  flags;               /* ADSB_TRACK_ES_COUNTED ... */
} adsb_frame_integrity;
/* (tag first, typedef after, as adsb_aircraft_commb: members of a struct type) */
struct adsb_aircraft_es {             /* 256 bytes, one per record place */
    adsb_es_rec operational_airborne, operational_surface, target_state, emergency, acas_ra; /* newest frame's record of each */
    double   time[5];             /* their frame times, same order; NaN = none */
    double   version_time, nic_a_time, nic_c_time, position_time; /* NaN = none */
    uint32_t rc_dm;               /* of the newest position message, resolved; 0 unknown */
    uint8_t  nic, position_tc, nic_b, position_supp; /* position_supp: A, B, C as handed over, then VERSIONED, STALE_A, STALE_C */
    uint8_t  version, nic_a, nic_c, category;   /* category 0 = none (a real one is >= 0xA0) */
    uint32_t n_es, n_position;    /* saturating at 2^32 - 1 */
    uint8_t  nac_v, velocity_flags, has, reserved; /* has bit 0: nac_v holds a value, bit 1: velocity_flags does */
};
typedef struct adsb_aircraft_es adsb_aircraft_es;
#ifdef __cplusplus
static_assert(sizeof(adsb_es_track_cfg) == 16 && sizeof(adsb_frame_integrity) == 8 && sizeof(adsb_aircraft_es) == 256,
              "adsb_aircraft_es layout");
#endif
/* Allocates the above and empties every es record.  cfg NULL: max_age_s = 60.0 (policy, not a measurement); +inf is
 * allowed.  May wait for the device.  A second reserve changes nothing, its cfg neither.  ADSB_E_ARG for a NULL table or
 * a max_age_s that is NaN or negative; ADSB_E_NOMEM if the memory is not to be had. */
int adsb_track_table_es_reserve(adsb_track_table *table, const adsb_es_track_cfg *cfg);
/* The update described above.  es[n] and, if given, recs[n], commb[n], fixes[n] and levels[n] are the frames' in list
 * order.  Each may be host memory or memory of the ctx's device, independently; host arrays have been copied when this
 * returns.  es may be adsb_es_device's pointer, recs adsb_modes_device's and commb adsb_commb_device's (the ctx's
 * scratch, ordered on the same stream).  ADSB_E_ARG for a NULL table, NULL frames or es with n > 0, or commb without
 * recs; ADSB_E_STATE without an es reserve, for recs without a modes reserve, for commb without a commb reserve, for
 * fixes without an mlat reserve, or for levels without a levels reserve; ADSB_E_CAPACITY for n > max_frames; n = 0 is
 * ADSB_OK. */
int adsb_track_table_update_es(adsb_track_table *table, const adsb_frame *frames, const adsb_es_rec *es,
                               const adsb_modes_rec *recs /* may be NULL */, const adsb_commb_rec *commb /* may be NULL */,
                               const adsb_mlat_fix *fixes /* may be NULL */,
                               const adsb_frame_level *levels /* may be NULL */, size_t n, uint64_t sample_base);
/* Waits; one es record per aircraft, in exactly the order adsb_track_table_fetch returns the records (ascending
 * ICAO); *n = records held even if more than max.  ADSB_E_ARG for a NULL table, or NULL out with max > 0;
 * ADSB_E_STATE without a reserve. */
int adsb_track_table_fetch_es(adsb_track_table *table, adsb_aircraft_es *out, size_t max, size_t *n);
/* Waits; the per-frame output of the last update_es, in list order (another update in between leaves it alone);
 * *n = min(frames of that update, max).  ADSB_E_ARG for a NULL table, or NULL out with max > 0; ADSB_E_STATE without a
 * reserve or before any update_es since the reserve or the last reset. */
int adsb_track_table_fetch_frame_es(adsb_track_table *table, adsb_frame_integrity *out, size_t max, size_t *n);
/* Does not synchronise: the device address of the es records, one per record PLACE in slot order; dev may be NULL.
 * ADSB_E_ARG for a NULL table, ADSB_E_STATE without a reserve. */
int adsb_track_table_es_device(adsb_track_table *table, const adsb_aircraft_es **dev);

/*
 * ---- several GPUs behind one call ---------------------------------------------------------
 * The reference's thread 2 is one function on one thread (src/adsb.rs:92, spawned at adsb.rs:147); a group is the
 * drop-in for that function when the buffer should be spread over N devices: one context per member, the offsets
 * [0, n - 240) of the buffer split evenly in member order, every member reading its own offsets plus a 239-sample
 * halo (neighbouring slices overlap by 240 samples: the window is 16 + 224, adsb.rs:98,106).  Every offset is
 * independent (adsb.rs:113 skips nothing), so the members' lists, which carry absolute offsets, concatenated in
 * member order ARE the single-context list: same frames, same order.  The lists meet in the root member's device
 * memory (hipMemcpyPeerAsync) as [ uint64 n_out | uint64 total_found | uint64 flags | uint64 0 | adsb_frame[...] ].
 * Members may name the same device more than once (several contexts on one GPU).  Like a context, a group is
 * not thread-safe: one calling thread.
 */
typedef struct adsb_group adsb_group;
typedef struct adsb_group_cfg {
    uint32_t       abi_version;  /* ADSB_ABI_VERSION                                                       */
    int32_t        sample_type;  /* ADSB_SAMPLE_I8 / ADSB_SAMPLE_I16                                       */
    uint32_t       n_members;    /* 1..64 contexts                                                         */
    uint32_t       root;         /* index of the member whose device receives the merged list              */
    const int32_t *devices;      /* [n_members] HIP device ordinal of each member                          */
    uint64_t       max_samples;  /* of the WHOLE buffer                                                    */
    uint64_t       max_out;      /* frames kept per launch, whole buffer                                   */
    uint32_t       host_staging; /* 1: per-member device staging so the host-pointer entry points work     */
    uint32_t       reserved;
} adsb_group_cfg;
typedef struct adsb_group_shard { /* what one member works on */
    uint64_t first_sample;       /* its slice starts here (a multiple of 8 samples) ...                    */
    uint64_t n_samples;          /* ... and is this long: n_offsets + 240; 0 = the member has nothing      */
    uint64_t n_offsets;          /* it owns the offsets [first_sample, first_sample + n_offsets)           */
} adsb_group_shard;
int adsb_group_create(const adsb_group_cfg *cfg, adsb_group **out_group);
void adsb_group_destroy(adsb_group *group);
uint32_t adsb_group_size(const adsb_group *group);
adsb_ctx *adsb_group_member(adsb_group *group, uint32_t index); /* e.g. for adsb_synth_fill_device on its device */
/* The split a group of n_members makes of an n_samples buffer (ADSB_E_SHORT below 240 samples). */
int adsb_group_plan(uint64_t n_samples, uint32_t n_members, adsb_group_shard *shards);
/* One iteration of the reference loop (adsb.rs:95-116) for one received buffer in HOST memory, spread over the
 * members: like adsb_demod().  Blocking.  Requires cfg.host_staging. */
int adsb_group_demod(adsb_group *group, const void *iq_host, size_t n_samples, adsb_frame *out, size_t max_out,
                     size_t *n_out, uint32_t *flags);
/* The same without waiting (copies and kernels are enqueued on the members' streams). */
int adsb_group_demod_host_async(adsb_group *group, const void *iq_host, size_t n_samples);
/* Device-resident form: iq_dev[i] = member i's slice (adsb_group_plan: samples [first_sample, first_sample +
 * n_samples) of the buffer) in ITS device's memory, 16-byte aligned; NULL where n_samples is 0. */
int adsb_group_demod_device_async(adsb_group *group, const void *const *iq_dev, size_t n_samples);
/* Waits for the members, merges, copies the list to the host (ascending offset). */
int adsb_group_fetch(adsb_group *group, adsb_frame *out, size_t max_out, size_t *n_out, uint64_t *total_found,
                     uint32_t *flags);
/* Waits for the members' counts and enqueues the merge; *blob_dev = the merged [header | frames] blob on the root
 * member's device, complete once *stream (hipStream_t, on that device) has drained. */
int adsb_group_result_device(adsb_group *group, const void **blob_dev, void **stream);

/* The stream the ctx enqueues on (hipStream_t as void*). */
void *adsb_stream(adsb_ctx *ctx);
/* cfg.sample_type the ctx was created with (ADSB_SAMPLE_*); ADSB_E_ARG for NULL. */
int adsb_sample_type(const adsb_ctx *ctx);

/* ---- measurement / test helpers (bench.py, tests; not part of the reference's surface) ----- */
/*
 * With timing on (on = N > 0), every N-th adsb_demod_device_async() attaches HIP events to the
 * scan kernel's dispatch and to the finishing kernel's (on the stream they run on).  adsb_timing_read()
 * waits for the stream, returns the mean milliseconds per launch of each since the last read
 * (at most the 512 most recent launches) and clears the log.
 */
int adsb_timing_enable(adsb_ctx *ctx, int on);
/* The two kernels of a launch separately: the scan kernel (demod_tiles: magnitude + preamble/DF17 gate over every
 * sample + PPM slice of the gate's survivors -- the kernel that reads the IQ bytes) and the finishing kernel
 * (finish_order: CRC-24, single-bit repair and the ordered frame list in one pass over the survivors; reported as
 * decode_ms_mean).  order_ms_mean is 0 since round 3 (the separate ordering pass was fused into finish_order).
 * adsb_timing_read reports the scan and the finishing kernel. */
int adsb_timing_read3(adsb_ctx *ctx, double *scan_ms_mean, double *decode_ms_mean, double *order_ms_mean,
                      uint32_t *n_launches);
int adsb_timing_read(adsb_ctx *ctx, double *demod_ms_mean, double *order_ms_mean,
                     uint32_t *n_launches);
/* Pure-read HBM ceiling on this device: streams `bytes` from `buf_dev` `iters` times with 16-byte loads in each of three
 * access shapes (4 / 8 / 16 loads in flight per lane; no shape is the fastest on every box and size) and returns the mean
 * milliseconds per pass of the fastest. */
int adsb_time_read_ceiling(adsb_ctx *ctx, const void *buf_dev, size_t bytes, int iters,
                           double *ms_per_pass);
/* Measurement: what one buffer costs when it comes from HOST memory through the streaming front end (adsb_feed_*, defined
 * further down; reference: src/adsb.rs:75-89 sends 20 000-sample buffers, adsb.rs:59-64 MTU-sized ones), timed from C with a
 * context and a feed of its own on `device`: in-place producer, two buffers in flight, every list popped, for about
 * `seconds`.  PCIe-inclusive by construction; bench.py prints it next to (never as) the HBM-resident `value`. */
int adsb_measure_feed(int device, int sample_type, size_t chunk_samples, double seconds, double *us_per_buffer,
                      double *frames_per_buffer, uint64_t *buffers);
/* Measurement: pinned host -> device copy rate of this box (GB/s), the ceiling of any host-fed path. */
int adsb_measure_pinned_copy(int device, size_t bytes, int iters, double *gbytes_per_s);
/* floor(sqrt(I^2+Q^2)) of n host samples through the device magnitude code (utils.rs:46-52). */
int adsb_debug_magnitudes(adsb_ctx *ctx, const void *iq_host, size_t n_samples,
                          uint16_t *mags_host);
/* How v_cvt_pk_u8_f32 was found to round on this device: 0 truncates, 1 truncates under
 * MODE.fp_round = toward-zero, 2 rounds to nearest (kernel subtracts 0.5 first). */
int adsb_debug_mag_mode(adsb_ctx *ctx);
/* v = I^2 + Q^2 + 72 of n host i8 samples through the packing code of the scan kernel's phase 1 (the gate and the
 * slicer of the i8 path work on these; utils.rs:46-52's root is only taken where a comparison needs it).  0xFFFF marks
 * a sample whose two packing paths disagree.  ADSB_E_STATE for a CS16 context. */
int adsb_debug_nsq_values(adsb_ctx *ctx, const void *iq_host, size_t n_samples, uint16_t *vals_host);
/* Measurement only: with on != 0 the following launches run the scan kernel (magnitude + preamble/DF17 gate + slice
 * of the survivors) but not the finishing kernel -- no survivor is CRC-checked, the header reports an empty list, so
 * NO frames come out.  on = 0 restores the full path. */
int adsb_debug_fused_pass_only(adsb_ctx *ctx, int on);
/* Which scan kernel an i8 context launches: 1 = floor(sqrt) per sample, the product's and the default (ADSB_SCAN=root or
 * unset in the environment at adsb_create); 0 / 2 / 3 / 4 = the A/B kernels of rounds 3-4 (ADSB_SCAN=nsq / reg / code / sieve;
 * only in builds with -DADSB_AB_KERNELS=1: the gate on I^2+Q^2, the same from registers, on an 8-bit log code, on two relation
 * bits per sample).  Same results; DESIGN.md sections 4.1b-d have the measurements.  Always 1 for CS16 (one kernel). */
int adsb_debug_scan(adsb_ctx *ctx);
/* The code scan's table as this device computes it, for n = I^2+Q^2 = 0 .. 32768: out[n] = c(n) | th(n) << 8 (c = the
 * 8-bit code of n, th = the threshold code of the gate's slack for a "high" of that code).  Returns ADSB_E_STATE if the
 * table does not have the properties the kernel's superset test rests on (adsb_create checks the same). */
int adsb_debug_code_table(adsb_ctx *ctx, uint16_t *out32769);
/* Test knob: with on != 0 the shared slot pool of the following launches hands out nothing, so every tile with
 * more gate survivors than its own 32 slots loses them: the launch's list comes out with ADSB_FLAG_INCOMPLETE (for
 * device-side consumers) and the host entry points take their re-run path -- deterministically. */
int adsb_debug_pool_limit(adsb_ctx *ctx, int on);
/* Test knob: the next launch counts as launch number `idx`.  finish_order tags its exchange words with the launch's epoch
 * ((index + 1) mod 2^30) and the library zeroes them whenever the epoch wraps: this lets a test cross the wrap. */
int adsb_debug_set_launch_index(adsb_ctx *ctx, uint32_t idx);
/* Test knob: workgroup `blk` of finish_order withholds its exchange word in the following launches (0xFFFFFFFF: none).
 * The workgroups behind it give up after ~0.1 s: adsb_fetch / adsb_fetch_counts return ADSB_E_STATE, the header carries
 * ADSB_FLAG_INCOMPLETE, nothing hangs, and the context stays usable (the reference's only failure mode is a closed
 * channel, src/adsb.rs:108-111: the replacement must not add a hang). */
int adsb_debug_finish_stall(adsb_ctx *ctx, uint32_t blk);
/* finish_order's constants (each may be NULL), for tests: tiles per workgroup; workgroups whose totals one second-level
 * sum holds; the largest number of workgroups that still exchange their totals in one level; second-level sums a
 * workgroup reads per round.  These are the sizes at which the kernel takes another path.  The list does not depend on
 * them. */
int adsb_debug_finish_geometry(uint32_t *tiles_per_workgroup, uint32_t *fan, uint32_t *flat, uint32_t *sums_per_round);
/* Diagnostic builds of demod_tiles (-DADSB_TILE_STAMPS=1) only: 16 uint32 per tile of the last launch (waves 0
 * and 3 of the tile's workgroup, 8 each: shader cycles in prologue, phase 1, barrier, phase 2, barrier, phase 3,
 * wait for the loads; s_memrealtime at start).  ADSB_E_STATE in a normal build. */
int adsb_debug_tile_stamps(adsb_ctx *ctx, uint32_t *out16_per_tile, size_t max_tiles, size_t *n_tiles);
/* ---- deterministic synthetic IQ source --------------------------------------- */
typedef struct adsb_synth_cfg {
    uint64_t seed;
    uint32_t slot_len;     /* one frame slot per slot_len samples (>= 256); 2000 = ~1000 msg/s */
    uint32_t frame_pct;    /* 0..100: share of slots that carry a frame                        */
    uint32_t pct_flip_data;/* of the frames: one flipped data bit  (must be repaired)          */
    uint32_t pct_flip_crc; /* of the frames: one flipped CRC bit   (must be rejected)          */
    uint32_t pct_flip_two; /* of the frames: two flipped data bits (must be rejected)          */
    uint32_t noise_div;    /* noise = (sum of 4 hash bytes - 510) / noise_div; 18 -> sigma~8   */
    uint32_t amp_shift;    /* i16 only: left shift applied to the i8-scale value (0..7)        */
    uint32_t reserved;
} adsb_synth_cfg;

void adsb_synth_default(adsb_synth_cfg *cfg);
/* Sample k of channel `channel` depends only on (cfg, channel, k): any slice of the stream can be
 * generated independently (time-sharding across GPUs needs no input exchange). */
int adsb_synth_fill_host(const adsb_synth_cfg *cfg, int sample_type, uint32_t channel,
                         uint64_t first_sample, size_t n_samples, void *iq_host);
int adsb_synth_fill_device(adsb_ctx *ctx, const adsb_synth_cfg *cfg, uint32_t channel,
                           uint64_t first_sample, size_t n_samples, void *iq_dev);
/* Threads of the grid adsb_synth_fill_device launches (may be NULL): a longer range sends threads round the kernel's
 * loop for a second sample, for tests.  The stream does not depend on it. */
int adsb_debug_synth_geometry(uint32_t *threads);
/* The frame (and what the demodulator must make of it) planted in slot `slot`:
 * returns 1 if the slot carries a frame; start = first preamble sample (absolute),
 * clean14 = the error-free frame, kind: 0 clean, 1 data-bit flip, 2 crc-bit flip, 3 two flips. */
int adsb_synth_slot(const adsb_synth_cfg *cfg, uint32_t channel, uint64_t slot, uint64_t *start,
                    uint8_t clean14[14], uint8_t sent14[14], int *kind);

#ifdef __cplusplus
}
#endif
#endif /* ADSB_HIP_H */
