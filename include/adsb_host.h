/*
 * adsb_host.h -- C ABI over the host-side mirror of air_rs's thread structure (libadsb_hip.so).
 *
 * The reference is a Rust binary with no Rust toolchain in this image, so the host side above
 * include/adsb_hip.h is written in C++ (air_rs_amd/csrc/host/) with the reference's names:
 * AdsbPacket (src/adsb/packet.rs:9-99), AircraftID / AircraftPosition / UknownMsg
 * (src/adsb/msgs.rs), playback_thread (src/adsb.rs:75-89), process_sdr_data_thread
 * (src/adsb.rs:92-122), load_data/save_data (src/utils.rs:6-43).  These C entry points exist so
 * tests (ctypes) and other languages can drive that C++.
 */
#ifndef ADSB_HOST_H
#define ADSB_HOST_H

#include "adsb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { ADSB_MSG_AIRCRAFT_ID = 0, ADSB_MSG_AIRCRAFT_POSITION = 1, ADSB_MSG_UNKNOWN = 2 };

/* Flat view of AdsbPacket (packet.rs:9-18) + its AdsbMsgType variant (msgs.rs:6-11). */
typedef struct adsb_packet_view {
    uint8_t  packet[14];
    uint8_t  downlink_format;      /* packet.rs:26 */
    uint8_t  capability;           /* packet.rs:27 (mask 5, as in the reference) */
    uint32_t icao;                 /* packet.rs:28 */
    uint8_t  msg_type;             /* packet.rs:29 */
    int32_t  msg_kind;             /* ADSB_MSG_* */
    char     callsign[9];          /* AircraftID, NUL terminated */
    uint8_t  surveillance_status;  /* AircraftPosition ... */
    uint8_t  nic_supplement;
    int32_t  altitude;
    uint8_t  cpr_time;
    uint8_t  cpr_odd;
    uint32_t cpr_latitude;
    uint32_t cpr_longitude;
    uint8_t  raw_msg[10];          /* UknownMsg: packet[4..14] */
} adsb_packet_view;

/* AdsbPacket::new (packet.rs:25-49). */
int adsb_packet_new(const uint8_t bytes[14], adsb_packet_view *out);
/* AdsbPacket::_new_from_string (packet.rs:56-68): 28 hex digits. */
int adsb_packet_new_from_string(const char *hex, adsb_packet_view *out);
/* `impl Display for AdsbPacket` (packet.rs:77-99).  time_text replaces the wall-clock value of
 * the "Processed Time" line.  Returns the text length (without NUL); writes only if cap suffices. */
size_t adsb_packet_display(const uint8_t bytes[14], const char *time_text, char *dst, size_t cap);

/*
 * launch_adsb in playback + stream mode (adsb.rs:126-173): thread 1 = playback_thread over
 * `data`, thread 2 = process_sdr_data_thread on `ctx` (GPU), thread 3 collects what the stream
 * printer would print ("\n{packet}\n" per packet, adsb.rs:157).
 *   sample_type : layout of `data`; ADSB_E_ARG unless it is the sample type the ctx was created with
 *   chunk_len   : samples per buffer (20000 in the reference); the tail is dropped as in adsb.rs:77
 *   frames/max_frames/n_frames : the frames behind the packets, offsets absolute in `data`
 *   text/text_cap/text_len     : optional stream-mode text, "Processed Time" lines blanked
 * Returns ADSB_OK or the first error thread 2 met.
 */
int adsb_pipeline_playback(adsb_ctx *ctx, int sample_type, const void *data, size_t n_samples,
                           size_t chunk_len, adsb_frame *frames, size_t max_frames, size_t *n_frames,
                           uint64_t *n_buffers, char *text, size_t text_cap, size_t *text_len);

/*
 * The same three threads with carry-over switched on in thread 2 (NOT reference
 * behaviour): the last 240 samples of every buffer are prepended to the next, so frames straddling
 * two buffers -- which the reference loses (adsb.rs:95-98) -- are decoded, and the chunked stream
 * yields exactly what one long buffer of the samples actually sent would.  The ctx must have been
 * created for max_samples >= chunk_len + 240.  (Both entry points run thread 2 on the streaming front end,
 * adsb_feed_*: pinned ring, asynchronous DMA, the 240-sample tail kept on the device.)
 */
int adsb_pipeline_playback_carry(adsb_ctx *ctx, int sample_type, const void *data, size_t n_samples,
                                 size_t chunk_len, adsb_frame *frames, size_t max_frames,
                                 size_t *n_frames, uint64_t *n_buffers);


/*
 * The general form of the two entry points above, and the replay entry: what
 * `air_rs adsb -p FILE -m stream` does (main.rs:19-23 -> launch_adsb, adsb.rs:126-173) with thread 2 on the GPU.
 *   flags: ADSB_REPLAY_CARRY      thread 2 carries the last 240 samples over (not reference behaviour)
 *          ADSB_REPLAY_SEND_TAIL  the playback thread also sends the last full or partial chunk, which
 *                                 adsb.rs:77's strict `<` never sends (not reference behaviour)
 *          0 reproduces the reference: per-buffer demodulation, tail dropped.
 * adsb_replay_file reads the whole file like utils.rs:22-43 (ADSB_FILE_C16: raw little-endian i16 I,Q pairs, the
 * reference's `.c16`; the ctx must be ADSB_SAMPLE_I16) or as a raw rtl_sdr capture (ADSB_FILE_U8: unsigned bytes
 * re-centred as x - 128; the ctx must be ADSB_SAMPLE_I8; not a format the reference reads), cuts it into
 * chunk_len-sample buffers (20000 in the reference) and returns the frames (offsets absolute in the file) and the
 * stream-mode text ("\n{packet}\n" per packet, adsb.rs:157, "Processed Time" values blanked).  The ctx must have
 * been created for max_samples >= chunk_len + 240.
 */
#define ADSB_REPLAY_CARRY 0x1u
#define ADSB_REPLAY_SEND_TAIL 0x2u
#define ADSB_FILE_C16 0
#define ADSB_FILE_U8 1
int adsb_pipeline_run(adsb_ctx *ctx, int sample_type, const void *data, size_t n_samples, size_t chunk_len,
                      uint32_t flags, adsb_frame *frames, size_t max_frames, size_t *n_frames, uint64_t *n_buffers,
                      char *text, size_t text_cap, size_t *text_len);
int adsb_replay_file(adsb_ctx *ctx, const char *path, int file_format, size_t chunk_len, uint32_t flags,
                     adsb_frame *frames, size_t max_frames, size_t *n_frames, uint64_t *n_buffers,
                     uint64_t *n_samples, char *text, size_t text_cap, size_t *text_len);

/*
 * CPU mirror of adsb_levels_of (adsb_hip.h, "Per-frame signal and noise power"): the same records, in plain C++,
 * from a one-channel HOST buffer of n_samples interleaved samples of sample_type.  Frame i sits at sample
 * frames[i].offset - first_sample_index; a frame whose 240-sample window is not wholly inside [0, n_samples) gets
 * flags = 0 and zeros, and nothing of it is read.  What a feed's consumer, who holds the host buffer, uses.
 * ADSB_E_ARG for a bad sample_type, NULL iq, or NULL frames / out with n > 0.
 */
int adsb_host_frame_levels(int sample_type, const void *iq, size_t n_samples, uint64_t first_sample_index,
                           const adsb_frame *frames, size_t n, adsb_frame_level *out);
/* CPU mirror of adsb_levels_modes_of (adsb_hip.h, "Level records by frame length"): the same records from the same
 * per-frame program text as the device's, from a HOST buffer of n_channels channels channel_stride samples apart.
 * frames[n] in channel order with counts[n_channels] that add up to n, all host memory; a short frame (bytes[0] >> 3
 * below 16) gets the 128-sample record with ADSB_LEVEL_SHORT, a long one adsb_host_frame_levels' record.  The same
 * argument errors as adsb_levels_modes_of, and ADSB_E_ARG for a bad sample_type or NULL out with n > 0. */
int adsb_host_frame_levels_modes(int sample_type, const void *iq, uint32_t n_channels, size_t n_samples,
                                 size_t channel_stride, uint64_t first_sample_index, const adsb_frame *frames,
                                 const uint64_t *counts, size_t n, adsb_frame_level *out);
/* 10 log10(sum / n_samples / FS) with FS = 32768 (ADSB_SAMPLE_I8) or 2^31 (ADSB_SAMPLE_I16): the mean power of
 * n_samples samples whose p add up to `sum`, in dB below a full-scale sample.  -INFINITY for sum == 0; NaN for a bad
 * sample_type or n_samples == 0.  adsb_level_dbfs(st, level.signal_sum, 116) and (st, level.noise_sum, 124); 60 and 68
 * for a record with ADSB_LEVEL_SHORT. */
double adsb_level_dbfs(int sample_type, uint64_t sum, uint32_t n_samples);

/*
 * CPU mirror of adsb_wire_of (adsb_hip.h, "Wire output"): the same bytes from the same program text as the device's, no
 * device needed.  frames[n] with levels[n] (NULL: s = 0), both host memory; sample_type gives the signal byte's full
 * scale.  out / cap / *n_bytes as adsb_fetch_wire: the whole stream if cap holds it, else the longest prefix of whole
 * frames, and *n_bytes = the stream's full length either way; ends (may be NULL) receives all n entries.  What a
 * feed's consumer uses on popped frames, together with adsb_host_frame_levels.  cfg->format takes ADSB_WIRE_SHORT as
 * adsb_wire_of's does.  ADSB_E_ARG for a NULL cfg or n_bytes,
 * an unknown format, tick_bias >= 2^48, a bad sample_type, NULL frames with n > 0 or NULL out with cap > 0;
 * ADSB_E_CAPACITY when 44 x n does not fit uint32.
 */
int adsb_host_wire_encode(const adsb_wire_cfg *cfg, int sample_type, const adsb_frame *frames,
                          const adsb_frame_level *levels /* NULL: s = 0 */, size_t n, uint8_t *out, size_t cap,
                          size_t *n_bytes, uint32_t *ends);

/*
 * CPU mirror of adsb_wire_in_of + adsb_fetch_wire_in (adsb_hip.h, "Wire input"): the same outputs from the same program
 * text as the device's, no device needed.  bytes and stream_ends as there, all host memory.  frames, rx and levels
 * (each may be NULL; levels is filled only with cfg.levels != 0) receive min(header.n_frames, max) entries and *n
 * (optional) that number; counts[n_streams], consumed[n_streams] and *header are optional.  What a feed-side consumer
 * without a GPU uses.  The same argument errors as adsb_wire_in_of.
 */
int adsb_host_wire_parse(const adsb_wire_in_cfg *cfg, const uint8_t *bytes, size_t n_bytes, const uint64_t *stream_ends,
                         uint32_t n_streams, adsb_frame *frames, adsb_wire_rx *rx, adsb_frame_level *levels, size_t max,
                         size_t *n, uint64_t *counts, uint64_t *consumed, adsb_wire_in_header *header);

/*
 * CPU mirror of adsb_correlate_of (adsb_hip.h, "Correlate"): the same messages, frames and receptions, built from the
 * same key compare, head rule and aggregate combine as the device's, no device needed.  frames[n] with levels[n] (NULL:
 * best_receiver 0xFFFF), counts[n_receivers] and sample_base[n_receivers] (NULL: all 0), all host memory.  recs
 * receives all n receptions; msgs and frames_out (either may be NULL) receive min(*n_msgs, max_msgs) entries, and
 * *n_msgs = the message count whatever max_msgs.  What a feed's consumer that holds several receivers' popped lists
 * uses.  ADSB_E_ARG for a NULL cfg, counts or n_msgs, n_receivers outside 1..256, counts not summing to n, NULL frames
 * or recs with n > 0; ADSB_E_CAPACITY for n >= 2^32.
 */
int adsb_host_correlate(const adsb_correlate_cfg *cfg, const adsb_frame *frames, const adsb_frame_level *levels, size_t n,
                        const uint64_t *counts, uint32_t n_receivers, const uint64_t *sample_base, adsb_message *msgs,
                        size_t max_msgs, size_t *n_msgs, adsb_frame *frames_out, adsb_reception *recs);

/*
 * CPU mirror of adsb_modes_of + adsb_fetch_modes (adsb_hip.h, "Mode S replies"): the same records, known_out, squitters
 * and header from the same program text as the device's, on one core, no device needed.  All arrays host memory.
 * recs[n] and squitters (room for n) may each be NULL; known_out (room for n + n_known_in, may be NULL) receives
 * header.n_known_out addresses; squitter_counts[n_receivers] is written when counts is given; *header is optional.
 * The same argument errors as adsb_modes_of.
 */
int adsb_host_modes(const adsb_frame *frames, size_t n, const uint64_t *counts, uint32_t n_receivers,
                    const uint32_t *known_in, size_t n_known_in, adsb_modes_rec *recs, uint32_t *known_out,
                    adsb_frame *squitters, uint64_t *squitter_counts, adsb_modes_header *header);

/*
 * CPU mirror of adsb_commb_of + adsb_fetch_commb (adsb_hip.h, "Comm-B registers"): the same records and header from
 * the same program text as the device's, on one core, no device needed.  frames host memory; recs[n] and *header may
 * each be NULL.  ADSB_E_ARG for NULL frames with n > 0; ADSB_E_CAPACITY for n >= 2^32.
 * commb_as decodes the MB field of one frame as the register `bds` (0x10, 0x17, 0x20, 0x30, 0x40, 0x50, 0x60),
 * whatever the inference says: *rec has state ONE, that bds and its values, with candidates and n_candidates as the
 * inference fills them.  A consumer that knows more settles an AMBIGUOUS record with it; the usual one is a tracker
 * that has the aircraft's ADS-B velocity.  ADSB_E_ARG for NULL bytes or rec, or a bds that is not among the frame's
 * candidates (so for every frame that is not DF20/21 and every empty MB); *rec is then left as it was.
 */
int adsb_host_commb(const adsb_frame *frames, size_t n, adsb_commb_rec *recs, adsb_commb_header *header);
int adsb_host_commb_as(const uint8_t bytes[14], uint32_t bds, adsb_commb_rec *rec);

/*
 * CPU mirror of adsb_es_of + adsb_fetch_es (adsb_hip.h, "Extended squitter status"): the same records and header from
 * the same program text as the device's, on one core, no device needed.  frames host memory; recs[n] and *header may
 * each be NULL.  ADSB_E_ARG for NULL frames with n > 0; ADSB_E_CAPACITY for n >= 2^32.
 * es_integrity: the navigation integrity category and the containment radius Rc in decimetres (0: unknown) of a
 * position message with type code tc, from an aircraft of ADS-B `version` whose NIC supplements are `supp` (bit 0 = A
 * and bit 2 = C from its operational status, bit 1 = B from the position message itself).  A version from 3 on reads
 * as 2, ADSB_ES_VERSION_UNKNOWN as 0; version 0 has no NIC (its NUCp is another scale) and reports 0; version 1
 * ignores B and C.  Each of *nic and *rc_dm may be NULL; always ADSB_OK.  THE TABLE, Rc in metres, "-" unknown:
 *     TC          version 0   version 1 and 2: NIC, Rc
 *     0, 18, 22   -           0, -
 *     9, 20       7.5         11, 7.5
 *     10, 21      25          10, 25
 *     11          185.2       9, 75 with A (v1) or A and B (v2); else 8, 185.2
 *     12          370.4       7, 370.4
 *     13          926         6; v1: 1111.2 with A, else 926; v2: 1111.2 with A, else 555.6 with B, else 926
 *     14          1852        5, 1852
 *     15          3704        4, 3704
 *     16          18520       3, 7408 with A (v1) or A and B (v2); else 2, 14816
 *     17          37040       1, 37040
 *     5           7.5         11, 7.5
 *     6           25          10, 25
 *     7           185.2       9, 75 with A (v1) or A and not C (v2); else 8, 185.2
 *     8           -           v1: 0, -; v2: A and C: 7, 370.4; A alone: 6, 555.6; C alone: 6, 1111.2; neither: 0, -
 *     any other   -           0, -
 *   The table was written down from memory of RTCA DO-260B table N-4 and of readsb's compute_nic / compute_rc, without
 *   either at hand: compare before relying on a row.
 */
int adsb_host_es(const adsb_frame *frames, size_t n, adsb_es_rec *recs, adsb_es_header *header);
int adsb_host_es_integrity(uint32_t tc, uint32_t version, uint32_t supp, uint32_t *nic, uint32_t *rc_dm);

/*
 * CPU mirror of adsb_replies_of + adsb_fetch_replies (adsb_hip.h, "Mode S replies from samples"): the same list, counts
 * and header from the same program text as the device's, on one core, no device needed.  iq is HOST memory of
 * n_channels buffers of n_samples interleaved samples of sample_type, channel_stride samples apart (any alignment;
 * ignored for one channel); known host memory.  out (may be NULL with max_out 0) receives min(header.n_out, max_out)
 * frames and *n_out (optional) that number; counts[n_channels] and *header are optional.  The capacity cfg.max_frames =
 * 0 stands for is unbounded here (there is no ctx).  What a feed's consumer, who holds the host buffer, uses.  The same
 * argument errors as adsb_replies_of but for alignment and the ctx's sizes; ADSB_E_ARG also for a bad sample_type or
 * NULL out with max_out > 0.
 * merge_lists mirrors adsb_merge_lists_of: all arrays host memory; src and counts_out may be NULL.
 */
int adsb_host_replies(int sample_type, const adsb_replies_cfg *cfg, const void *iq, uint32_t n_channels, size_t n_samples,
                      size_t channel_stride, const uint32_t *known, size_t n_known, adsb_frame *out, size_t max_out,
                      size_t *n_out, uint64_t *counts, adsb_replies_header *header);
int adsb_host_merge_lists(const adsb_frame *a, const uint64_t *counts_a, const adsb_frame *b, const uint64_t *counts_b,
                          uint32_t n_channels, adsb_frame *out, uint32_t *src, uint64_t *counts_out);

/*
 * CPU mirror of adsb_multilaterate_of (adsb_hip.h, "Multilaterate"): the same fixes and header from the same program text
 * as the device's -- the solver, and the 16 partial sums of every sum over receptions folded in the same butterfly -- on
 * one core, no device needed.  All arrays host memory; rx / n_rx may be NULL / 0 with ADSB_MLAT_TIME_RECEPTION; fixes
 * receives n_msgs records; *header is optional.  The same argument errors as adsb_multilaterate_of, and ADSB_E_ARG for
 * NULL fixes with n_msgs > 0; ADSB_E_ARG after writing everything when a message has ADSB_MLAT_BAD_INDEX.
 */
int adsb_host_multilaterate(const adsb_mlat_cfg *cfg, const adsb_mlat_receiver *receivers, uint32_t n_receivers,
                            const adsb_message *msgs, size_t n_msgs, const adsb_reception *recs, size_t n_recs,
                            const adsb_wire_rx *rx, size_t n_rx, adsb_mlat_fix *fixes, adsb_mlat_header *header);

/*
 * CPU mirror of adsb_clock_sync_of (adsb_hip.h, "Clock sync"): the same clocks and header from the same program text as
 * the device's -- the rows, the pair order, the 64 partial sums folded in the same butterfly, the normal equations, the
 * factorisation and the second pass -- on one core, no device needed.  All arrays host memory; clocks receives
 * n_receivers records; *header is optional; row_state (optional) receives one byte per reception slot: 0 empty, 1 a kept
 * row, 2 a dropped row.  The same argument errors as adsb_clock_sync_of, and ADSB_E_ARG for NULL clocks; ADSB_E_ARG after
 * writing everything when the header has ADSB_CLOCK_HDR_BAD_INDEX.
 */
int adsb_host_clock_sync(const adsb_clock_cfg *cfg, const adsb_mlat_receiver *receivers, uint32_t n_receivers,
                         const adsb_message *msgs, size_t n_msgs, const adsb_reception *recs, size_t n_recs,
                         const adsb_wire_rx *rx, size_t n_rx, adsb_clock *clocks, adsb_clock_header *header,
                         uint8_t *row_state);
/* CPU mirror of adsb_clock_apply: corrected[n_recs] from clocks[n_receivers] (of which offset_s and drift are read) and
 * the cfg and lists of the sync.  The argument errors of adsb_host_clock_sync (receivers are not needed), and ADSB_E_ARG
 * for NULL clocks, or NULL corrected with n_recs > 0. */
int adsb_host_clock_apply(const adsb_clock_cfg *cfg, const adsb_clock *clocks, uint32_t n_receivers,
                          const adsb_message *msgs, size_t n_msgs, const adsb_reception *recs, size_t n_recs,
                          const adsb_wire_rx *rx, size_t n_rx, adsb_reception *corrected);

/*
 * CPU mirror of the per-frame fix decode of a table or bank with a fixes reserve (adsb_hip.h, "Positions from single
 * messages"): the same program text as the device's, no device needed.  *out = the adsb_fix of an aircraft whose only
 * frame since admission is this one, heard at frame time `time` by a receiver at *site: accepted: the fix with
 * n_fixes = 1; rejected: the empty fix with n_rejected = 1; no position message: the empty fix.  *frame_flags
 * (optional) = the frame's adsb_frame_fix.flags.  ADSB_E_ARG for a NULL site, bytes or out, or a site that
 * adsb_track_table_fixes_reserve would refuse.
 */
int adsb_host_fix_of(const adsb_site *site, const uint8_t bytes[14], double time, adsb_fix *out, uint32_t *frame_flags);

/*
 * CPU mirror of the per-frame step of a table with an mlat reserve (adsb_hip.h, "Multilaterated positions per
 * aircraft"): the same program text as the device's, no device needed.  *out = the adsb_aircraft_mlat of an aircraft
 * whose only counted frame since admission is this one, with fix *fix, heard at frame time `time`, under the limit
 * max_disagreement_m.  *frame_flags and *disagreement_m (each optional) = the frame's adsb_frame_mlat.flags and
 * disagreement_m.  ADSB_E_ARG for NULL bytes, fix or out, or a limit that adsb_track_table_mlat_reserve would refuse.
 */
int adsb_host_track_mlat_of(double max_disagreement_m, const uint8_t bytes[14], const adsb_mlat_fix *fix, double time,
                            adsb_aircraft_mlat *out, uint32_t *frame_flags, float *disagreement_m);

/*
 * CPU mirror of a table's filter reserve (adsb_hip.h, "Filtered mlat track per aircraft"): the same program text as the
 * device's, no device needed.  cfg NULL: every default; a cfg as adsb_track_table_filter_reserve takes it.
 * filter_operand: *operand = the operand of a frame with fix *fix at frame time `time`; counted 0: a frame of an aircraft
 * the table turned away (64 zero bytes).  filter_step: *record (EMPTY: all zeros with time NaN) becomes the record after
 * a frame with *operand, and *frame_out (optional) that frame's adsb_frame_filter; an operand that is not usable leaves
 * the record alone.  ADSB_E_ARG for a NULL fix, operand or record, or a cfg the reserve would refuse.
 */
int adsb_host_track_filter_operand(const adsb_track_filter_cfg *cfg, const adsb_mlat_fix *fix, double time, int counted,
                                   adsb_filter_operand *operand);
int adsb_host_track_filter_step(const adsb_track_filter_cfg *cfg, adsb_aircraft_filter *record,
                                const adsb_filter_operand *operand, adsb_frame_filter *frame_out);

/*
 * CPU mirror of the per-frame step and the combine of a table with a modes reserve (adsb_hip.h, "Mode S replies per
 * aircraft"): the same program text as the device's, no device needed.  track_modes_of: *accepted (optional) = 1 iff
 * the record's kind is SELF or KNOWN; *one = the adsb_aircraft_modes of an aircraft whose only counted frame since
 * admission is this one, heard at frame time `time` (the EMPTY record for a frame that is not accepted).
 * track_modes_merge: *into becomes *into followed by *later, a record of the frames that come after into's: the
 * combine the device's segment tails apply.  ADSB_E_ARG for a NULL rec, one, into or later.
 */
int adsb_host_track_modes_of(const adsb_modes_rec *rec, double time, adsb_aircraft_modes *one, uint32_t *accepted);
int adsb_host_track_modes_merge(adsb_aircraft_modes *into, const adsb_aircraft_modes *later);

/*
 * CPU mirror of the Comm-B step of a table with a commb reserve (adsb_hip.h, "Comm-B registers per aircraft"): the same
 * program text as the device's, no device needed.
 * commb_settle: *out = the per-frame output of a COUNTED frame with these bytes and stateless record *rec, heard at
 * frame time `time`, against the reference *reference (NULL, or subtype 0: none); cfg NULL: the reserve's defaults.
 * *out is *rec byte for byte unless the frame is settled.  rec and out may be the same.
 * commb_reference: the fields of an adsb_velocity that the rule reads, from the 14 bytes of a DF17/18 TC 19 frame heard
 * at `time` (integers only: speed_kt and direction_deg are filled for ST 3-4 and left 0 for ST 1-2); subtype 0 for ST 0
 * and 5-7.  It is what the device reads for a reference in the current list.
 * track_commb_of: *one = the adsb_aircraft_commb of an aircraft whose only counted frame since admission has the
 * per-frame output *rec, heard at `time` (the EMPTY record for NOT_COMMB).  track_commb_merge: *into becomes *into
 * followed by *later, a record of the frames that come after into's: the combine the device's segment tails apply.
 * ADSB_E_ARG for a NULL bytes, rec, out, reference (commb_reference), one, into or later, or a cfg whose max_age_s is
 * NaN or negative.
 */
int adsb_host_commb_settle(const uint8_t bytes[14], const adsb_commb_rec *rec, const adsb_velocity *reference, double time,
                           const adsb_commb_settle_cfg *cfg, adsb_commb_rec *out);
int adsb_host_commb_reference(const uint8_t bytes[14], double time, adsb_velocity *reference);
int adsb_host_track_commb_of(const adsb_commb_rec *rec, double time, adsb_aircraft_commb *one);
int adsb_host_track_commb_merge(adsb_aircraft_commb *into, const adsb_aircraft_commb *later);

/*
 * CPU mirror of the extended squitter step of a table with an es reserve (adsb_hip.h, "Extended squitter status per
 * aircraft"): the same program text as the device's, no device needed.
 * es_resolve: *out = the per-frame output of a frame with stateless record *rec heard at frame time `time`, whose key
 * and point let it count, of an aircraft whose record before the frame is *held (NULL: the empty record): read from it
 * are version / version_time, nic_a / nic_a_time and nic_c / nic_c_time, a time of NaN meaning "none".  For a position
 * message that is NIC and Rc resolved by adsb_host_es_integrity's table; all zero for a record whose state is NOT_ES or
 * FOREIGN.  cfg NULL: the reserve's default, max_age_s = 60.0.
 * track_es_of: *one = the adsb_aircraft_es of an aircraft whose only counted frame since admission has the record *rec
 * and the per-frame output *integrity, heard at `time` (the EMPTY record if *integrity is not COUNTED).
 * track_es_merge: *into becomes *into followed by *later, a record of the frames that come after into's: the combine
 * the device's segment tails apply.  A table's record after a list is the fold of these three over the aircraft's
 * frames in list order.
 * ADSB_E_ARG for a NULL rec, out, integrity, one, into or later, or a cfg whose max_age_s is NaN or negative.
 */
int adsb_host_es_resolve(const adsb_es_rec *rec, double time, const adsb_aircraft_es *held /* may be NULL */,
                         const adsb_es_track_cfg *cfg /* may be NULL */, adsb_frame_integrity *out);
int adsb_host_track_es_of(const adsb_es_rec *rec, const adsb_frame_integrity *integrity, double time,
                          adsb_aircraft_es *one);
int adsb_host_track_es_merge(adsb_aircraft_es *into, const adsb_aircraft_es *later);

/* ---- behind the channel: tracker + CPR ------------------------------------------- */

/* cpr.rs:39-54 calc_num_zones; cpr.rs:135-147 calculate_geographic_position (returns 1 = Some, 0 = None).
 * first_is_odd: the OLDER message's CPR format (`first`), 0 = Even, 1 = Odd. */
uint32_t adsb_cpr_num_zones(double latitude);
int adsb_cpr_position(uint32_t even_lat, uint32_t even_lon, uint32_t odd_lat, uint32_t odd_lon, int first_is_odd,
                      double *latitude, double *longitude);

/* AircraftSummary (aircraft.rs:14-23) */
typedef struct adsb_aircraft_summary {
    uint32_t icao;
    char     callsign[9];   /* "" while None */
    int32_t  altitude;
    int32_t  has_position;  /* geo_position.is_some() */
    double   latitude, longitude;
    double   last_contact;  /* seconds on the caller's clock (the reference: wall clock) */
} adsb_aircraft_summary;

/* The `HashMap<u32, Aircraft>` of the display threads + handle_aircraft_update (aircraft.rs:158-165). */
typedef struct adsb_tracker adsb_tracker;
adsb_tracker *adsb_tracker_create(void);
void adsb_tracker_destroy(adsb_tracker *t);
/* Feeds one packet (time_s stands in for AdsbPacket::time_processed).  Returns 1 if the packet produced a
 * new geographic position, 0 if not, < 0 on error; *out (optional) = the aircraft's summary afterwards. */
int adsb_tracker_update(adsb_tracker *t, const uint8_t bytes[14], double time_s, adsb_aircraft_summary *out);
size_t adsb_tracker_count(const adsb_tracker *t);
/* Summary of one aircraft; ADSB_E_ARG if the ICAO address has not been seen. */
int adsb_tracker_get(const adsb_tracker *t, uint32_t icao, adsb_aircraft_summary *out);

/* utils.rs:22-43 / 6-20.  adsb_load_c16 allocates *data with malloc (free with adsb_free). */
int adsb_load_c16(const char *path, int16_t **data, size_t *n_samples);
int adsb_save_c16(const char *path, const int16_t *data, size_t n_samples);
/* Raw rtl_sdr capture: interleaved unsigned bytes I,Q (zero level 127.5).  Not a reference format; samples
 * are re-centred as x - 128 into the ADSB_SAMPLE_I8 layout.  *data is malloc'ed (free with adsb_free);
 * ADSB_E_ARG for an unreadable file or an odd length. */
int adsb_load_u8(const char *path, int8_t **data, size_t *n_samples);
void adsb_free(void *p);

#ifdef __cplusplus
}
#endif
#endif
