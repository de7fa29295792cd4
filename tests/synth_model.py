"""Independent NumPy model of the synthetic IQ source (air_rs_amd/csrc/adsb_synth.h, include/adsb_hip.h "deterministic
synthetic IQ source"), written from the rules and shared by the CPU tier (tests/test_synth_model.py: host fill == model)
and the GPU tier (tests/test_gpu_synth.py: device fill == host fill == model).  Calls no library entry point.

The rules.  The stream of channel c is cut into slots of slot_len samples; slot s draws three 64-bit words
    h  = mix64(seed ^ c * CH ^ s * SL ^ TAG),  h2 = mix64(h),  h3 = mix64(h2)
and reads its fields out of them (FIELDS below: a shift and a modulus or mask each).  A slot carries a frame when
`roll` < frame_pct; the frame's first sample is `jitter` = (h >> 8) mod (slot_len - 240) samples into the slot, so the
240 samples never leave the slot.  A frame is DF17 / CA5 (0x8D), a 24-bit address, a type code of one of three ranges
(1-4, 9-18, 19-28), 51 more payload bits and the Mode-S CRC-24 of those 11 bytes; what is SENT is that frame with, by
`kind`, nothing flipped (0), one bit of the first 88 (1), one bit of the last 24 (2) or two distinct bits of the first
88 (3); kind is chosen by `kroll` against the running sums of pct_flip_data, pct_flip_crc, pct_flip_two.  On the air a
frame is 240 half-microsecond positions: pulses at 0, 2, 7, 9 of the 16 preamble positions, then two positions per bit,
pulse first for a 1 and pulse second for a 0.  A pulse adds the slot's amplitude pair (one of eight) to the noise, which
for sample k is drawn from mix64(seed ^ c * CH ^ k * NZ): I from the sum of its four low bytes, Q from its four high
bytes, each minus 510 and divided by noise_div the way C divides (toward zero).  i8 clips the sum to [-128, 127]; i16
shifts it left by amp_shift first and clips to [-32768, 32767].

Everything is vectorised: the slot table is computed once for all slots a range touches, the samples over
k = first + arange(n) in wrapping uint64 arithmetic."""
import functools
import types

import numpy as np

from tests.hostile_traffic import crc24

I8, I16 = 0, 1          # ADSB_SAMPLE_I8 / ADSB_SAMPLE_I16
FRAME = 240
U = np.uint64
CH, SL, NZ, TAG = U(0xD1B54A32D192ED03), U(0x9FB21C651E98DF25), U(0xC2B2AE3D27D4EB4F), U(0x5157415453594E54)
AMPS = np.array([(40, 0), (0, 50), (45, 45), (60, -30), (-70, 20), (80, 40), (-64, -64), (100, 45)], dtype=np.int64)
PREAMBLE = (0, 2, 7, 9)
# name: (word, shift, "mod" | "mask", operand)
FIELDS = {"roll": (0, 0, "mod", 100), "amp": (0, 40, "mask", 7), "kroll": (0, 44, "mod", 100),
          "address": (1, 0, "mask", 0xFFFFFF), "tc_range": (1, 24, "mod", 3), "tc_low": (1, 28, "mask", 3),
          "tc_mid": (1, 28, "mod", 10), "tc_sub": (1, 36, "mask", 7),
          "payload": (2, 0, "mask", (1 << 48) - 1), "flip0": (2, 48, "mod", 88), "flip1": (2, 56, "mod", 87),
          "flip_crc": (2, 48, "mod", 24)}


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def mix64(x):
    """The splitmix64 finaliser, on uint64 arrays (wrapping)."""
    x = _u64(x) + U(0x9E3779B97F4A7C15)
    x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
    return x ^ (x >> U(31))


def _channel_word(cfg, channel):
    return U(cfg.seed) ^ (_u64(channel & 0xFFFFFFFF) * CH)


def slots(cfg, channel, slot_numbers):
    """The slot table of `slot_numbers` (any uint64 values): a dict of arrays, one row per slot."""
    s = _u64(slot_numbers)
    h = mix64(_channel_word(cfg, channel) ^ (s * SL) ^ TAG)
    words = (h, mix64(h), mix64(mix64(h)))
    f = {}
    for name, (w, shift, how, operand) in FIELDS.items():
        v = words[w] >> U(shift)
        f[name] = (v % U(operand) if how == "mod" else v & U(operand)).astype(np.int64)
    jitter = ((h >> U(8)) % U(cfg.slot_len - FRAME)).astype(np.int64)
    d, c, t = cfg.pct_flip_data, cfg.pct_flip_crc, cfg.pct_flip_two
    kind = np.select([f["kroll"] < d, f["kroll"] < d + c, f["kroll"] < d + c + t], [1, 2, 3], 0)
    tc = np.choose(f["tc_range"], [1 + f["tc_low"], 9 + f["tc_mid"], 19 + f["tc_mid"]])
    clean = np.zeros((len(s), 14), dtype=np.uint8)
    clean[:, 0] = 0x8D
    clean[:, 1:4] = f["address"][:, None] >> np.array([0, 8, 16]) & 0xFF     # low byte first
    clean[:, 4] = tc << 3 | f["tc_sub"]
    clean[:, 5:11] = f["payload"][:, None] >> (8 * np.arange(6)) & 0xFF      # low byte first
    clean[:, 11:14] = crc24(clean)[:, None].astype(np.int64) >> np.array([16, 8, 0]) & 0xFF
    second = f["flip1"] + (f["flip1"] >= f["flip0"])                         # the 87 positions that are not flip0
    flips = np.zeros((len(s), 112), dtype=np.uint8)
    rows = np.arange(len(s))
    for k, where in ((1, f["flip0"]), (2, 88 + f["flip_crc"]), (3, f["flip0"]), (3, second)):
        flips[rows[kind == k], where[kind == k]] = 1
    sent = np.packbits(np.unpackbits(clean, axis=1) ^ flips, axis=1)
    return {"present": f["roll"] < cfg.frame_pct, "jitter": jitter, "start": s * U(cfg.slot_len) + jitter.astype(U),
            "kind": kind, "amp": AMPS[f["amp"]], "clean": clean, "sent": sent}


def slot(cfg, channel, slot_number):
    """What air_rs_amd.synth_slot returns: (present, start, clean bytes, sent bytes, kind)."""
    t = slots(cfg, channel, [slot_number])
    return bool(t["present"][0]), int(t["start"][0]), bytes(t["clean"][0]), bytes(t["sent"][0]), int(t["kind"][0])


def pulse_at(sent):
    """(n, 240) 0/1: is there a pulse at each position of the frames with these (n, 14) bytes?"""
    bits = np.unpackbits(np.asarray(sent, dtype=np.uint8), axis=1)
    on = np.zeros((len(bits), FRAME), dtype=np.uint8)
    on[:, PREAMBLE] = 1
    on[:, 16::2] = bits          # a 1: pulse in the first half of its microsecond
    on[:, 17::2] = 1 - bits      # a 0: in the second half
    return on


def noise(cfg, channel, k):
    """(n, 2) int64 noise of the samples k."""
    h = mix64(_channel_word(cfg, channel) ^ (_u64(k) * NZ))
    halves = h.astype("<u8").view(np.uint8).reshape(-1, 2, 4).sum(axis=2, dtype=np.int64) - 510
    return np.sign(halves) * (np.abs(halves) // int(cfg.noise_div))          # C division: toward zero


def pulses(cfg, channel, first, n):
    """(pulse 0/1 per sample, slot-table row per sample, the slot table) of [first, first + n)."""
    k = U(first) + np.arange(n, dtype=np.uint64)
    sl = U(cfg.slot_len)
    s0, s1 = int(U(first) // sl), int((U(first) + U(max(n, 1) - 1)) // sl)
    table = slots(cfg, channel, U(s0) + np.arange(s1 - s0 + 1, dtype=np.uint64))
    row = (k // sl - U(s0)).astype(np.int64)
    pos = (k % sl).astype(np.int64) - table["jitter"][row]
    inside = table["present"][row] & (pos >= 0) & (pos < FRAME)
    on = pulse_at(table["sent"])[row, np.clip(pos, 0, FRAME - 1)] * inside
    return on, row, table


def fill(cfg, sample_type, channel, first, n):
    """Samples [first, first + n) of channel `channel`: an (n, 2) int8 / int16 array of (I, Q)."""
    with np.errstate(over="ignore"):
        k = U(first) + np.arange(n, dtype=np.uint64)
        on, row, table = pulses(cfg, channel, first, n)
        v = noise(cfg, channel, k) + on[:, None] * table["amp"][row]
    if sample_type == I8:
        return np.clip(v, -128, 127).astype(np.int8)
    return np.clip(v * (1 << cfg.amp_shift), -32768, 32767).astype(np.int16)


# ---- the configurations both tiers run: name -> (overrides of the default config, samples) --------------------------
# Each is at least 40 slots long.  The seeds are chosen so that every case shows what it is named for
# (tests/test_synth_model.py asserts it on the model's output).
CONFIGS = {
    "default":      (dict(), 40 * 2000 + 7),
    "kinds":        (dict(seed=11), 400 * 2000),                    # the default 90/5/2/3 mix, long enough for every kind
    "slot256":      (dict(seed=12, slot_len=256), 200 * 256 + 3),   # the smallest slot: jitter is taken mod 16
    "slot100003":   (dict(seed=13, slot_len=100003), 40 * 100003 + 1),
    "pct0":         (dict(seed=14, frame_pct=0), 40 * 2000),
    "pct100":       (dict(seed=15, frame_pct=100, slot_len=300), 100 * 300),
    "pct50":        (dict(seed=16, frame_pct=50, slot_len=300), 100 * 300),
    "noise1":       (dict(seed=17, noise_div=1), 40 * 2000),        # noise up to +-510: i8 clips both ways
    "noise255":     (dict(seed=18, noise_div=255), 40 * 2000),      # the largest divisor the tests use: noise in -2 .. 2, mostly 0
    "shift0noise1": (dict(seed=19, noise_div=1, amp_shift=0), 40 * 2000),
    "shift7noise1": (dict(seed=20, noise_div=1, amp_shift=7), 40 * 2000),   # i16 clips both ways
    "mix20_10_10":  (dict(seed=21, slot_len=300, pct_flip_data=20, pct_flip_crc=10, pct_flip_two=10), 100 * 300),
    "mix100_0_0":   (dict(seed=22, slot_len=300, pct_flip_data=100, pct_flip_crc=0, pct_flip_two=0), 50 * 300),
    "mix0_100_0":   (dict(seed=23, slot_len=300, pct_flip_data=0, pct_flip_crc=100, pct_flip_two=0), 50 * 300),
    "mix0_0_100":   (dict(seed=24, slot_len=300, pct_flip_data=0, pct_flip_crc=0, pct_flip_two=100), 50 * 300),
}
DEFAULT = dict(seed=0x0AD5B0001, slot_len=2000, frame_pct=100, pct_flip_data=5, pct_flip_crc=2, pct_flip_two=3,
               noise_div=18, amp_shift=0)       # adsb_synth_default: 90 / 5 / 2 / 3, one slot per millisecond at 2 MSPS


def config(**overrides):
    return types.SimpleNamespace(**{**DEFAULT, **overrides})


@functools.lru_cache(maxsize=None)
def reference(name, sample_type):
    """The model's fill of configuration `name` (channel 0, from sample 0), computed once and read-only."""
    over, n = CONFIGS[name]
    out = fill(config(**over), sample_type, 0, 0, n)
    out.setflags(write=False)
    return out


FIRSTS = (0, 123457, 2**32 - 1000, 2**33 * 7, 2**48 + 5)    # 2^32 - 1000 with n = 2000 crosses 32 bits; 2^33 * 7: rank 7's base
CHANNELS = (0, 3, 255, 2**32 - 1)
REJECTED = (dict(slot_len=255), dict(noise_div=0), dict(amp_shift=8), dict(pct_flip_data=50, pct_flip_crc=50, pct_flip_two=1))
