"""Airborne-velocity messages (DF17 TC 19) for the velocity tests: a frame builder with a correct CRC, an independent
NumPy model of the decode rules in include/adsb_hip.h, and traffic that mixes velocity frames into random_traffic."""
import math

import numpy as np

from tests.traffic import random_traffic

SPEED, DIRECTION, VRATE = 0x1, 0x2, 0x4
# the 32-byte adsb_velocity layout, written out here so the model does not depend on the library
MODEL_DTYPE = np.dtype([("time", "<f8"), ("speed_kt", "<f4"), ("direction_deg", "<f4"), ("vertical_rate_fpm", "<i4"),
                        ("v_ew_kt", "<i2"), ("v_ns_kt", "<i2"), ("subtype", "u1"), ("flags", "u1"),
                        ("vrate_baro", "u1"), ("airspeed_tas", "u1"), ("reserved", "<u4")])
# ME bit fields (bit 0 = the top bit of frame byte 4): name -> (first bit, width)
FIELDS = {"tc": (0, 5), "st": (5, 3), "dew": (13, 1), "vew": (14, 10), "dns": (24, 1), "vns": (25, 10),
          "status": (13, 1), "heading": (14, 10), "as_type": (24, 1), "airspeed": (25, 10),
          "vrsrc": (35, 1), "svr": (36, 1), "vr": (37, 9)}


def empty():
    """What a record holds before its first velocity message."""
    v = np.zeros((), dtype=MODEL_DTYPE)
    v["time"] = np.nan
    return v


def velocity_frame(oracle, icao, st, tc=19, **raw):
    """A DF17 frame with TC `tc` and subtype `st` whose ME bits carry the raw fields of FIELDS (ST 1-2: dew, vew, dns,
    vns; ST 3-4: status, heading, as_type, airspeed; all: vrsrc, svr, vr), with a correct CRC."""
    me = tc << 51 | st << 48
    for name, value in raw.items():
        first, width = FIELDS[name]
        assert 0 <= value < 1 << width, (name, value)
        me |= value << (56 - first - width)
    data = bytes([0x8D, (icao >> 16) & 0xFF, (icao >> 8) & 0xFF, icao & 0xFF]) + me.to_bytes(7, "big")
    crc = oracle.get_adsb_crc(data)
    return data + bytes([(crc >> 16) & 0xFF, (crc >> 8) & 0xFF, crc & 0xFF])


def decode(frame, time):
    """The model: a MODEL_DTYPE scalar for a TC 19 frame of subtype 1-4, else None.  f64, rounded once to f32."""
    frame = bytes(frame)
    me = int.from_bytes(frame[4:11], "big")

    def f(name):
        first, width = FIELDS[name]
        return (me >> (56 - first - width)) & ((1 << width) - 1)

    st = f("st")
    if f("tc") != 19 or not 1 <= st <= 4:
        return None
    k = 4 if st in (2, 4) else 1
    v = np.zeros((), dtype=MODEL_DTYPE)
    v["time"], v["subtype"] = time, st
    flags = 0
    if st <= 2:
        if f("vew") != 0 and f("vns") != 0:
            ew = (-1 if f("dew") else 1) * (f("vew") - 1) * k
            ns = (-1 if f("dns") else 1) * (f("vns") - 1) * k
            speed = np.sqrt(np.float64(ew * ew + ns * ns))        # the integer sum is exact
            v["v_ew_kt"], v["v_ns_kt"], v["speed_kt"] = ew, ns, np.float32(speed)
            flags |= SPEED
            if speed > 0:
                d = math.atan2(ew, ns) * 180.0 / math.pi
                v["direction_deg"] = np.float32(d + 360.0 if d < 0 else d)
                flags |= DIRECTION
    else:
        if f("status") == 1:
            v["direction_deg"] = np.float32(f("heading") * 360.0 / 1024.0)
            flags |= DIRECTION
        if f("airspeed") != 0:
            v["speed_kt"] = np.float32((f("airspeed") - 1) * k)
            v["airspeed_tas"] = f("as_type")
            flags |= SPEED
    if f("vr") != 0:
        v["vertical_rate_fpm"] = (-1 if f("svr") else 1) * (f("vr") - 1) * 64
        v["vrate_baro"] = f("vrsrc")
        flags |= VRATE
    v["flags"] = flags
    return v


def last_velocity(items, icao_of=lambda fr: int.from_bytes(bytes(fr)[1:4], "big")):
    """{icao: the model's velocity of its last TC 19 ST 1-4 frame} for a time-ordered [(time_s, frame)]."""
    out = {}
    for t, fr in items:
        v = decode(fr, t)
        if v is not None:
            out[icao_of(fr)] = v
    return out


def _raw_value(rng, width):
    """0, 1, the maximum or a random value of a `width`-bit field"""
    c = int(rng.integers(0, 5))
    return (0, 1, (1 << width) - 1)[c] if c < 3 else int(rng.integers(0, 1 << width))


def random_velocity_frame(oracle, rng, icao):
    """A TC 19 frame of any subtype 0-7 (so also the ones that are no velocity message), every raw field drawn from
    zero, one, its maximum or random, both sign and source bits."""
    st = int(rng.integers(0, 8))
    raw = {"vrsrc": int(rng.integers(0, 2)), "svr": int(rng.integers(0, 2)), "vr": _raw_value(rng, 9)}
    if st in (3, 4):
        raw.update(status=int(rng.integers(0, 2)), heading=_raw_value(rng, 10), as_type=int(rng.integers(0, 2)),
                   airspeed=_raw_value(rng, 10))
    else:
        raw.update(dew=int(rng.integers(0, 2)), vew=_raw_value(rng, 10), dns=int(rng.integers(0, 2)),
                   vns=_raw_value(rng, 10))
    return velocity_frame(oracle, icao, st, **raw)


def velocity_traffic(oracle, seed, n_aircraft=40, n_frames=3000, span_s=60.0, velocity_share=1 / 3):
    """random_traffic with about `velocity_share` of the frames replaced by TC 19 frames of the same aircraft at the
    same times (random_velocity_frame), so the list stays time-ordered."""
    rng = np.random.default_rng(seed + 7919)
    out = []
    for t, fr in random_traffic(oracle, seed=seed, n_aircraft=n_aircraft, n_frames=n_frames, span_s=span_s):
        if rng.random() < velocity_share:
            fr = random_velocity_frame(oracle, rng, int.from_bytes(fr[1:4], "big"))
        out.append((t, fr))
    return out
