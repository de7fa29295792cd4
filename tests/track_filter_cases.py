"""Case builders for the filter behind a table's multilaterated fixes: lists of (aircraft address, sample offset, fix)
that the tests make themselves, since the filter does not care where a fix came from.  Every frame is an identification
message of its aircraft (the filter reads no frame byte).  A case is a dict: icaos, offsets, fixes (model's FIX_DTYPE),
cfg (keyword arguments of the reserve), planted (a fix displaced on purpose: must be an OUTLIER), honest (must not be),
and optionally flags (what every frame's adsb_frame_filter.flags must be, written out by hand).  No device, no library."""
import math

import numpy as np

from tests import track_filter_model as M
from tests import track_mlat_model as MM

SPS = 0.5e-6
TICKS = 2_000_000                    # samples per second
BASE = 1_000_000
FRAME_DTYPE = np.dtype([("offset", "<u8"), ("bytes", "u1", (14,)), ("status", "u1"), ("fixed_bit", "u1")])
OK = M.FIX_ATTEMPTED | M.FIX_CONVERGED | M.FIX_VALID
FAR = (15.0, 20.0)                   # degrees added to a planted fix: 1 600 km and more, whatever the covariance


def times(case, base=BASE):
    """The store's frame times: (sample_base + offset) x seconds_per_sample, one rounded product."""
    return np.array([float(base + int(o)) * SPS for o in case["offsets"]])


def frames(case):
    return MM.frames_array([(int(o), MM.raw_frame(int(i), 4 << 51)) for i, o in zip(case["icaos"], case["offsets"])],
                           FRAME_DTYPE)


def _case(rows, cfg=None, flags=None, order=None):
    """rows: (seconds, icao, fix, planted, honest), sorted here (stable) by time, or by order[k] where a list is to hold
    a frame out of its place."""
    keys = [r[0] for r in rows] if order is None else order
    rows = [rows[k] for k in sorted(range(len(rows)), key=lambda k: keys[k])]
    out = dict(icaos=np.array([r[1] for r in rows], dtype=np.uint32),
               offsets=np.array([int(round(r[0] * TICKS)) for r in rows], dtype=np.uint64),
               fixes=np.array([r[2] for r in rows], dtype=M.FIX_DTYPE) if rows else np.zeros(0, dtype=M.FIX_DTYPE),
               planted=np.array([r[3] for r in rows], dtype=bool), honest=np.array([r[4] for r in rows], dtype=bool),
               cfg=dict(cfg or {}))
    if flags is not None:
        out["flags"] = flags
    return out


def cut(case, lo, hi):
    out = {k: (v[lo:hi] if isinstance(v, np.ndarray) else v) for k, v in case.items() if k != "flags"}
    return out


class Flyer:
    """A point moving at constant speed, heading and climb over a flat map of its start latitude."""

    def __init__(self, lat, lon, h=10000.0, speed=230.0, heading=60.0, climb=0.0):
        self.lat, self.lon, self.h, self.speed, self.heading, self.climb = lat, lon, h, speed, heading, climb

    def advance(self, dt):
        vn, ve = self.speed * math.cos(math.radians(self.heading)), self.speed * math.sin(math.radians(self.heading))
        self.lat += vn * dt / 111_000.0
        self.lon += ve * dt / (111_000.0 * math.cos(math.radians(self.lat)))
        self.lon = (self.lon + 180.0) % 360.0 - 180.0
        self.h += self.climb * dt

    def place(self, north_m=0.0, east_m=0.0, up_m=0.0):
        lon = self.lon + east_m / (111_000.0 * math.cos(math.radians(self.lat)))
        return self.lat + north_m / 111_000.0, (lon + 180.0) % 360.0 - 180.0, self.h + up_m


def _honest_fix(rng, fly, hdop=None, vdop=None, residual=None, altitude=None, noise=0.3):
    """A fix within noise x (hdop x sr) of the flyer (uniform in a disc), noise x the vertical sigma above or below."""
    hdop = float(np.float32(rng.uniform(0.8, 3.0))) if hdop is None else hdop
    vdop = float(np.float32(rng.uniform(1.0, 4.0))) if vdop is None else vdop
    residual = float(rng.choice([3.0, 60.0])) if residual is None else residual
    altitude = bool(rng.random() < 0.5) if altitude is None else altitude
    sr = max(30.0, residual)
    r, th = noise * hdop * sr * math.sqrt(rng.random()), rng.uniform(0.0, 2.0 * math.pi)
    sv = 15.0 if altitude else vdop * sr
    lat, lon, h = fly.place(r * math.cos(th), r * math.sin(th), noise * sv * rng.uniform(-1.0, 1.0))
    return M.fix(lat, lon, h, OK | (M.FIX_ALTITUDE if altitude else 0), residual, hdop, vdop)


def traffic(seed, n_frames, icaos, t0=5.0):
    """n_frames frames of the given aircraft around (47, 8), each flying straight: honest fixes with a little noise,
    single planted outliers, fixes that are not valid, not attempted, NaN, beyond max_hdop, without a usable height, and
    gaps longer than reset_gap_s.  Aircraft get unequal shares of the list."""
    rng = np.random.default_rng(seed)
    share = rng.dirichlet(np.full(len(icaos), 0.7)) if len(icaos) > 1 else np.array([1.0])
    counts = np.maximum(1, np.floor(share * n_frames).astype(int))
    while counts.sum() > n_frames:
        counts[np.argmax(counts)] -= 1
    counts[np.argmax(counts)] += n_frames - counts.sum()
    rows = []
    for icao, n in zip(icaos, counts):
        fly = Flyer(47.0 + rng.uniform(-1, 1), 8.0 + rng.uniform(-1, 1), rng.uniform(1000, 12000), rng.uniform(120, 260),
                    rng.uniform(0, 360), rng.uniform(-10, 10))
        t, last_planted = t0 + rng.uniform(0, 20), True
        for _ in range(int(n)):
            dt = rng.uniform(0.5, 2.0)
            u = rng.random()
            if u < 0.03:
                dt += rng.uniform(31.0, 40.0)
            t += dt
            fly.advance(dt)
            planted, honest = False, False
            if u < 0.03 or u >= 0.20 or last_planted:
                fx, honest = _honest_fix(rng, fly), True
            elif u < 0.07:
                fx, planted = _honest_fix(rng, fly), True
                fx["latitude"] += FAR[0]
                fx["longitude"] += FAR[1]
            elif u < 0.11:
                fx = M.fix(1.0, 2.0, flags=M.FIX_ATTEMPTED | 0x20)
            elif u < 0.13:
                fx = M.fix(0.0, 0.0, flags=0)
            elif u < 0.15:
                fx = _honest_fix(rng, fly)
                fx[["latitude", "longitude", "height_m"][int(rng.integers(3))]] = math.nan
            elif u < 0.17:
                fx = _honest_fix(rng, fly, hdop=25.0)
            else:
                fx, honest = _honest_fix(rng, fly, vdop=80.0, altitude=False), True
            last_planted = planted
            rows.append((t, int(icao), fx, planted, honest))
    return _case(rows)


def one_aircraft(seed, n, icao=0x4CA001):
    return traffic(seed, n, [icao])


def straddle():
    """Aircraft `low` fills sorted positions 0-249, `t` 250-261: t's segment begins in one 256-thread block (and one
    64-thread one) and ends in the next."""
    low, t = 0x400001, 0x400002
    rng = np.random.default_rng(31)
    t_frames = set(range(7, 240, 20))
    a, b = Flyer(47.0, 8.0, heading=10.0), Flyer(46.0, 9.0, heading=200.0, climb=5.0)
    rows = []
    for k in range(262):
        for f in (a, b):
            f.advance(1.0)
        rows.append((10.0 + k, t if k in t_frames else low, _honest_fix(rng, b if k in t_frames else a), False, True))
    return _case(rows)


def no_usable(n=300):
    rng = np.random.default_rng(33)
    rows = [(5.0 + k, 0x480000 + int(rng.integers(7)), M.fix(47.0, 8.0, flags=M.FIX_ATTEMPTED | 0x20), False, False)
            for k in range(n)]
    return _case(rows)


def rules():
    """Every rule of the header on aircraft of their own, one list; `flags` spells out what each frame must get."""
    U, AP, IN, RS, OU, SK = M.USABLE, M.APPLIED, M.INIT, M.RESET, M.OUTLIER, M.SKIPPED
    rng = np.random.default_rng(35)
    rows, order, want = [], [], {}

    def add(icao, t, fx, flags, planted=False, place=None):
        rows.append((t, icao, fx, planted, bool(flags & AP)))
        order.append(t if place is None else place)
        want.setdefault(icao, []).append(flags)

    still = Flyer(47.0, 8.0, speed=0.0)

    def here(altitude=None, **fields):
        fx = _honest_fix(rng, still, noise=0.1, altitude=altitude)
        for name, value in fields.items():
            fx[name] = value
        return fx

    # dt = 0, and a negative dt between applied frames: the frame of second 11 lies behind the one of second 12
    for t, flags, place in ((10.0, U | IN, None), (10.0, U | AP, None), (12.0, U | AP, None), (11.0, U | SK, 12.5),
                            (13.0, U | AP, None)):
        add(0x4D0001, t, here(), flags, place=place)
    # dt just below and just above reset_gap_s (30 s): one sample is 0.5 us, far above what the times' rounding moves
    t = 100.0
    add(0x4D0002, t, here(), U | IN)
    for gap, flags in ((30.0 - 1 / TICKS, U | AP), (30.0 + 1 / TICKS, U | RS | IN), (1.0, U | AP)):
        t += gap
        add(0x4D0002, t, here(), flags)
    # max_outliers (3) reached: the aircraft really is elsewhere
    there = Flyer(47.0 + FAR[0], 8.0 + FAR[1], speed=0.0)
    for k in range(4):
        add(0x4D0003, 200.0 + k, here(), U | (AP if k else IN))
    for k, flags in enumerate((U | OU, U | OU, U | OU | RS | IN, U | AP, U | AP)):
        add(0x4D0003, 204.0 + k, _honest_fix(rng, there, noise=0.1), flags, planted=k < 3)
    # longitude across +-180, eastbound at latitude 10
    east = Flyer(10.0, 179.99, speed=250.0, heading=90.0)
    for k in range(12):
        add(0x4D0004, 300.0 + k, _honest_fix(rng, east, noise=0.1), U | (AP if k else IN))
        east.advance(1.0)
    assert east.lon < -179.9
    # latitude 88.9 is usable, 89.1 is not
    for icao, lat, flags in ((0x4D0005, 88.9, (U | IN, U | AP)), (0x4D0006, 89.1, (0, 0)), (0x4D0007, -89.1, (0, 0))):
        pole = Flyer(lat, 8.0, speed=0.0)
        for k in range(2):
            add(icao, 400.0 + k, _honest_fix(rng, pole, noise=0.1), flags[k])
    # hdop at max_hdop (20) and above it
    for k, (hdop, flags) in enumerate(((1.0, U | IN), (20.0, U | AP), (20.5, 0), (float("inf"), 0), (0.0, 0), (-1.0, 0),
                                       (2.0, U | AP))):
        add(0x4D0008, 500.0 + k, here(hdop=hdop), flags)
    # vdop above max_vdop (50) with and without ALTITUDE: with it the height is measured all the same
    for k, (vdop, alt) in enumerate(((2.0, False), (60.0, True), (60.0, False), (0.0, False), (2.0, False))):
        add(0x4D0009, 600.0 + k, here(vdop=vdop, altitude=alt), U | (AP if k else IN))
    add(0x4D000A, 600.0, here(vdop=60.0, altitude=False), U | IN)       # a start without a height
    add(0x4D000A, 601.0, here(vdop=60.0, altitude=False), U | AP)
    add(0x4D000A, 602.0, here(vdop=2.0, altitude=False), U | AP)
    # NaN fields in a VALID fix
    add(0x4D000B, 700.0, here(), U | IN)
    for k, name in enumerate(("latitude", "longitude", "height_m", "hdop")):
        add(0x4D000B, 701.0 + k, here(**{name: math.nan}), 0)
    for k, (name, value, flags) in enumerate((("vdop", math.nan, U | AP), ("residual_rms_m", math.nan, U | AP),
                                              ("residual_rms_m", math.inf, 0), ("height_m", 100001.0, 0),
                                              ("height_m", -1001.0, 0))):
        add(0x4D000B, 705.0 + k, here(altitude=False, **{name: value}), flags)
    add(0x4D000B, 711.0, here(), U | AP)
    # usable frames only at a segment's head, or only at its tail
    bad = M.fix(1.0, 2.0, flags=M.FIX_ATTEMPTED | 0x20)
    for k in range(6):
        add(0x4D000C, 800.0 + k, here() if k == 0 else bad, (U | IN) if k == 0 else 0)
        add(0x4D000D, 800.0 + k, here() if k == 5 else bad, (U | IN) if k == 5 else 0)
    case = _case(rows, order=order)
    seen = {icao: 0 for icao in want}
    flags = []
    for icao in case["icaos"]:                                              # the sort is stable: per aircraft, as added
        flags.append(want[int(icao)][seen[int(icao)]])
        seen[int(icao)] += 1
    case["flags"] = np.array(flags, dtype=np.uint32)
    return case


def flight(seed, icao=0x4CA5E5):
    """The usefulness check's flight: 230 m/s, a straight leg, a 3 degrees/s turn through 90 degrees, a straight leg;
    fixes every 0.5..2 s with Gaussian noise of hdop x 50 m per horizontal axis (residual_rms_m says 50), and 5 % of the
    fixes displaced by 20 km.  The turn is 12 m/s^2 across the track, so the case sets accel_h = 12: with the default of
    3 m/s^2 the filter takes the turn itself for a run of outliers and restarts behind it, which is what max_outliers is
    for.  -> (case, truth [n, 3] = latitude, longitude, height of the aircraft at each fix,
    straight [n] = the fix lies on a straight leg)."""
    rng = np.random.default_rng(seed)
    fly = Flyer(47.0, 8.0, speed=230.0, heading=40.0)
    rows, truth, straight = [], [], []
    t, phase_end = 10.0, (150.0, 180.0, 330.0)
    while t < phase_end[2]:
        dt = rng.uniform(0.5, 2.0)
        for _ in range(20):                                                 # the turn in small steps
            fly.advance(dt / 20.0)
            t += dt / 20.0
            if phase_end[0] <= t < phase_end[1]:
                fly.heading += 3.0 * dt / 20.0
        hdop = float(np.float32(rng.uniform(0.8, 2.0)))
        displaced = bool(rng.random() < 0.05)
        north, east = rng.normal(0.0, hdop * 50.0, size=2)
        if displaced:
            th = rng.uniform(0.0, 2.0 * math.pi)
            north, east = north + 20_000.0 * math.cos(th), east + 20_000.0 * math.sin(th)
        lat, lon, h = fly.place(north, east, rng.normal(0.0, 15.0))
        rows.append((t, icao, M.fix(lat, lon, h, OK | M.FIX_ALTITUDE, 50.0, hdop, 2.0), displaced, not displaced))
        truth.append((fly.lat, fly.lon, fly.h))
        straight.append(not (phase_end[0] - 5.0 <= t < phase_end[1] + 30.0))
    return _case(rows, cfg=dict(accel_h=12.0)), np.array(truth), np.array(straight)


MODE_S = 0x3C4A5B


def flying_network(n=30, speed=220.0, heading=60.0):
    """Five receivers' Beast streams of ONE aircraft that sends no ADS-B: an all-call reply, then a DF4 reply a second,
    from a point moving at `speed` m/s on `heading` at 6 000 m, 12 MHz ticks.  -> dict(rcv, streams, truth [n, 2]) for
    tests/track_modes_cases.recordings."""
    from tests import mlat_cases as MK
    from tests import modes_model as MD
    from tests import wire_in_short_model as S
    rcv = MK.receivers(5, seed=946)
    fly = Flyer(MK.LAT0 - 0.15, MK.LON0 - 0.3, h=6000.0, speed=speed, heading=heading)
    pos, truth, msgs = [], [], []
    for i in range(n):
        pos.append(MK.M.ecef_of(fly.lat, fly.lon, fly.h))
        truth.append((fly.lat, fly.lon))
        msgs.append(MD.all_call(MODE_S) if i == 0 else
                    MD.reply(4, MODE_S, b1=i, field=MD.field_of(Q=1) | (0x0A80 + 0x80 * (i % 4))))
        fly.advance(1.0)
    lst = MK.build(rcv, np.array(pos), [m.ljust(14, b"\0") for m in msgs], spt=1 / 12e6, spacing_s=1.0)
    streams, at = [], 0
    for r in range(5):
        mine = lst["frames"][at:at + int(lst["counts"][r])]
        at += len(mine)
        streams.append(b"".join(S.beast_frame(b"2", int(f["offset"]), 40 + r, f["bytes"].tobytes()[:7]) for f in mine))
    return dict(rcv=rcv, streams=streams, truth=np.array(truth), speed=speed, heading=heading)
