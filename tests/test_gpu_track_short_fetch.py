"""What the fetch entry points of the device track table and bank do with a buffer SHORTER than what they hold
(adsb_track_{table,bank}_fetch, _fetch_last_heard, _fetch_velocity, _fetch_points), called through the C interface
directly: the Python wrappers always pass a full-size buffer, so no other test sees these rules.
  * *n is the full count whatever `max` is (fetch_points: min(n, max));
  * the first min(n, max) entries are the prefix of the full fetch, and not a byte is written past them;
  * a bank's per_receiver_counts are the records COPIED for each receiver, so they add up to min(n, max);
  * the flags are the device words, whatever `max` is, and ADSB_TRACK_TABLE_FULL survives an expire."""
import ctypes as C

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib as L
from tests.traffic import ident_frame, position_frame
from tests.velocity_traffic import velocity_frame

FULL = A.ADSB_TRACK_TABLE_FULL
SENTINEL = 0xA5
SPS = 1e-3                                   # 1000 samples a second
MAX_AIRCRAFT, MAX_FRAMES = 8, 64
SLACK = 3                                    # entries behind the full size, which no call may touch


def _frames(items):
    """[(offset, 14 frame bytes)] -> FRAME_DTYPE array."""
    out = np.zeros(len(items), dtype=A.FRAME_DTYPE)
    for k, (off, b) in enumerate(items):
        out[k]["offset"] = off
        out[k]["bytes"] = np.frombuffer(bytes(b), dtype=np.uint8)
        out[k]["fixed_bit"] = 0xFF
    return out


def _aircraft_frames(oracle, icao, at):
    """Five frames of one aircraft from sample `at`: a position pair that decodes (the reference's own pair,
    aircraft.rs:201-212), an identification, a velocity message and one more position half."""
    return [(at, position_frame(oracle, icao, False, 93000, 51372)),
            (at + 100, position_frame(oracle, icao, True, 74158, 50194)),
            (at + 200, ident_frame(oracle, icao, [1 + icao % 26] * 8)),
            (at + 300, velocity_frame(oracle, icao, 1, dew=icao & 1, vew=100 + icao % 400, dns=0, vns=7, vrsrc=1, svr=0,
                                      vr=20)),
            (at + 400, position_frame(oracle, icao, False, 93010, 51380))]


def _list(oracle, icaos, at=0):
    """One time-ordered frame list: the aircraft interleaved, a few samples apart."""
    items = [x for k, icao in enumerate(icaos) for x in _aircraft_frames(oracle, icao, at + 7 * k)]
    return _frames(sorted(items, key=lambda x: x[0]))


def _sentinel(count, dtype):
    return np.full(count * np.dtype(dtype).itemsize, SENTINEL, dtype=np.uint8).view(dtype)


def _call(fn, handle, dtype, max_n, room, *extra):
    """fn(handle, out, max_n, &n, *extra) on a sentinel buffer of `room` entries -> (buffer, n)."""
    out, n = _sentinel(room, dtype), C.c_size_t(0xDEAD)
    L.check(fn(handle, C.cast(out.ctypes.data, C.c_void_p) if fn.argtypes[1] is C.c_void_p
               else out.ctypes.data_as(fn.argtypes[1]), max_n, C.byref(n), *extra), "short fetch")
    return out, n.value


def _check_short(out, n, want_n, full, max_n):
    """*n = want_n; out = the first min(full size, max_n) entries of `full`, then nothing but the sentinel."""
    take = min(len(full), max_n)
    assert n == want_n
    assert out[:take].tobytes() == full[:take].tobytes()
    assert (out[take:].view(np.uint8) == SENTINEL).all()


TABLE_ICAOS = (0x4B1805, 0x3C6444, 0xA00001, 0x000101, 0x7FFFFF)                       # 5, not in ascending order
BANK_ICAOS = ((0x4B1805, 0x000101, 0x3C6444), (), (0xABCDEF, 0x4B1805, 0x000001, 0x800000))   # 3, 0 and 4


@pytest.mark.gpu
def test_short_fetch_keeps_count_prefix_and_untouched_tail(gpu, oracle):
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_aircraft=MAX_AIRCRAFT, max_frames=MAX_FRAMES, seconds_per_sample=SPS) as t, \
            A.TrackBank(d, 3, max_aircraft=MAX_AIRCRAFT, max_frames=MAX_FRAMES, seconds_per_sample=SPS) as b:
        lib = d._lib
        table_list = _list(oracle, TABLE_ICAOS)
        t.update(table_list, 1000)
        lists = [_list(oracle, icaos) for icaos in BANK_ICAOS]
        b.update(np.concatenate(lists), [len(x) for x in lists], [1000, 2000, 3000])
        held = [len(x) for x in BANK_ICAOS]
        total = sum(held)

        # the full fetches, through the wrappers (a full-size buffer)
        t_recs, t_flags = t.aircraft()
        b_recs, b_flags = b.aircraft()
        assert [int(x) for x in t_recs["icao"]] == sorted(TABLE_ICAOS) and t_flags == 0
        assert [[int(x) for x in r["icao"]] for r in b_recs] == [sorted(x) for x in BANK_ICAOS] and b_flags == [0, 0, 0]
        t_vel, b_vel = t.velocity(), np.concatenate(b.velocity())
        assert (t_vel["subtype"] == 1).all() and (b_vel["subtype"] == 1).all()      # a velocity message each: not empty
        full = {"t": (t_recs, t.last_heard(), t_vel, t.points()),
                "b": (np.concatenate(b_recs), np.concatenate(b.last_heard()), b_vel, b.points())}
        assert len(full["t"][3]) == len(table_list) and len(full["b"][3]) == sum(len(x) for x in lists)

        for max_n in (0, 2, 4, len(TABLE_ICAOS)):
            flags = C.c_uint32(0xDEAD)
            out, n = _call(lib.adsb_track_table_fetch, t._h, A.AIRCRAFT_DTYPE, max_n, len(TABLE_ICAOS) + SLACK,
                           C.byref(flags))
            _check_short(out, n, len(TABLE_ICAOS), full["t"][0], max_n)
            assert flags.value == t_flags
            out, n = _call(lib.adsb_track_table_fetch_last_heard, t._h, np.float64, max_n, len(TABLE_ICAOS) + SLACK)
            _check_short(out, n, len(TABLE_ICAOS), full["t"][1], max_n)
            out, n = _call(lib.adsb_track_table_fetch_velocity, t._h, A.VELOCITY_DTYPE, max_n, len(TABLE_ICAOS) + SLACK)
            _check_short(out, n, len(TABLE_ICAOS), full["t"][2], max_n)

        for max_n, want_counts in ((0, [0, 0, 0]), (2, [2, 0, 0]), (4, [3, 0, 1]), (total, held)):
            counts, flags = (C.c_uint64 * 3)(9, 9, 9), (C.c_uint32 * 3)(9, 9, 9)
            out, n = _call(lib.adsb_track_bank_fetch, b._h, A.AIRCRAFT_DTYPE, max_n, total + SLACK, counts, flags)
            _check_short(out, n, total, full["b"][0], max_n)
            assert list(counts) == want_counts and list(flags) == b_flags
            out, n = _call(lib.adsb_track_bank_fetch_last_heard, b._h, np.float64, max_n, total + SLACK)
            _check_short(out, n, total, full["b"][1], max_n)
            out, n = _call(lib.adsb_track_bank_fetch_velocity, b._h, A.VELOCITY_DTYPE, max_n, total + SLACK)
            _check_short(out, n, total, full["b"][2], max_n)

        for kind, fn, h in (("t", lib.adsb_track_table_fetch_points, t._h),
                            ("b", lib.adsb_track_bank_fetch_points, b._h)):
            pts = full[kind][3]
            for max_n in (0, 2, 4, len(pts)):
                out, n = _call(fn, h, A.TRACK_POINT_DTYPE, max_n, len(pts) + SLACK)
                _check_short(out, n, min(len(pts), max_n), pts, max_n)


@pytest.mark.gpu
def test_table_full_flag_survives_expire_and_update(gpu, oracle):
    """11 aircraft for 8 places; 5 of the 8 admitted are heard again at 5 s; an expire at 3 s evicts the other 3; the
    next update admits 2 of the 3 that were turned away."""
    icaos = sorted(0x400000 + 0x1111 * k for k in range(11))
    admitted, again, late = icaos[:MAX_AIRCRAFT], icaos[:5], icaos[9:]
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_aircraft=MAX_AIRCRAFT, max_frames=MAX_FRAMES, seconds_per_sample=SPS) as t:
        lib = d._lib

        def fetch():
            flags = C.c_uint32(0xDEAD)
            out, n = _call(lib.adsb_track_table_fetch, t._h, A.AIRCRAFT_DTYPE, MAX_AIRCRAFT, MAX_AIRCRAFT + SLACK,
                           C.byref(flags))
            assert (out[n:].view(np.uint8) == SENTINEL).all()
            return [int(x) for x in out[:n]["icao"]], flags.value

        t.update(_list(oracle, icaos), 0)
        t.update(_list(oracle, again), 5000)
        assert fetch() == (admitted, FULL)                # before the expire: 8
        t.expire(3.0)
        assert fetch() == (again, FULL)                   # after it: 5, and the flag stays
        t.update(_list(oracle, late), 6000)
        assert fetch() == (sorted(again + late), FULL)    # after the update: 7; only a reset clears the flag
        _, n = _call(lib.adsb_track_table_fetch, t._h, A.AIRCRAFT_DTYPE, 0, 1, None)
        assert n == 7
