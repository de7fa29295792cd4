"""adsb_host_fix_of, the CPU mirror of the tracker's single-message position decode (the text the device compiles too,
air_rs_amd/csrc/adsb_fix.h), against tests/fix_model.py: random frames, encoded true positions, and known answers (CPU
tier).  Tolerances: integers, flags and the f32 surface fields exact; latitude and longitude equal as doubles (no math
library before NL, an integer); range 1e-4 NM and bearing 1e-4 degree, above f32 spacing at 256 NM and 360 degrees."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import fix_model as M


def _host(lib, site, frames, times):
    """host_fix_of over a list of frames -> (FIX_DTYPE array, flags array)."""
    out = np.zeros(len(frames), dtype=lib.FIX_DTYPE)
    flags = np.zeros(len(frames), dtype=np.uint32)
    for k, fr in enumerate(frames):
        out[k], flags[k] = lib.host_fix_of(site, fr, times[k])
    return out, flags


def _model(site, frames, times):
    out = np.zeros(len(frames), dtype=M.MODEL_DTYPE)
    flags = np.zeros(len(frames), dtype=np.uint32)
    for k, fr in enumerate(frames):
        out[k], flags[k] = M.fix_of(site, fr, times[k])
    return out, flags


def test_layouts(lib):
    assert lib.FIX_DTYPE == M.MODEL_DTYPE and lib.FRAME_FIX_DTYPE == M.FRAME_DTYPE
    assert (lib.ADSB_FIX_VALID, lib.ADSB_FIX_SURFACE, lib.ADSB_FIX_ALT, lib.ADSB_FIX_SPEED, lib.ADSB_FIX_TRACK,
            lib.ADSB_FIX_REJECTED) == (M.VALID, M.SURFACE, M.ALT, M.SPEED, M.TRACK, M.REJECTED)


def test_random_frames_equal_the_model(lib, oracle):
    """3000 random frames at each of seven sites: every type code, both CPR formats, every raw movement, track valid or
    not, a few that are not DF 17."""
    rng = np.random.default_rng(2024)
    seen_tc, kinds = set(), {"none": 0, "rejected": 0, "airborne": 0, "surface": 0}
    total = 0
    for s, site in enumerate(M.SITES):
        frames = [M.random_frame(oracle, rng, int(rng.integers(0, 1 << 24))) for _ in range(3000)]
        times = rng.uniform(0, 1e5, len(frames))
        want, want_flags = _model(site, frames, times)
        # no generated range lies within 1e-6 NM of a limit, so the two sides cannot disagree on a rejection by rounding
        for fr in frames:
            d = M.decode(site, fr)
            if d is not None and math.isfinite(d["range"]):
                assert abs(d["range"] - site[2]) > 1e-6 and abs(d["range"] - min(site[2], 45.0)) > 1e-6
            seen_tc.add(M.bits(fr)(0, 5))
        got, got_flags = _host(lib, site, frames, times)
        assert np.array_equal(got_flags, want_flags), s
        M.assert_fixes_equal(got, want, f"site {s}")
        kinds["none"] += int((want_flags == 0).sum())
        kinds["rejected"] += int(((want_flags & M.REJECTED) != 0).sum())
        kinds["airborne"] += int(((want_flags & (M.VALID | M.SURFACE)) == M.VALID).sum())
        kinds["surface"] += int(((want_flags & (M.VALID | M.SURFACE)) == (M.VALID | M.SURFACE)).sum())
        total += len(frames)
    assert total >= 20_000 and seen_tc == set(range(32))
    assert min(kinds.values()) > 500, kinds


def test_decode_finds_the_encoded_position(lib, oracle):
    """True positions within 170 NM (airborne) or 40 NM (surface) of the site, encoded by DO-260's encoder: the decode
    lies within half a quantisation step (dLat / 2^18, dLon / 2^18) plus 1e-9 degree of the truth, nothing excluded; and
    range and bearing are those of the decoded position."""
    rng = np.random.default_rng(77)
    n = 0
    for s, site in enumerate(M.SITES):
        site = (site[0], site[1], 180.0)
        for surface, reach in ((0, 170.0), (1, 40.0)):
            for _ in range(800):
                lat, lon = M.destination(site, float(rng.uniform(0, reach)), float(rng.uniform(0, 360)))
                odd = int(rng.integers(0, 2))
                tc = int(rng.integers(5, 9)) if surface else int(rng.choice([9, 14, 18, 20, 21, 22]))
                yz, xz = M.cpr_encode(lat, lon, odd, surface)
                fr = M.position_frame(oracle, 0x4B0000 + n, tc, odd, yz, xz)
                fix, flags = lib.host_fix_of(site, fr, 1.0)
                assert flags & lib.ADSB_FIX_VALID and bool(flags & lib.ADSB_FIX_SURFACE) == bool(surface), (s, n, flags)
                d_lat = (90.0 if surface else 360.0) / (60 - odd)
                d_lon = (90.0 if surface else 360.0) / max(M.num_zones(float(fix["latitude"])) - odd, 1)
                assert abs(fix["latitude"] - lat) <= d_lat / 2 ** 18 + 1e-9, (s, n, lat, lon, fix)
                off = abs((float(fix["longitude"]) - lon + 180.0) % 360.0 - 180.0)
                assert off <= d_lon / 2 ** 18 + 1e-9, (s, n, lat, lon, fix)
                rng_nm, brg = M.range_bearing(site[0], site[1], float(fix["latitude"]), float(fix["longitude"]))
                assert abs(float(fix["range_nm"]) - rng_nm) <= 1e-4
                if rng_nm >= 1.0:
                    diff = abs(float(fix["bearing_deg"]) - brg)
                    assert min(diff, 360.0 - diff) <= 1e-4
                assert bool(flags & lib.ADSB_FIX_ALT) == (9 <= tc <= 18)
                n += 1
    assert n == 7 * 2 * 800


def test_movement_and_track_known_answers(lib, oracle):
    site = (47.45, 8.56, 180.0)
    want = {0: None, 1: 0.0, 2: 0.125, 8: 0.875, 9: 1.0, 12: 1.75, 13: 2.0, 38: 14.5, 39: 15.0, 93: 69.0, 94: 70.0,
            108: 98.0, 109: 100.0, 123: 170.0, 124: 175.0, 125: None, 126: None, 127: None}
    for m, kt in want.items():
        fr = M.frame_at(oracle, 0x4B1234, site, 0.4, 200.0, 7, m & 1, movement=m, track_valid=0, track=77)
        fix, flags = lib.host_fix_of(site, fr, 2.5)
        assert flags & lib.ADSB_FIX_VALID and flags & lib.ADSB_FIX_SURFACE and not flags & lib.ADSB_FIX_TRACK
        assert bool(flags & lib.ADSB_FIX_SPEED) == (kt is not None), m
        assert fix["ground_speed_kt"] == (0.0 if kt is None else kt) and fix["track_deg"] == 0.0, m
        assert (fix["time"], fix["n_fixes"], fix["n_rejected"], fix["type_code"], fix["cpr_odd"]) == (2.5, 1, 0, 7, m & 1)
        assert fix["flags"] == flags and fix["altitude"] == 0 and abs(float(fix["range_nm"]) - 0.4) < 0.01
    for track, deg in ((0, 0.0), (127, 357.1875), (64, 180.0)):
        fr = M.frame_at(oracle, 0x4B1234, site, 0.4, 200.0, 5, 1, movement=0, track_valid=1, track=track)
        fix, flags = lib.host_fix_of(site, fr, 0.0)
        assert flags == lib.ADSB_FIX_VALID | lib.ADSB_FIX_SURFACE | lib.ADSB_FIX_TRACK and fix["track_deg"] == deg


def test_range_limits_known_answers(lib, oracle):
    site = (40.0, -100.0, 180.0)
    # 181 NM east of the site (inside half a longitude zone there, 183.8 NM): decoded where it is, and turned away
    far = M.frame_at(oracle, 0x4B0001, site, 181.0, 90.0, 11, 0)
    d = M.decode(site, far)
    assert d["flags"] == M.REJECTED and abs(d["range"] - 181.0) < 0.01
    fix, flags = lib.host_fix_of(site, far, 3.0)
    assert flags == lib.ADSB_FIX_REJECTED and fix["n_rejected"] == 1 and fix["n_fixes"] == 0
    assert math.isnan(fix["time"]) and fix["flags"] == 0 and fix["latitude"] == 0.0 and fix["range_nm"] == 0.0
    near = M.frame_at(oracle, 0x4B0001, site, 179.0, 90.0, 11, 0, alt_code=0xC38)
    fix, flags = lib.host_fix_of(site, near, 3.0)
    assert flags == lib.ADSB_FIX_VALID | lib.ADSB_FIX_ALT and abs(float(fix["range_nm"]) - 179.0) < 0.01
    assert abs(float(fix["bearing_deg"]) - 90.0) < 0.01 and fix["altitude"] == 38000
    assert lib.host_fix_of((40.0, -100.0, 178.0), near, 3.0)[1] == lib.ADSB_FIX_REJECTED       # the site's own limit
    # 46 NM east (odd format: half a surface zone is 47 NM there): a surface message is turned away at 45 NM whatever the
    # site allows, an airborne one from the same place is not
    lat, lon = M.destination(site, 46.0, 90.0)
    ground = M.position_frame(oracle, 0x4B0002, 6, 1, *M.cpr_encode(lat, lon, 1, 1), movement=20)
    air = M.position_frame(oracle, 0x4B0002, 12, 1, *M.cpr_encode(lat, lon, 1, 0))
    assert abs(M.decode(site, ground)["range"] - 46.0) < 0.01
    fix, flags = lib.host_fix_of(site, ground, 3.0)
    assert flags == lib.ADSB_FIX_REJECTED | lib.ADSB_FIX_SURFACE and fix["n_rejected"] == 1
    fix, flags = lib.host_fix_of(site, air, 3.0)
    assert flags == lib.ADSB_FIX_VALID | lib.ADSB_FIX_ALT and abs(float(fix["range_nm"]) - 46.0) < 0.01
    assert abs(fix["latitude"] - lat) < 1e-4 and abs(fix["longitude"] - lon) < 1e-4
    closer = M.frame_at(oracle, 0x4B0002, site, 44.0, 90.0, 6, 1, movement=20)
    assert lib.host_fix_of(site, closer, 3.0)[1] == lib.ADSB_FIX_VALID | lib.ADSB_FIX_SURFACE | lib.ADSB_FIX_SPEED
    assert lib.host_fix_of((40.0, -100.0, 30.0), closer, 3.0)[1] == lib.ADSB_FIX_REJECTED | lib.ADSB_FIX_SURFACE
    # a widely published pair of messages of one aircraft at 38000 ft, each decoded on its own: the even one is where the
    # pair decodes to (52.2572 N, 3.9194 E), the odd one, sent at another moment, a mile further on
    for text, odd, lat, lon in (("8D40621D58C382D690C8AC2863A7", 0, 52.2572, 3.9194),
                                ("8D40621D58C386435CC412692AD6", 1, 52.2658, 3.9389)):
        fix, flags = lib.host_fix_of((52.0, 4.0), bytes.fromhex(text), 0.0)
        assert flags == lib.ADSB_FIX_VALID | lib.ADSB_FIX_ALT and fix["altitude"] == 38000 and fix["cpr_odd"] == odd
        assert abs(fix["latitude"] - lat) < 1e-4 and abs(fix["longitude"] - lon) < 1e-4


def test_host_fix_of_arguments(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    b = (C.c_uint8 * 14)()
    out, site = _lib.AdsbFix(), _lib.AdsbSite(10.0, 20.0, 180.0)
    assert L.adsb_host_fix_of(None, C.byref(b), 0.0, C.byref(out), None) == lib.ADSB_E_ARG
    assert L.adsb_host_fix_of(C.byref(site), None, 0.0, C.byref(out), None) == lib.ADSB_E_ARG
    assert L.adsb_host_fix_of(C.byref(site), C.byref(b), 0.0, None, None) == lib.ADSB_E_ARG
    assert L.adsb_host_fix_of(C.byref(site), C.byref(b), 0.0, C.byref(out), None) == lib.ADSB_OK
    assert math.isnan(out.time) and bytes(out)[8:] == bytes(56)            # no position message: the empty fix
    for bad in ((91.0, 0.0, 10.0), (0.0, 181.0, 10.0), (0.0, 0.0, 0.0), (0.0, 0.0, 180.5), (math.nan, 0.0, 10.0)):
        with pytest.raises(lib.AdsbError) as e:
            lib.host_fix_of(bad, bytes(14))
        assert e.value.code == lib.ADSB_E_ARG
