"""The persistent aircraft table on the device (adsb_track_table_*, air_rs_amd.TrackTable): the reference keeps ONE
HashMap<u32, Aircraft> for the life of its display thread (src/adsb/tui.rs:22-42, web.rs:115) and pairs an even and
an odd position message up to 10 s apart (aircraft.rs:62-95), so with its 20 000-sample buffers most pairs cross
buffers.  Checked against the oracle's sequential restatement of aircraft.rs fed the same frames at the same times."""
import math

import numpy as np
import pytest

import air_rs_amd as A
from tests.traffic import position_frame, random_traffic

REF_EVEN, REF_ODD = "8D40621D58C386435CC412692AD6", "8D40621D58C382D690C8AC2863A7"  # aircraft.rs:201-212
REF_LAT, REF_LON = 52.2572021484375, 3.91937255859375  # the code's longitude, not the reference test's 3.8295


def _frames(items):
    """[(offset, 14 frame bytes)] -> FRAME_DTYPE array."""
    out = np.zeros(len(items), dtype=A.FRAME_DTYPE)
    for k, (off, b) in enumerate(items):
        out[k]["offset"] = off
        out[k]["bytes"] = np.frombuffer(bytes(b), dtype=np.uint8)
        out[k]["fixed_bit"] = 0xFF
    return out


def _icao(fr):
    b = fr["bytes"]
    return (int(b[1]) << 16) | (int(b[2]) << 8) | int(b[3])


def _odd(fr):
    return (int(fr["bytes"][6]) >> 2) & 1


def _same_table(recs, want, counts):
    assert [int(r["icao"]) for r in recs] == [s.icao for s in want]
    for rec, s in zip(recs, want):
        assert rec["n_frames"] == counts[s.icao]
        assert rec["callsign"].decode() == s.callsign.decode() and rec["altitude"] == s.altitude
        assert bool(rec["has_position"]) == bool(s.has_position)
        if s.has_position:
            assert (rec["latitude"], rec["longitude"]) == pytest.approx((s.latitude, s.longitude), abs=1e-9)
        assert (math.isnan(rec["last_contact"]) and math.isnan(s.last_contact)) or \
            rec["last_contact"] == pytest.approx(s.last_contact, abs=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [21, 22])
def test_streaming_table_equals_oracle(gpu, oracle, seed):
    """Modulated traffic through the per-buffer feed in 20 000-sample buffers, one table update per popped buffer:
    every point and, every few buffers, the whole table equal the oracle's; most pairs cross buffers."""
    from tests.golden.make_golden import modulate, place
    traffic = random_traffic(oracle, seed=seed, n_aircraft=35, n_frames=3000)
    chunk, gap = 20_000, 400
    sps = 1.0 / chunk                              # a buffer spans 1 s: the 10 s window covers 10 buffers
    n = 300 + gap * len(traffic) + 600
    items = [(300 + gap * k, modulate(fr, (80, 30), None)) for k, (_, fr) in enumerate(traffic)]
    iq = place(n, items, np.int8, floor=3, seed=seed)
    ot = oracle.tracker()
    counts, last_pos_buf = {}, {}                  # per ICAO: frames so far; buffer of the last even / odd message
    n_new = n_cross = n_buf = 0
    with A.AdsbDemod(max_samples=chunk, max_out=1 << 12) as d, \
            A.TrackTable(d, max_frames=1 << 12, seconds_per_sample=sps) as table, \
            A.Feed(d, max_chunk=chunk, carry=False) as f:

        def consume():
            nonlocal n_new, n_cross, n_buf
            frames, flags, first = f.pop()
            assert flags == 0
            table.update(frames, first)
            pts = table.points()
            assert len(pts) == len(frames)
            for k, fr in enumerate(frames):
                new, s = ot.update(bytes(fr["bytes"]), float(first + int(fr["offset"])) * sps)
                icao = _icao(fr)
                counts[icao] = counts.get(icao, 0) + 1
                assert bool(pts[k]["flags"] & A.ADSB_TRACK_NEW_POSITION) == new, (n_buf, k)
                assert pts[k]["icao"] == s.icao == icao and not pts[k]["flags"] & A.ADSB_TRACK_UNTRACKED
                if new:
                    n_new += 1
                    assert (pts[k]["latitude"], pts[k]["longitude"]) == pytest.approx((s.latitude, s.longitude),
                                                                                      abs=1e-9)
                    n_cross += last_pos_buf[(icao, 1 - _odd(fr))] < n_buf
                if 9 <= int(fr["bytes"][4]) >> 3 <= 18:   # a position message (msgs.rs:122-124)
                    last_pos_buf[(icao, _odd(fr))] = n_buf
            if n_buf % 5 == 0 or f.in_flight == 0:
                recs, tflags = table.aircraft()
                assert tflags == 0
                _same_table(recs, sorted(ot.aircraft(), key=lambda s: s.icao), counts)
            n_buf += 1

        for a in range(0, n, chunk):
            b = min(a + chunk, n)
            if b - a < A.WINDOW:
                break
            f.push(iq[a:b])
            if f.in_flight == 2:
                consume()
        while f.in_flight:
            consume()
        recs, _ = table.aircraft()
        _same_table(recs, sorted(ot.aircraft(), key=lambda s: s.icao), counts)
    assert n_buf >= 50 and len(recs) >= 30
    assert n_new > 300 and n_cross >= 100, (n_new, n_cross)


def _pair_run(d, oracle, gap_samples, split):
    """The reference's even/odd pair as host frames, the odd one gap_samples later: one update or two."""
    sps = 2.0 ** -20
    even, odd = bytes.fromhex(REF_EVEN), bytes.fromhex(REF_ODD)
    ot = oracle.tracker()
    ot.update(even, 0.0)
    new, s = ot.update(odd, gap_samples * sps)
    with A.TrackTable(d, max_frames=16, seconds_per_sample=sps) as t:
        if split:
            t.update(_frames([(0, even)]))
            assert int(t.points()[0]["flags"]) == 0
            t.update(_frames([(0, odd)]), sample_base=gap_samples)
            pt = t.points()[0]
        else:
            t.update(_frames([(0, even), (gap_samples, odd)]))
            pt = t.points()[1]
        recs, flags = t.aircraft()
    assert flags == 0 and len(recs) == 1 and recs[0]["icao"] == 0x40621D and recs[0]["n_frames"] == 2
    assert bool(pt["flags"] & A.ADSB_TRACK_NEW_POSITION) == new
    assert bool(recs[0]["has_position"]) == bool(s.has_position) and recs[0]["altitude"] == 38000
    assert recs[0]["last_contact"] == gap_samples * sps
    return pt, s


@pytest.mark.gpu
def test_reference_pair_split_across_updates(gpu, oracle):
    with A.AdsbDemod(max_samples=4096, max_out=64) as d:
        for split in (False, True):
            pt, s = _pair_run(d, oracle, 1 << 20, split)                   # 1 s apart
            assert pt["flags"] == A.ADSB_TRACK_NEW_POSITION
            assert abs(pt["latitude"] - REF_LAT) < 1e-9 and abs(pt["longitude"] - REF_LON) < 1e-9
            assert (pt["latitude"], pt["longitude"]) == pytest.approx((s.latitude, s.longitude), abs=1e-9)
            pt, _ = _pair_run(d, oracle, 10 * (1 << 20) + (1 << 19), split)  # 10.5 s: too old (aircraft.rs:68-70)
            assert pt["flags"] == 0
            pt, _ = _pair_run(d, oracle, 10 * (1 << 20), split)             # exactly 10 s: the test is `> 10`
            assert pt["flags"] == A.ADSB_TRACK_NEW_POSITION and abs(pt["longitude"] - REF_LON) < 1e-9


@pytest.mark.gpu
def test_per_launch_tracker_loses_the_split_pair(gpu):
    """The gap the table closes: adsb_track_device starts from an empty map on every launch."""
    from tests.golden.make_golden import modulate, place
    for h in (REF_EVEN, REF_ODD):
        iq = place(1000, [(300, modulate(bytes.fromhex(h), (90, 20), None))], np.int8)
        with A.AdsbDemod(max_samples=len(iq), max_out=64) as d:
            frames, _ = d.demod(iq)
            points, _ = d.track(0.5e-6)
        assert len(frames) == 1 and int(points[0]["flags"]) == 0


@pytest.mark.gpu
def test_any_cut_gives_the_same_result(gpu, oracle):
    """One update from the device list equals adsb_track_device bit for bit; any cut into host chunks equals it too."""
    from tests.golden.make_golden import modulate, place
    traffic = random_traffic(oracle, seed=31, n_aircraft=25, n_frames=2500, span_s=80.0)
    gap = 400
    n = 300 + gap * len(traffic) + 600
    sps = 80.0 / (gap * len(traffic))
    items = [(300 + gap * k, modulate(fr, (80, 30), None)) for k, (_, fr) in enumerate(traffic)]
    iq = place(n, items, np.int8, floor=3, seed=31)
    with A.AdsbDemod(max_samples=n, max_out=1 << 13) as d:
        frames, flags = d.demod(iq)
        assert flags == 0 and len(frames) >= len(traffic)
        want_pts, want_acs = d.track(sps)
        n_out, _, _ = d.fetch_counts()
        frames_dev, _ = d.result_device()
        with A.TrackTable(d, max_frames=1 << 13, seconds_per_sample=sps) as t:
            t.update_device(frames_dev, n_out)
            pts = t.points()
            acs, tflags = t.aircraft()
            assert tflags == 0
            assert pts.tobytes() == want_pts.tobytes()
            assert acs.tobytes() == want_acs.tobytes()
            assert int((pts["flags"] & A.ADSB_TRACK_NEW_POSITION != 0).sum()) > 400
            rng = np.random.default_rng(7)
            for rep in range(3):
                t.reset()
                sizes = [1] * 64 + list(rng.integers(1, 201, size=len(frames)))  # single frames: every pair is cut
                parts, a = [], 0
                for sz in sizes:
                    if a >= len(frames):
                        break
                    t.update(frames[a:a + sz])
                    parts.append(t.points())
                    a += sz
                assert np.concatenate(parts).tobytes() == want_pts.tobytes()
                acs, tflags = t.aircraft()
                assert tflags == 0 and acs.tobytes() == want_acs.tobytes()


def _even_odd(oracle, icao, odd):
    # the CPR halves of the reference pair, under another ICAO: every such pair decodes
    return position_frame(oracle, icao, odd, 74158 if odd else 93000, 50194 if odd else 51372)


@pytest.mark.gpu
def test_reset_empties_the_table(gpu, oracle):
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, A.TrackTable(d, max_frames=16) as t:
        with pytest.raises(A.AdsbError) as e:
            t.points()
        assert e.value.code == A.ADSB_E_STATE
        t.update(_frames([(0, _even_odd(oracle, 0x123456, False))]))
        recs, flags = t.aircraft()
        assert len(recs) == 1 and flags == 0
        t.reset()
        recs, flags = t.aircraft()
        assert len(recs) == 0 and flags == 0
        t.update(_frames([(1000, _even_odd(oracle, 0x123456, True))]))  # its even half is gone with the reset
        assert int(t.points()[0]["flags"]) == 0
        recs, _ = t.aircraft()
        assert len(recs) == 1 and recs[0]["n_frames"] == 1 and not recs[0]["has_position"]
        t.update(_frames([(2000, _even_odd(oracle, 0x123456, False))]))  # a new even pairs with the odd after reset
        assert int(t.points()[0]["flags"]) == A.ADSB_TRACK_NEW_POSITION


@pytest.mark.gpu
def test_full_table_admits_the_lowest_icaos(gpu, oracle):
    rng = np.random.default_rng(3)
    icaos = [int(x) for x in rng.choice(np.arange(0x100000, 0xF00000), size=12, replace=False)]
    order = list(rng.permutation(12))                       # list order unrelated to ICAO order
    admitted = set(sorted(icaos)[:8])
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_aircraft=8, max_frames=64, seconds_per_sample=1e-3) as t:
        t.update(_frames([(10 * k, _even_odd(oracle, icaos[j], False)) for k, j in enumerate(order)]))
        pts = t.points()
        for k, j in enumerate(order):
            assert pts[k]["icao"] == icaos[j]
            if icaos[j] in admitted:
                assert pts[k]["flags"] == 0
            else:
                assert pts[k]["flags"] == A.ADSB_TRACK_UNTRACKED and pts[k]["latitude"] == pts[k]["longitude"] == 0.0
        recs, flags = t.aircraft()
        assert flags == A.ADSB_TRACK_TABLE_FULL
        assert [int(r["icao"]) for r in recs] == sorted(admitted) and all(r["n_frames"] == 1 for r in recs)
        # one second later: the odd halves; admitted aircraft pair across the two updates, the others stay out
        t.update(_frames([(1000 + 10 * k, _even_odd(oracle, icaos[j], True)) for k, j in enumerate(order)]))
        pts = t.points()
        for k, j in enumerate(order):
            want = A.ADSB_TRACK_NEW_POSITION if icaos[j] in admitted else A.ADSB_TRACK_UNTRACKED
            assert pts[k]["flags"] == want
        recs, flags = t.aircraft()
        assert flags == A.ADSB_TRACK_TABLE_FULL and len(recs) == 8
        assert all(r["has_position"] and r["n_frames"] == 2 for r in recs)
        with pytest.raises(A.AdsbError) as e:
            t.update(_frames([(k, _even_odd(oracle, icaos[0], False)) for k in range(65)]))
        assert e.value.code == A.ADSB_E_CAPACITY
        t.reset()
        recs, flags = t.aircraft()
        assert len(recs) == 0 and flags == 0
