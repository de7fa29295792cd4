"""The track bank on the device (adsb_track_bank_*, air_rs_amd.TrackBank): one aircraft table per receiver, the
reference's one HashMap<u32, Aircraft> per display thread (src/adsb/tui.rs:22-42, web.rs:115), all updated by one
call over a multi-receiver frame list.  Receiver r must equal a separate TrackTable fed receiver r's part of every
update bit for bit, and the oracle's sequential restatement of aircraft.rs fed the same frames at the same times."""
import contextlib
import math

import numpy as np
import pytest

import air_rs_amd as A
from tests.traffic import ident_frame, position_frame, random_traffic

REF_EVEN, REF_ODD = "8D40621D58C386435CC412692AD6", "8D40621D58C382D690C8AC2863A7"  # aircraft.rs:201-212
REF_LAT, REF_LON = 52.2572021484375, 3.91937255859375
SHARED = [0x3ABCDE, 0xA00011, 0xA00022, 0xC0FFEE]  # outside random_traffic's range: active on every receiver


def _frames(items):
    """[(offset, 14 frame bytes)] -> FRAME_DTYPE array."""
    out = np.zeros(len(items), dtype=A.FRAME_DTYPE)
    for k, (off, b) in enumerate(items):
        out[k]["offset"] = off
        out[k]["bytes"] = np.frombuffer(bytes(b), dtype=np.uint8)
        out[k]["fixed_bit"] = 0xFF
    return out


def _icao(b):
    return (int(b[1]) << 16) | (int(b[2]) << 8) | int(b[3])


def _reicao(oracle, frame, icao):
    data = bytes([frame[0], (icao >> 16) & 0xFF, (icao >> 8) & 0xFF, icao & 0xFF]) + bytes(frame[4:11])
    crc = oracle.get_adsb_crc(data)
    return data + bytes([(crc >> 16) & 0xFF, (crc >> 8) & 0xFF, crc & 0xFF])


def _receiver_traffic(oracle, seed, n_frames, span_s=60.0, n_aircraft=12):
    """random_traffic for one receiver; its lowest aircraft fly under the SHARED ICAOs (other positions, callsigns)."""
    traffic = random_traffic(oracle, seed=seed, n_aircraft=n_aircraft, n_frames=n_frames, span_s=span_s)
    remap = dict(zip(sorted({_icao(fr) for _, fr in traffic}), SHARED))
    return [(t, _reicao(oracle, fr, remap[_icao(fr)]) if _icao(fr) in remap else fr) for t, fr in traffic]


def _concat(lists):
    return np.concatenate(lists) if lists else np.zeros(0, dtype=A.FRAME_DTYPE)


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


class _Oracles:
    """One oracle tracker per receiver, fed frame by frame; checks points as they come."""

    def __init__(self, oracle, n):
        self.ot = [oracle.tracker() for _ in range(n)]
        self.counts = [{} for _ in range(n)]
        self.n_new = 0

    def feed(self, r, frames, pts, base, sps):
        assert len(pts) == len(frames)
        for k, fr in enumerate(frames):
            new, s = self.ot[r].update(bytes(fr["bytes"]), float(base + int(fr["offset"])) * sps)
            icao = _icao(fr["bytes"])
            self.counts[r][icao] = self.counts[r].get(icao, 0) + 1
            assert pts[k]["icao"] == s.icao == icao and not pts[k]["flags"] & A.ADSB_TRACK_UNTRACKED
            assert bool(pts[k]["flags"] & A.ADSB_TRACK_NEW_POSITION) == new, (r, k)
            if new:
                self.n_new += 1
                assert (pts[k]["latitude"], pts[k]["longitude"]) == pytest.approx((s.latitude, s.longitude), abs=1e-9)

    def check_tables(self, recs_per_receiver):
        for r, recs in enumerate(recs_per_receiver):
            _same_table(recs, sorted(self.ot[r].aircraft(), key=lambda s: s.icao), self.counts[r])


def _check_against_tables(bank, tables, lists):
    """bank points of the last update and every receiver's records == the separate tables', bit for bit."""
    pts = bank.points()
    assert len(pts) == sum(len(x) for x in lists)
    a = 0
    for r, t in enumerate(tables):
        want = t.points()
        assert pts[a:a + len(want)].tobytes() == want.tobytes(), r
        a += len(want)
    recs, flags = bank.aircraft()
    assert len(recs) == len(tables) == len(flags)
    for r, t in enumerate(tables):
        want, wflags = t.aircraft()
        assert recs[r].tobytes() == want.tobytes(), r
        assert flags[r] == wflags
    return pts, recs, flags


@pytest.mark.gpu
@pytest.mark.parametrize("n_receivers,seed", [(1, 1), (3, 2), (8, 3), (64, 4)])
def test_bank_equals_separate_tables(gpu, oracle, n_receivers, seed):
    """Random traffic per receiver, some ICAOs on every receiver at once, fed in 3 s windows with a sample_base of
    each receiver's own: the bank equals R tables bit for bit (and, for R = 8, R oracle trackers)."""
    R = n_receivers
    sps, window = 1e-3, 3000                          # samples per update
    streams = [_receiver_traffic(oracle, 100 * seed + r, 400 if R == 64 else 1500) for r in range(R)]
    shift = [1000 * r + 7 for r in range(R)]          # receiver r's sample index = round(t / sps) + shift[r]
    cursor = [0] * R
    orc = _Oracles(oracle, R) if R == 8 else None
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackBank(d, R, max_frames=1 << 14, seconds_per_sample=sps) as bank, contextlib.ExitStack() as es:
        tables = [es.enter_context(A.TrackTable(d, max_frames=1 << 12, seconds_per_sample=sps)) for _ in range(R)]
        for u in range(60000 // window + 1):
            lists, bases = [], []
            for r in range(R):
                base = u * window + shift[r] - 100 * (r % 3)  # offsets >= 0: the window starts at u * window + shift
                items = []
                while cursor[r] < len(streams[r]) and round(streams[r][cursor[r]][0] / sps) < (u + 1) * window:
                    t, fr = streams[r][cursor[r]]
                    items.append((round(t / sps) + shift[r] - base, fr))
                    cursor[r] += 1
                lists.append(_frames(items))
                bases.append(base)
            bank.update(_concat(lists), [len(x) for x in lists], bases)
            for r, t in enumerate(tables):
                t.update(lists[r], bases[r])
            pts, recs, flags = _check_against_tables(bank, tables, lists)
            assert flags == [0] * R
            if orc:
                a = 0
                for r in range(R):
                    orc.feed(r, lists[r], pts[a:a + len(lists[r])], bases[r], sps)
                    a += len(lists[r])
                if u % 5 == 0:
                    orc.check_tables(recs)
        assert cursor == [len(s) for s in streams]
        recs, _ = bank.aircraft()
        for r in range(R):
            assert set(SHARED) <= {int(x) for x in recs[r]["icao"]}
            assert int(recs[r]["has_position"].sum()) >= 8
        if orc:
            orc.check_tables(recs)
            assert orc.n_new > 1000
        # the shared aircraft are different aircraft on different receivers: their records differ
        if R > 1:
            assert recs[0][recs[0]["icao"] == SHARED[0]].tobytes() != recs[1][recs[1]["icao"] == SHARED[0]].tobytes()


@pytest.mark.gpu
def test_same_icao_on_every_receiver(gpu, oracle):
    """The reference pair on receiver 0; the same ICAO on the others with other CPR messages and callsigns: every
    receiver keeps its own position and callsign, and no even/odd pair mixes receivers."""
    icao, sps = 0x40621D, 1e-3
    even2 = position_frame(oracle, icao, False, 93100, 51400)   # near the reference pair, not on it
    odd2 = position_frame(oracle, icao, True, 74250, 50220)
    odd_other = position_frame(oracle, icao, True, 12345, 67890)
    even3 = position_frame(oracle, icao, False, 40000, 20000)
    idents = [ident_frame(oracle, icao, [k + 1] * 8) for k in range(4)]
    first = [[(0, idents[0]), (10, bytes.fromhex(REF_EVEN))],      # r0: the reference pair across the two updates
             [(0, idents[1])],                                     # r1: only an odd half later (r0 has an even)
             [(5, even2)],                                         # r2: a pair of its own
             [(3, even3), (8, idents[3])]]                         # r3: an even half, nothing in the second update
    second = [[(20, bytes.fromhex(REF_ODD))],
              [(30, odd_other)],
              [(25, odd2), (40, idents[2])],
              []]
    R = len(first)
    orc = _Oracles(oracle, R)
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackBank(d, R, max_frames=64, seconds_per_sample=sps) as bank, contextlib.ExitStack() as es:
        tables = [es.enter_context(A.TrackTable(d, max_frames=64, seconds_per_sample=sps)) for _ in range(R)]
        for upd, base in ((first, 0), (second, 1000)):
            lists = [_frames(x) for x in upd]
            bank.update(_concat(lists), [len(x) for x in lists], base)   # scalar sample_base: the same for every r
            for r, t in enumerate(tables):
                t.update(lists[r], base)
            pts, recs, flags = _check_against_tables(bank, tables, lists)
            a = 0
            for r in range(R):
                orc.feed(r, lists[r], pts[a:a + len(lists[r])], base, sps)
                a += len(lists[r])
        orc.check_tables(recs)
        assert flags == [0] * R
        assert [len(x) for x in recs] == [1] * R and all(int(x["icao"][0]) == icao for x in recs)
        r0, r1, r2, r3 = (x[0] for x in recs)
        assert r0["has_position"] and abs(r0["latitude"] - REF_LAT) < 1e-9 and abs(r0["longitude"] - REF_LON) < 1e-9
        assert not r1["has_position"] and not r3["has_position"]
        assert r2["has_position"] and (r2["latitude"], r2["longitude"]) != (r0["latitude"], r0["longitude"])
        assert [x["callsign"].decode() for x in (r0, r1, r2, r3)] == ["AAAAAAAA", "BBBBBBBB", "CCCCCCCC", "DDDDDDDD"]
        assert [int(x["n_frames"]) for x in (r0, r1, r2, r3)] == [3, 2, 3, 2]
        assert r0["last_contact"] == 1020 * sps and r1["last_contact"] == 1030 * sps and r3["last_contact"] == 3 * sps


@pytest.mark.gpu
def test_any_cut_gives_the_same_result(gpu, oracle):
    """Each receiver's stream in one update equals the same streams cut at random, with many updates in which some
    receivers get no frames at all."""
    R, sps = 5, 1e-3
    streams = [_receiver_traffic(oracle, 700 + r, 800, span_s=80.0) for r in range(R)]
    samples = [[round(t / sps) for t, _ in s] for s in streams]
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackBank(d, R, max_frames=1 << 13, seconds_per_sample=sps) as bank:
        whole = [_frames([(samples[r][k], fr) for k, (_, fr) in enumerate(streams[r])]) for r in range(R)]
        bank.update(_concat(whole), [len(x) for x in whole], [0] * R)
        want_pts = bank.points()
        want_recs, want_flags = bank.aircraft()
        assert want_flags == [0] * R and int((want_pts["flags"] & A.ADSB_TRACK_NEW_POSITION != 0).sum()) > 500
        edges = np.concatenate([[0], np.cumsum([len(x) for x in whole])])
        rng = np.random.default_rng(11)
        for rep in range(2):
            bank.reset()
            cursor, got, n_upd, n_some_empty = [0] * R, [[] for _ in range(R)], 0, 0
            while any(cursor[r] < len(whole[r]) for r in range(R)):
                take = [int(rng.integers(0, 4)) if rng.random() < 0.5 else int(rng.integers(0, 60)) for _ in range(R)]
                take = [min(k, len(whole[r]) - cursor[r]) for r, k in enumerate(take)]
                lists, bases = [], []
                for r in range(R):
                    part = whole[r][cursor[r]:cursor[r] + take[r]].copy()
                    base = samples[r][cursor[r]] if take[r] else 0     # offsets relative to the part's first frame
                    part["offset"] -= base
                    lists.append(part)
                    bases.append(base)
                bank.update(_concat(lists), take, bases)
                pts = bank.points()
                a = 0
                for r in range(R):
                    got[r].append(pts[a:a + take[r]])
                    a += take[r]
                    cursor[r] += take[r]
                n_upd += 1
                n_some_empty += 0 in take
            assert n_upd > 30 and n_some_empty > 10
            for r in range(R):
                assert np.concatenate(got[r]).tobytes() == want_pts[edges[r]:edges[r + 1]].tobytes(), r
            recs, flags = bank.aircraft()
            assert flags == [0] * R
            for r in range(R):
                assert recs[r].tobytes() == want_recs[r].tobytes(), r


@pytest.mark.gpu
def test_update_launch_equals_oracle_per_channel(gpu, oracle):
    """Modulated traffic in a 4-channel device buffer over 24 launches (one channel empty in some; one launch whose
    list max_out truncates): after each launch update_launch applies exactly what adsb_fetch / per_channel_counts
    return -- the same as a bank fed those host lists, and the oracle's points and tables per channel."""
    import torch

    from tests.golden.make_golden import modulate, place
    C_, n, stride, R, max_out = 4, 20_000, 20_480, 5, 256
    sps = 1.0 / n                                   # a launch spans 1 s: the 10 s window covers 10 launches
    streams = [iter(_receiver_traffic(oracle, 900 + c, 1200, n_aircraft=60)) for c in range(C_)]
    orc = _Oracles(oracle, R)
    last_pos = {}                                   # (channel, icao, odd) -> launch of the last position message
    n_cross = n_trunc = n_empty = 0
    with A.AdsbDemod(max_samples=n, max_out=max_out, max_channels=C_, host_staging=False) as d, \
            A.TrackBank(d, R, max_frames=max_out, seconds_per_sample=sps) as bank, \
            A.TrackBank(d, R, max_frames=max_out, seconds_per_sample=sps) as host_bank, \
            A.TrackBank(d, C_ - 1, max_frames=max_out, seconds_per_sample=sps) as small:
        with pytest.raises(A.AdsbError) as e:
            bank.update_launch()                    # no launch yet
        assert e.value.code == A.ADSB_E_STATE
        for launch in range(24):
            gap = 260 if launch == 14 else 500      # launch 14: ~296 frames for 256 places
            host = np.full((C_, stride, 2), 77, dtype=np.int8)  # padding between channels is never looked at
            for c in range(C_):
                quiet = c == 2 and launch % 4 == 1
                items = [] if quiet else [(300 + gap * k, modulate(next(streams[c])[1], (80, 30), None))
                                          for k in range((n - 600) // gap)]
                host[c, :n] = place(n, items, np.int8, floor=3, seed=1000 * launch + c)
            buf = torch.from_numpy(host).cuda()
            d.demod_device_async(buf.data_ptr(), n, C_, stride)
            bases = [launch * n + 3 * r for r in range(R)]
            bank.update_launch(bases)
            if launch == 0:
                with pytest.raises(A.AdsbError) as e:
                    small.update_launch()           # more channels than receivers
                assert e.value.code == A.ADSB_E_ARG
            frames, counts, _, flags = d.fetch(n_channels=C_)
            counts = [int(x) for x in counts] + [0] * (R - C_)
            assert sum(counts) == len(frames)
            if launch == 14:
                assert flags & A.ADSB_FLAG_TRUNCATED and len(frames) == max_out and counts[3] < counts[0]
                n_trunc += 1
            else:
                assert flags == 0 and all(k >= 30 for c, k in enumerate(counts[:C_]) if not (c == 2 and launch % 4 == 1))
            if launch % 4 == 1:
                assert counts[2] == 0
                n_empty += 1
            host_bank.update(frames, counts, bases)
            pts = bank.points()
            assert pts.tobytes() == host_bank.points().tobytes()
            recs, bflags = bank.aircraft()
            hrecs, hflags = host_bank.aircraft()
            assert bflags == hflags == [0] * R and len(recs[R - 1]) == 0
            assert all(a.tobytes() == b.tobytes() for a, b in zip(recs, hrecs))
            a = 0
            for r in range(R):
                part = frames[a:a + counts[r]]
                orc.feed(r, part, pts[a:a + counts[r]], bases[r], sps)
                for k, fr in enumerate(part):
                    b = fr["bytes"]
                    if 9 <= int(b[4]) >> 3 <= 18:   # a position message (msgs.rs:122-124)
                        odd = (int(b[6]) >> 2) & 1
                        if pts[a + k]["flags"] & A.ADSB_TRACK_NEW_POSITION:
                            n_cross += last_pos[(r, _icao(b), 1 - odd)] < launch
                        last_pos[(r, _icao(b), odd)] = launch
                a += counts[r]
            if launch % 6 == 5 or launch == 14:
                orc.check_tables(recs)
        orc.check_tables(recs)
    assert n_trunc == 1 and n_empty == 6
    assert orc.n_new > 500 and n_cross > 200, (orc.n_new, n_cross)


def _even_odd(oracle, icao, odd):
    # the CPR halves of the reference pair, under another ICAO: every such pair decodes
    return position_frame(oracle, icao, odd, 74158 if odd else 93000, 50194 if odd else 51372)


@pytest.mark.gpu
def test_capacity_is_per_receiver(gpu, oracle):
    """max_aircraft = 8: receiver 1 sees 12 new ICAOs and admits its lowest 8, sets its own flag and marks the
    others' frames UNTRACKED; receivers 0 and 2 (some ICAOs shared with receiver 1) match their tables, flags clear."""
    rng = np.random.default_rng(3)
    pool = [int(x) for x in rng.choice(np.arange(0x100000, 0xF00000), size=20, replace=False)]
    icaos = [pool[:3] + pool[12:14], pool[:12], pool[14:19]]    # receiver 1 overflows; 0 shares three of its ICAOs
    orders = [list(rng.permutation(len(x))) for x in icaos]     # list order unrelated to ICAO order
    admitted = set(sorted(icaos[1])[:8])
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackBank(d, 3, max_aircraft=8, max_frames=64, seconds_per_sample=1e-3) as bank, \
            contextlib.ExitStack() as es:
        tables = [es.enter_context(A.TrackTable(d, max_aircraft=8, max_frames=64, seconds_per_sample=1e-3))
                  for _ in range(3)]
        for odd, t0 in ((False, 0), (True, 1000)):              # one second later: the odd halves
            lists = [_frames([(t0 + 10 * k, _even_odd(oracle, icaos[r][j], odd)) for k, j in enumerate(orders[r])])
                     for r in range(3)]
            bank.update(_concat(lists), [len(x) for x in lists])
            for r, t in enumerate(tables):
                t.update(lists[r])
            pts, recs, flags = _check_against_tables(bank, tables, lists)
            assert flags == [0, A.ADSB_TRACK_TABLE_FULL, 0]
            p1 = pts[len(lists[0]):len(lists[0]) + len(lists[1])]
            for k, j in enumerate(orders[1]):
                assert p1[k]["icao"] == icaos[1][j]
                if icaos[1][j] not in admitted:
                    assert p1[k]["flags"] == A.ADSB_TRACK_UNTRACKED
                else:
                    assert p1[k]["flags"] == (A.ADSB_TRACK_NEW_POSITION if odd else 0)
            assert [int(x) for x in recs[1]["icao"]] == sorted(admitted)
            assert [len(x) for x in recs] == [5, 8, 5]
            assert not any(p["flags"] & A.ADSB_TRACK_UNTRACKED for p in np.concatenate([pts[:len(lists[0])],
                                                                                         pts[-len(lists[2]):]]))
        assert all(x["has_position"].all() and (x["n_frames"] == 2).all() for x in recs)
        with pytest.raises(A.AdsbError) as e:
            bank.update(_frames([(k, _even_odd(oracle, pool[0], False)) for k in range(65)]), [65, 0, 0])
        assert e.value.code == A.ADSB_E_CAPACITY
        with pytest.raises(A.AdsbError) as e:
            bank.update(_frames([(0, _even_odd(oracle, pool[0], False))]), [1, 1, 0])   # counts do not sum to n
        assert e.value.code == A.ADSB_E_ARG


@pytest.mark.gpu
def test_reset_empties_every_receiver(gpu, oracle):
    R, sps = 3, 1e-3
    streams = [_receiver_traffic(oracle, 40 + r, 300, span_s=20.0) for r in range(R)]
    lists = [_frames([(round(t / sps), fr) for t, fr in s]) for s in streams]
    later = [_frames([(round(t / sps), fr) for t, fr in s]) for s in
             (_receiver_traffic(oracle, 60 + r, 200, span_s=20.0) for r in range(R))]
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackBank(d, R, max_frames=1 << 12, seconds_per_sample=sps) as bank, \
            A.TrackBank(d, R, max_frames=1 << 12, seconds_per_sample=sps) as fresh:
        with pytest.raises(A.AdsbError) as e:
            bank.points()
        assert e.value.code == A.ADSB_E_STATE
        bank.update(_concat(lists), [len(x) for x in lists], 0)
        recs, _ = bank.aircraft()
        assert all(len(x) >= 10 for x in recs)
        bank.reset()
        recs, flags = bank.aircraft()
        assert [len(x) for x in recs] == [0] * R and flags == [0] * R
        with pytest.raises(A.AdsbError) as e:
            bank.points()
        assert e.value.code == A.ADSB_E_STATE
        for b in (bank, fresh):
            b.update(_concat(later), [len(x) for x in later], [5, 6, 7])
        assert bank.points().tobytes() == fresh.points().tobytes()
        recs, flags = bank.aircraft()
        frecs, fflags = fresh.aircraft()
        assert flags == fflags == [0] * R
        assert all(a.tobytes() == b.tobytes() for a, b in zip(recs, frecs))
        bank.update(_concat([]), [0] * R)                       # an empty update: no points, nothing changes
        assert len(bank.points()) == 0
        assert all(a.tobytes() == b.tobytes() for a, b in zip(bank.aircraft()[0], frecs))
