"""Per-frame summaries and the changed list of a track table / bank (adsb_track_*_summaries_reserve, TrackTable /
TrackBank .summaries() and .changed()): what the reference's web thread broadcasts, one AircraftSummary per packet as
the aircraft stands right after that packet (src/adsb/web.rs:117-128, aircraft.rs:141-165).  The yardstick is the
oracle's per-packet summary (oracle_tracker_update's `out`), fed the same frames at the same times; the bit-for-bit
properties (last frame = record, any cut, bank = tables, determinism) are checked as bytes."""
import contextlib
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import air_rs_amd as A
from tests.traffic import ident_frame, position_frame, random_traffic
from tests.velocity_traffic import velocity_traffic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9                                    # what the table tests allow against the oracle


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


def _close(a, b):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= TOL


def _same_summary(rec, s, n_frames, where):
    """One device summary against the oracle's summary of the same packet: callsign, altitude and has_position
    exactly, the three doubles within TOL (both NaN = equal), n_frames = the running count."""
    assert int(rec["icao"]) == s.icao, where
    assert rec["callsign"].decode("latin-1") == s.callsign.decode("latin-1"), where
    assert int(rec["altitude"]) == s.altitude and bool(rec["has_position"]) == bool(s.has_position), where
    assert _close(float(rec["latitude"]), s.latitude) and _close(float(rec["longitude"]), s.longitude), where
    assert _close(float(rec["last_contact"]), s.last_contact), where
    assert int(rec["n_frames"]) == n_frames, where


def _empty(icao):
    rec = np.zeros((), dtype=A.AIRCRAFT_DTYPE)
    rec["icao"], rec["last_contact"] = icao, np.nan
    return rec


def _is_position(b):
    return 9 <= int(b[4]) >> 3 <= 18          # msgs.rs:122-124


def _is_ident(b):
    return 1 <= int(b[4]) >> 3 <= 4


# ---- 1 + 2: streaming against the oracle; the last frame's summary is the record ------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", [21, 22])
def test_streaming_summaries_equal_oracle(gpu, oracle, seed):
    """The set-up of test_streaming_table_equals_oracle: every frame's summary equals what the oracle returned for that
    packet, and after every update the summary at each aircraft's last frame is its aircraft() row, as bytes."""
    from tests.golden.make_golden import modulate, place
    traffic = random_traffic(oracle, seed=seed, n_aircraft=35, n_frames=3000)
    chunk, gap = 20_000, 400
    sps = 1.0 / chunk
    n = 300 + gap * len(traffic) + 600
    items = [(300 + gap * k, modulate(fr, (80, 30), None)) for k, (_, fr) in enumerate(traffic)]
    iq = place(n, items, np.int8, floor=3, seed=seed)
    ot = oracle.tracker()
    counts, callsign_from = {}, {}
    n_frames = n_inherit = n_old_callsign = n_buf = 0
    with A.AdsbDemod(max_samples=chunk, max_out=1 << 12) as d, \
            A.TrackTable(d, max_frames=1 << 12, seconds_per_sample=sps) as table, \
            A.Feed(d, max_chunk=chunk, carry=False) as f:
        table.summaries_reserve()

        def consume():
            nonlocal n_frames, n_inherit, n_old_callsign, n_buf
            frames, flags, first = f.pop()
            assert flags == 0
            known = set(counts)
            table.update(frames, first)
            sums = table.summaries()
            assert len(sums) == len(frames)
            seen, last = set(), {}
            for k, fr in enumerate(frames):
                _, s = ot.update(bytes(fr["bytes"]), float(first + int(fr["offset"])) * sps)
                icao = _icao(fr["bytes"])
                counts[icao] = counts.get(icao, 0) + 1
                _same_summary(sums[k], s, counts[icao], (n_buf, k))
                n_inherit += icao not in seen and icao in known
                seen.add(icao)
                last[icao] = k
                if _is_ident(fr["bytes"]):
                    callsign_from[icao] = n_buf
                n_old_callsign += callsign_from.get(icao, n_buf) < n_buf
            n_frames += len(frames)
            recs, tflags = table.aircraft()
            assert tflags == 0
            rows = {int(r["icao"]): r for r in recs}
            for icao, k in last.items():                       # 2: last frame = record, bit for bit
                assert sums[k].tobytes() == rows[icao].tobytes(), (n_buf, icao)
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
    assert n_buf >= 50 and n_frames >= 2900
    # the lists inherit from the table: frames that are their aircraft's first in their update while the table
    # already holds it, and frames whose callsign comes from an earlier update
    assert n_inherit >= 1200 and n_old_callsign >= 1200, (n_inherit, n_old_callsign)


# ---- 3: any cut ------------------------------------------------------------------------------------------------------
def _host_list(traffic, sps):
    return _frames([(round(t / sps), fr) for t, fr in traffic])


@pytest.mark.gpu
def test_any_cut_gives_the_same_summaries(gpu, oracle):
    """One list applied whole and in random cuts (single frames first, so every even / odd pair is cut; empty updates
    in between): the concatenated summaries are the same bytes."""
    sps = 1e-3
    frames = _host_list(random_traffic(oracle, seed=41, n_aircraft=20, n_frames=2500, span_s=80.0), sps)
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_frames=1 << 12, seconds_per_sample=sps) as t:
        t.summaries_reserve()
        t.update(frames)
        whole = t.summaries()
        assert len(whole) == len(frames) and int(whole["has_position"].sum()) > 1000
        ot, cnt = oracle.tracker(), {}
        for k, fr in enumerate(frames):                            # and the whole list is the oracle's
            _, s = ot.update(bytes(fr["bytes"]), float(int(fr["offset"])) * sps)
            cnt[s.icao] = cnt.get(s.icao, 0) + 1
            _same_summary(whole[k], s, cnt[s.icao], k)
        rng = np.random.default_rng(11)
        for rep in range(3):
            t.reset()
            sizes = [1] * 64 + [0, 0]                                # 0: an empty update
            for x in rng.integers(1, 201, size=len(frames)):
                sizes += [int(x)] if len(sizes) % 3 else [int(x), 0]
            parts, a, n_empty = [], 0, 0
            for sz in sizes:
                if a >= len(frames):
                    break
                t.update(frames[a:a + sz])
                got = t.summaries()
                assert len(got) == min(sz, len(frames) - a)
                parts.append(got)
                n_empty += sz == 0
                if sz == 0:
                    assert len(t.changed()[0]) == 0
                a += sz
            assert n_empty >= 5
            assert np.concatenate(parts).tobytes() == whole.tobytes()


# ---- 4: a bank's receiver = a table of its own ----------------------------------------------------------------------
SHARED = [0x3ABCDE, 0xA00011, 0xA00022, 0xC0FFEE]    # active on every receiver


def _reicao(oracle, frame, icao):
    data = bytes([frame[0], (icao >> 16) & 0xFF, (icao >> 8) & 0xFF, icao & 0xFF]) + bytes(frame[4:11])
    crc = oracle.get_adsb_crc(data)
    return data + bytes([(crc >> 16) & 0xFF, (crc >> 8) & 0xFF, crc & 0xFF])


def _receiver_traffic(oracle, seed, n_frames, n_aircraft=12):
    traffic = velocity_traffic(oracle, seed=seed, n_aircraft=n_aircraft, n_frames=n_frames, span_s=60.0,
                               velocity_share=0.2)
    remap = dict(zip(sorted({_icao(fr) for _, fr in traffic}), SHARED))
    return [(t, _reicao(oracle, fr, remap[_icao(fr)]) if _icao(fr) in remap else fr) for t, fr in traffic]


def _concat(lists):
    return np.concatenate(lists) if lists else np.zeros(0, dtype=A.FRAME_DTYPE)


def _bank_equals_tables(bank, tables, lists):
    sums = bank.summaries()
    recs, heard, vel, counts = bank.changed()
    assert len(sums) == sum(len(x) for x in lists) and sum(counts) == len(recs) == len(heard) == len(vel)
    a = c = 0
    for r, t in enumerate(tables):
        want = t.summaries()
        assert len(want) == len(lists[r])
        assert sums[a:a + len(want)].tobytes() == want.tobytes(), r
        a += len(want)
        wrecs, wheard, wvel = t.changed()
        assert counts[r] == len(wrecs), r
        assert recs[c:c + counts[r]].tobytes() == wrecs.tobytes(), r
        assert heard[c:c + counts[r]].tobytes() == wheard.tobytes(), r
        assert vel[c:c + counts[r]].tobytes() == wvel.tobytes(), r
        c += counts[r]
    return sums


@pytest.mark.gpu
@pytest.mark.parametrize("n_receivers,seed", [(1, 1), (3, 2), (8, 3), (64, 4)])
def test_bank_summaries_equal_separate_tables(gpu, oracle, n_receivers, seed):
    R = n_receivers
    sps, window = 1e-3, 6000
    streams = [_receiver_traffic(oracle, 300 * seed + r, 300 if R == 64 else 1000) for r in range(R)]
    shift = [1000 * r + 7 for r in range(R)]
    cursor = [0] * R
    n_shared_multi = 0
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackBank(d, R, max_frames=1 << 14, seconds_per_sample=sps) as bank, contextlib.ExitStack() as es:
        tables = [es.enter_context(A.TrackTable(d, max_frames=1 << 11, seconds_per_sample=sps)) for _ in range(R)]
        bank.summaries_reserve()
        for t in tables:
            t.summaries_reserve()
        for u in range(60000 // window + 1):
            lists, bases = [], []
            for r in range(R):
                base = u * window + shift[r] - 100 * (r % 3)
                items = []
                while cursor[r] < len(streams[r]) and round(streams[r][cursor[r]][0] / sps) < (u + 1) * window:
                    t_s, fr = streams[r][cursor[r]]
                    items.append((round(t_s / sps) + shift[r] - base, fr))
                    cursor[r] += 1
                lists.append(_frames(items))
                bases.append(base)
            bank.update(_concat(lists), [len(x) for x in lists], bases)
            for r, t in enumerate(tables):
                t.update(lists[r], bases[r])
            sums = _bank_equals_tables(bank, tables, lists)
            n_shared_multi += int(np.isin(sums["icao"], SHARED).sum())
        assert cursor == [len(s) for s in streams]
        assert n_shared_multi >= 50 * R                    # the same ICAOs were active on several receivers


@pytest.mark.gpu
def test_bank_update_launch_summaries(gpu, oracle):
    """update_launch (the ctx's device list, split by its channel prefix) leaves the summaries and the changed list a
    bank fed the fetched host lists leaves."""
    import torch

    from tests.golden.make_golden import modulate, place
    C_, n, stride, R = 3, 20_000, 20_480, 4
    sps = 1.0 / n
    streams = [iter(_receiver_traffic(oracle, 700 + c, 400, n_aircraft=20)) for c in range(C_)]
    with A.AdsbDemod(max_samples=n, max_out=512, max_channels=C_, host_staging=False) as d, \
            A.TrackBank(d, R, max_frames=512, seconds_per_sample=sps) as bank, \
            A.TrackBank(d, R, max_frames=512, seconds_per_sample=sps) as host_bank:
        bank.summaries_reserve()
        host_bank.summaries_reserve()
        total = 0
        for launch in range(6):
            host = np.full((C_, stride, 2), 77, dtype=np.int8)
            for c in range(C_):
                items = [(300 + 500 * k, modulate(next(streams[c])[1], (80, 30), None)) for k in range((n - 600) // 500)]
                host[c, :n] = place(n, items, np.int8, floor=3, seed=50 * launch + c)
            buf = torch.from_numpy(host).cuda()
            d.demod_device_async(buf.data_ptr(), n, C_, stride)
            bases = [launch * n + 3 * r for r in range(R)]
            bank.update_launch(bases)
            frames, counts, _, flags = d.fetch(n_channels=C_)
            assert flags == 0
            counts = [int(x) for x in counts] + [0] * (R - C_)
            host_bank.update(frames, counts, bases)
            got, want = bank.summaries(), host_bank.summaries()
            assert len(got) == len(frames) and got.tobytes() == want.tobytes()
            for x, y in zip(bank.changed(), host_bank.changed()):
                assert (x == y) if isinstance(x, list) else x.tobytes() == y.tobytes()
            total += len(frames)
        assert total >= 6 * C_ * 30


# ---- 5: a full table, and an aircraft heard again after expire -------------------------------------------------------
def _even_odd(oracle, icao, odd):
    return position_frame(oracle, icao, odd, 74158 if odd else 93000, 50194 if odd else 51372)


@pytest.mark.gpu
def test_full_table_and_expire(gpu, oracle):
    rng = np.random.default_rng(5)
    icaos = [int(x) for x in rng.choice(np.arange(0x100000, 0xF00000), size=12, replace=False)]
    order = [int(x) for x in rng.permutation(12)]
    admitted = set(sorted(icaos)[:8])
    sps = 1e-3
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_aircraft=8, max_frames=64, seconds_per_sample=sps) as t:
        t.summaries_reserve()
        ot, cnt = oracle.tracker(), {}
        for base, odd in ((0, False), (1000, True)):
            items = [(base + 10 * k, _even_odd(oracle, icaos[j], odd)) for k, j in enumerate(order)]
            items += [(base + 500 + 10 * k, ident_frame(oracle, icaos[j], [k + 1] * 8)) for k, j in enumerate(order)]
            t.update(_frames(items))
            sums, pts = t.summaries(), t.points()
            for k, (off, fr) in enumerate(items):
                icao = _icao(fr)
                if icao in admitted:
                    _, s = ot.update(fr, off * sps)
                    cnt[icao] = cnt.get(icao, 0) + 1
                    _same_summary(sums[k], s, cnt[icao], k)
                else:                                       # turned away: the empty record with its ICAO
                    assert pts[k]["flags"] == A.ADSB_TRACK_UNTRACKED
                    assert sums[k].tobytes() == _empty(icao).tobytes(), k
            recs, heard, vel = t.changed()
            assert [int(x) for x in recs["icao"]] == sorted(admitted)
            assert recs.tobytes() == t.aircraft()[0].tobytes()
        assert int(sums["has_position"].sum()) == 16 and t.aircraft()[1] == A.ADSB_TRACK_TABLE_FULL
        # everything is older than t = 5 s: evicted.  One aircraft comes back, is evicted again and comes back once more
        back = sorted(admitted)[3]
        t.expire(5.0)
        assert len(t.aircraft()[0]) == 0
        t.update(_frames([(6000, ident_frame(oracle, back, [9] * 8))]))
        s0 = t.summaries()[0]
        want = _empty(back)
        want["n_frames"], want["callsign"] = 1, b"IIIIIIII"
        assert s0.tobytes() == want.tobytes()
        t.expire(6.5)
        t.update(_frames([(7000, bytes([0x8D, back >> 16, (back >> 8) & 0xFF, back & 0xFF] + [0] * 10)),
                          (7100, _even_odd(oracle, back, False))]))
        sums = t.summaries()
        first = _empty(back)
        first["n_frames"] = 1                               # no callsign, last_contact NaN: the record started over
        assert sums[0].tobytes() == first.tobytes()
        assert sums[1]["n_frames"] == 2 and sums[1]["last_contact"] == 7100 * sps and not sums[1]["has_position"]
        assert sums[1]["callsign"] == b""
        assert sums[1]["altitude"] == oracle.packet_new(_even_odd(oracle, back, False)).altitude != 0


# ---- 6: one long segment ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_aircraft_owns_the_whole_list(gpu, oracle):
    """max_frames = 65 536 frames of ONE aircraft (even, odd and identification messages mixed) in one update, equal
    to the oracle frame by frame: the case a per-frame walk over the segment would make quadratic.  Frames are 0.1 s
    apart, so the pairs step's 10 s window holds at most 100 of them.  Results only; the time is the timing tool's."""
    n, sps, step = 1 << 16, 1e-3, 100
    palette = [fr for _, fr in random_traffic(oracle, seed=61, n_aircraft=1, n_frames=512, span_s=60.0)]
    assert len({_icao(fr) for fr in palette}) == 1
    assert sum(_is_ident(fr) for fr in palette) >= 20 and sum(_is_position(fr) for fr in palette) >= 400
    pick = np.random.default_rng(61).integers(0, len(palette), size=n)
    frames = np.zeros(n, dtype=A.FRAME_DTYPE)
    pal = np.array([np.frombuffer(fr, dtype=np.uint8) for fr in palette])
    frames["bytes"] = pal[pick]
    frames["offset"] = np.arange(n, dtype=np.uint64) * step
    frames["fixed_bit"] = 0xFF
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_aircraft=16, max_frames=n, seconds_per_sample=sps) as t:
        t.summaries_reserve()
        t.update(frames)
        sums = t.summaries()
        recs, flags = t.aircraft()
        changed = t.changed()[0]
    assert len(sums) == n and len(recs) == 1 and flags == 0
    assert sums[-1].tobytes() == recs[0].tobytes() == changed[0].tobytes() and len(changed) == 1
    ot = oracle.tracker()
    n_fix_changes = 0
    for k in range(n):
        new, s = ot.update(palette[pick[k]], float(k * step) * sps)
        _same_summary(sums[k], s, k + 1, k)
        n_fix_changes += new
    assert n_fix_changes > 10_000 and len(set(sums["callsign"])) >= 20


# ---- 7: the changed list ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_changed_list(gpu, oracle):
    from air_rs_amd import _lib
    sps = 1e-3
    traffic = velocity_traffic(oracle, seed=71, n_aircraft=40, n_frames=3000, span_s=60.0)
    frames = _host_list(traffic, sps)
    L = _lib.load()
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_aircraft=30, max_frames=1 << 12, seconds_per_sample=sps) as t:
        t.summaries_reserve()
        n_untracked = n_vel = 0
        for a in range(0, len(frames), 40):
            part = frames[a:a + 40]
            t.update(part)
            pts = t.points()
            tracked = sorted({int(p["icao"]) for p in pts if not p["flags"] & A.ADSB_TRACK_UNTRACKED})
            n_untracked += len({int(p["icao"]) for p in pts}) - len(tracked)
            recs, heard, vel = t.changed()
            assert [int(x) for x in recs["icao"]] == tracked
            all_recs, all_heard, all_vel = t.aircraft()[0], t.last_heard(), t.velocity()
            rows = np.searchsorted(all_recs["icao"], recs["icao"])
            assert recs.tobytes() == all_recs[rows].tobytes()
            assert heard.tobytes() == all_heard[rows].tobytes()
            assert vel.tobytes() == all_vel[rows].tobytes()
            n_vel += int((vel["subtype"] != 0).sum())
        assert n_untracked > 50 and n_vel > 200
        # *n counts them all when max is smaller; NULL arrays are allowed
        n = C.c_size_t()
        few = np.zeros(3, dtype=A.AIRCRAFT_DTYPE)
        assert L.adsb_track_table_fetch_changed(t._h, few.ctypes.data, None, None, 3, C.byref(n)) == A.ADSB_OK
        assert n.value == len(recs) > 3 and few.tobytes() == recs[:3].tobytes()
        assert L.adsb_track_table_fetch_changed(t._h, None, None, None, 0, C.byref(n)) == A.ADSB_OK
        assert n.value == len(recs)
        # NULL out with max > 0 (the check the CPU tier cannot make: it needs a live table)
        assert L.adsb_track_table_fetch_summaries(t._h, None, 4, C.byref(n)) == A.ADSB_E_ARG
        # slots move with expire and reset: no changed list until the next update; the summaries stay (like points)
        before = t.summaries()
        t.expire(10.0)
        with pytest.raises(A.AdsbError) as e:
            t.changed()
        assert e.value.code == A.ADSB_E_STATE
        assert t.summaries().tobytes() == before.tobytes()
        t.update(frames[:5])
        assert len(t.changed()[0]) == len({int(p["icao"]) for p in t.points() if not p["flags"] & A.ADSB_TRACK_UNTRACKED})
        t.reset()
        for call in (t.changed, t.summaries, t.summaries_device):
            with pytest.raises(A.AdsbError) as e:
                call()
            assert e.value.code == A.ADSB_E_STATE
        t.update(frames[:5])                               # an empty table admits them all
        assert len(t.changed()[0]) == len({_icao(fr["bytes"]) for fr in frames[:5]}) and t.summaries_device()
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackBank(d, 2, max_frames=64, seconds_per_sample=sps) as b:
        b.summaries_reserve()
        b.update(frames[:20], [12, 8])
        assert sum(b.changed()[3]) == len(b.changed()[0]) >= 2
        assert L.adsb_track_bank_fetch_summaries(b._h, None, 4, C.byref(n)) == A.ADSB_E_ARG
        b.expire(-math.inf)
        with pytest.raises(A.AdsbError) as e:
            b.changed()
        assert e.value.code == A.ADSB_E_STATE
        b.reset()
        with pytest.raises(A.AdsbError) as e:
            b.summaries()
        assert e.value.code == A.ADSB_E_STATE


# ---- 8 + 9: opt-in, determinism --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_opt_in_and_determinism(gpu, oracle):
    sps = 1e-3
    frames = _host_list(velocity_traffic(oracle, seed=81, n_aircraft=30, n_frames=2000, span_s=60.0), sps)
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, contextlib.ExitStack() as es:
        plain, res1, res2 = (es.enter_context(A.TrackTable(d, max_aircraft=25, max_frames=256, seconds_per_sample=sps))
                             for _ in range(3))
        for call in (plain.summaries, plain.changed, plain.summaries_device):
            with pytest.raises(A.AdsbError) as e:
                call()
            assert e.value.code == A.ADSB_E_STATE
        res1.summaries_reserve()
        res2.summaries_reserve()
        with pytest.raises(A.AdsbError) as e:
            res1.summaries()                               # reserved, but no update yet
        assert e.value.code == A.ADSB_E_STATE
        for a in range(0, len(frames), 211):
            part = frames[a:a + 211]
            for t in (plain, res1, res2):
                t.update(part)
            with pytest.raises(A.AdsbError):
                plain.summaries()
            assert res1.summaries().tobytes() == res2.summaries().tobytes()          # 9: two tables, the same bytes
            for x, y in zip(res1.changed(), res2.changed()):
                assert x.tobytes() == y.tobytes()
            assert plain.points().tobytes() == res1.points().tobytes()               # 8: the reserve changes nothing
            assert plain.aircraft()[0].tobytes() == res1.aircraft()[0].tobytes()
            assert plain.aircraft()[1] == res1.aircraft()[1]
            assert plain.last_heard().tobytes() == res1.last_heard().tobytes()
            assert plain.velocity().tobytes() == res1.velocity().tobytes()
        assert plain.aircraft()[1] == A.ADSB_TRACK_TABLE_FULL


# ---- 10: tools/replay.py --web ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_replay_web(gpu, oracle, tmp_path):
    """tools/replay.py --web on a .c16 capture: one JSON line per frame, the reference's AircraftSummary keys, the
    oracle's per-packet values."""
    from tests.golden.make_golden import modulate, place
    traffic = random_traffic(oracle, seed=91, n_aircraft=15, n_frames=400, span_s=10.0)
    chunk, per_chunk, gap = 20_000, 40, 400
    offsets = [chunk * (k // per_chunk) + 300 + gap * (k % per_chunk) for k in range(len(traffic))]
    n = chunk * (len(traffic) // per_chunk + 2)
    iq = place(n, [(o, modulate(fr, (80, 30), None)) for o, (_, fr) in zip(offsets, traffic)], np.int16, floor=3,
               seed=91)
    path = tmp_path / "capture.c16"
    iq.astype("<i2").tofile(path)
    sps = 0.5e-6
    tool = os.path.join(ROOT, "tools", "replay.py")
    out = subprocess.run([sys.executable, tool, str(path), "--web"], capture_output=True, text=True, timeout=300,
                         check=True).stdout
    lines = out.splitlines()
    assert len(lines) == len(traffic)
    ot = oracle.tracker()
    n_pos = 0
    for line, off, (_, fr) in zip(lines, offsets, traffic):
        _, s = ot.update(fr, off * sps)
        got = json.loads(line)
        assert list(got) == ["icao", "callsign", "altitude", "geoPosition", "lastContact"]
        assert got["icao"] == s.icao and got["callsign"] == s.callsign.decode() and got["altitude"] == s.altitude
        if s.has_position:
            n_pos += 1
            assert list(got["geoPosition"]) == ["latitude", "longitude"]
            assert abs(got["geoPosition"]["latitude"] - s.latitude) <= TOL
            assert abs(got["geoPosition"]["longitude"] - s.longitude) <= TOL
        else:
            assert got["geoPosition"] is None
        want_contact = 0.0 if math.isnan(s.last_contact) else s.last_contact
        assert isinstance(got["lastContact"], int)
        # whole seconds of a time that may differ by TOL from the oracle's
        assert got["lastContact"] in (int(want_contact - TOL), int(want_contact + TOL))
    assert n_pos >= 100
