"""Per-aircraft signal levels on the device (adsb_track_*_levels_reserve / update_levels / fetch_levels, the fused
levels of a bank): every comparison is of raw bytes, against tests/track_levels_model.py for the level records and
against a twin store fed by plain update for the points and records.  The frame lists come from
tests/traffic.random_traffic at 2 MSPS; the levels the merge is fed are synthetic, since it does not care where they
came from; the launch test feeds it the launch's own."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from tests import levels_model
from tests import track_levels_model as M
from tests.traffic import ident_frame, position_frame, random_traffic

pytestmark = pytest.mark.gpu
SPS = 0.5e-6
EMPTY = M.records({}, [0])[0].tobytes()


def _frames(items):
    """[(offset, 14 frame bytes)] -> FRAME_DTYPE array."""
    out = np.zeros(len(items), dtype=A.FRAME_DTYPE)
    for k, (off, b) in enumerate(items):
        out[k]["offset"] = off
        out[k]["bytes"] = np.frombuffer(bytes(b), dtype=np.uint8)
        out[k]["fixed_bit"] = 0xFF
    return out


def _traffic(oracle, seed, n_aircraft, n_frames, span_s=60.0):
    return _frames([(round(t / SPS), fr) for t, fr in random_traffic(oracle, seed=seed, n_aircraft=n_aircraft,
                                                                      n_frames=n_frames, span_s=span_s)])


def _levels(n, seed):
    """Synthetic adsb_frame_level records: sums below 2^38, about one in five invalid."""
    rng = np.random.default_rng(seed)
    lv = np.zeros(n, dtype=A.LEVEL_DTYPE)
    lv["signal_sum"] = rng.integers(0, 1 << 38, size=n, dtype=np.uint64)
    lv["noise_sum"] = rng.integers(0, 1 << 38, size=n, dtype=np.uint64)
    lv["peak"] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    lv["pulse_min"] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    lv["quiet_max"] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    lv["weak_bits"] = rng.integers(0, 113, size=n)
    lv["flags"] = (rng.random(n) >= 0.2).astype(np.uint16)
    return lv


def _level(signal, noise=0, peak=0, weak=0, flags=1):
    lv = np.zeros(1, dtype=A.LEVEL_DTYPE)
    lv["signal_sum"], lv["noise_sum"], lv["peak"], lv["weak_bits"], lv["flags"] = signal, noise, peak, weak, flags
    return lv


def _same(got, want):
    assert got.dtype.itemsize == want.dtype.itemsize and len(got) == len(want), (len(got), len(want))
    if got.tobytes() != want.tobytes():                      # say where, then fail
        for k in range(len(got)):
            assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])


def _check(table, state):
    """table.levels() == the model's records, aligned with aircraft()."""
    recs, _ = table.aircraft()
    got = table.levels()
    assert got.dtype == A.AIRCRAFT_LEVEL_DTYPE and len(got) == len(recs)
    _same(got, M.records(state, recs["icao"]))
    return recs, got


def _twin_equal(table, twin):
    assert table.points().tobytes() == twin.points().tobytes()
    (a, fa), (b, fb) = table.aircraft(), twin.aircraft()
    assert a.tobytes() == b.tobytes() and fa == fb
    assert table.last_heard().tobytes() == twin.last_heard().tobytes()
    assert table.velocity().tobytes() == twin.velocity().tobytes()


@contextlib.contextmanager
def _tables(d, **kw):
    """A table with a levels reserve and a twin without one, both closed before the ctx on every path."""
    kw.setdefault("max_frames", 1 << 12)
    with A.TrackTable(d, seconds_per_sample=SPS, **kw) as table, A.TrackTable(d, seconds_per_sample=SPS, **kw) as twin:
        table.levels_reserve()
        yield table, twin


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()


# ---- 1: one update and every cutting of it equal the model; points and records equal a twin fed by update ------------
def test_equals_the_model_whatever_the_cut(gpu, oracle):
    frames = _traffic(oracle, seed=41, n_aircraft=12, n_frames=600)
    levels = _levels(len(frames), seed=42)
    base = 12_345
    want = M.apply({}, frames, levels, base, SPS)
    assert len(want) == 12 and (levels["flags"] == 0).sum() > 60
    rng = np.random.default_rng(43)
    random_cut = sorted(int(x) for x in rng.choice(np.arange(1, 600), size=9, replace=False))
    cuts = {"whole": [], "random": random_cut}
    for size in (1, 7, 64, 65, 300):
        cuts[size] = list(range(size, 600, size))
    first = None
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        with _tables(d) as (table, twin):
            for name, cut in cuts.items():
                table.reset()
                twin.reset()
                edges = [0] + cut + [600]
                for a, b in zip(edges[:-1], edges[1:]):
                    table.update(frames[a:b], base, levels=levels[a:b])
                    twin.update(frames[a:b], base)
                    assert table.points().tobytes() == twin.points().tobytes(), (name, a)
                _twin_equal(table, twin)
                recs, got = _check(table, want)
                assert len(recs) == 12, name
                first = got.tobytes() if first is None else first
                assert got.tobytes() == first, name
            assert (got["n_levels"] > 10).all() and not np.isnan(got["last_time"]).any()


# ---- 2: segment and list boundaries ------------------------------------------------------------------------------------
def test_boundaries(gpu, oracle):
    others = _traffic(oracle, seed=51, n_aircraft=10, n_frames=300)
    icaos = sorted(set(int(x) for x in M.frame_icaos(others)))
    long_icao = (icaos[4] + icaos[5]) // 2                          # in the middle of the sorted list
    mute_icao = (icaos[7] + icaos[8]) // 2                          # every frame of it invalid
    assert long_icao not in icaos and mute_icao not in icaos
    t0 = int(others[150]["offset"]) + 1
    long_run = _frames([(t0 + 3 * k, position_frame(oracle, long_icao, k & 1, 1000 + k, 2000 + k)) for k in range(700)])
    mute = _frames([(t0 + 5000 + 7 * k, ident_frame(oracle, mute_icao, [1 + k % 26] * 8)) for k in range(9)])
    lo = _frames([(t0 + 1, position_frame(oracle, 0x000000, 0, 5, 6))])       # first sorted position, one frame
    hi = _frames([(t0 + 2, ident_frame(oracle, 0xFFFFFF, [3] * 8))])          # last sorted position, one frame
    frames = np.concatenate([others, long_run, mute, lo, hi])
    order = np.argsort(frames["offset"], kind="stable")
    frames = frames[order]
    levels = _levels(len(frames), seed=52)
    fi = M.frame_icaos(frames)
    levels["flags"][fi == mute_icao] = 0
    levels["flags"][(fi == 0) | (fi == 0xFFFFFF)] = 1
    want = M.apply({}, frames, levels, 0, SPS)
    assert want[long_icao]["n_levels"] > 500 and mute_icao not in want
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        with _tables(d) as (table, twin):
            table.update(frames, levels=levels)
            twin.update(frames)
            _twin_equal(table, twin)
            recs, got = _check(table, want)
            assert len(recs) == 14 and recs["icao"][0] == 0 and recs["icao"][-1] == 0xFFFFFF
            assert got[0]["n_levels"] == 1 == got[-1]["n_levels"]
            k = list(recs["icao"]).index(mute_icao)
            assert got[k].tobytes() == EMPTY and math.isnan(got[k]["last_time"]) and recs[k]["n_frames"] == 9
            # two runs give the same bytes
            table.reset()
            table.update(frames, levels=levels)
            assert table.levels().tobytes() == got.tobytes()
            # n = 1, then n = 0
            table.reset()
            table.update(frames[:1], levels=levels[:1])
            _check(table, M.apply({}, frames[:1], levels[:1], 0, SPS))
            before = table.levels().tobytes()
            table.update(frames[:0], levels=levels[:0])
            assert table.levels().tobytes() == before and len(table.points()) == 0
            table.reset()
            table.update(frames[:0], levels=levels[:0])
            assert len(table.levels()) == 0


# ---- 3: equal offsets are applied in list order -----------------------------------------------------------------------
def test_equal_offsets_the_later_in_list_order_is_last(gpu, oracle):
    icao = 0x4B1234
    frames = _frames([(1000, position_frame(oracle, icao, 0, 11, 12)), (1000, position_frame(oracle, 0x4B0000, 0, 1, 2)),
                      (1000, position_frame(oracle, icao, 1, 13, 14)), (1000, ident_frame(oracle, icao, [2] * 8))])
    levels = np.concatenate([_level(500, 50, 9), _level(1, 1, 1), _level(300, 30, 4), _level(400, 40, 2, flags=0)])
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        with _tables(d) as (table, twin):
            table.update(frames, levels=levels)
            recs, got = _check(table, M.apply({}, frames, levels, 0, SPS))
            mine = got[list(recs["icao"]).index(icao)]
            assert (mine["last_signal_sum"], mine["last_noise_sum"]) == (300, 30)
            assert (mine["signal_total"], mine["max_signal_sum"], mine["peak"], mine["n_levels"]) == (800, 500, 9, 2)
            assert mine["last_time"] == 1000 * SPS


# ---- 4: saturation ------------------------------------------------------------------------------------------------------
def test_saturation(gpu, oracle):
    icao = 0x4B1234
    frames = _frames([(100 * k, position_frame(oracle, icao, k & 1, 11, 12)) for k in range(4)])
    big = np.concatenate([_level(1 << 63, M.U64, 7, 65535), _level(1 << 63, 5, 8, 65535)])
    more = np.concatenate([_level(12345, 1, 2, 3), _level(1 << 62, 0, 1, 0)])
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        with _tables(d) as (table, twin):
            table.update(frames[:2], levels=big)
            state = M.apply({}, frames[:2], big, 0, SPS)
            _, got = _check(table, state)
            assert got[0]["signal_total"] == M.U64 == got[0]["noise_total"] and got[0]["max_signal_sum"] == 1 << 63
            table.update(frames[2:3], levels=more[:1])                  # a third update leaves it there
            _, got = _check(table, M.apply(state, frames[2:3], more[:1], 0, SPS))
            assert got[0]["signal_total"] == M.U64 and got[0]["noise_total"] == M.U64
            assert (got[0]["max_signal_sum"], got[0]["last_signal_sum"], got[0]["n_levels"]) == (1 << 63, 12345, 3)
            table.update(frames[3:], levels=more[1:])
            _, got = _check(table, M.apply(state, frames[3:], more[1:], 0, SPS))
            assert (got[0]["signal_total"], got[0]["last_signal_sum"], got[0]["max_signal_sum"]) == (M.U64, 1 << 62, 1 << 63)
            assert got[0]["weak_bits_total"] == 2 * 65535 + 3


# ---- 5: a full table --------------------------------------------------------------------------------------------------
def test_full_table_turned_away_aircraft_contribute_nothing(gpu, oracle):
    frames = _traffic(oracle, seed=61, n_aircraft=6, n_frames=240)
    levels = _levels(len(frames), seed=62)
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        with _tables(d, max_aircraft=4) as (table, twin):
            state = {}
            for a, b in ((0, 100), (100, 240)):
                table.update(frames[a:b], levels=levels[a:b])
                twin.update(frames[a:b])
                away = (twin.points()["flags"] & A.ADSB_TRACK_UNTRACKED) != 0
                M.apply(state, frames[a:b], levels[a:b], 0, SPS, untracked=away)
                _twin_equal(table, twin)
            assert away.sum() > 20 and table.aircraft()[1] == A.ADSB_TRACK_TABLE_FULL
            recs, got = _check(table, state)
            assert len(recs) == 4 and len(state) == 4 and (got["n_levels"] > 10).all()


# ---- 6: expire and reset ---------------------------------------------------------------------------------------------
def test_expire_and_reset(gpu, oracle):
    frames = _traffic(oracle, seed=71, n_aircraft=14, n_frames=500)
    levels = _levels(len(frames), seed=72)
    fi = M.frame_icaos(frames)
    icaos = sorted(set(int(x) for x in fi))
    quiet = set(icaos[1::3])                                         # silent in the second half: evicted
    keep = np.array([k < 250 or int(fi[k]) not in quiet for k in range(500)])
    frames, levels, fi = frames[keep], levels[keep], fi[keep]
    half = int(keep[:250].sum())
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        with _tables(d) as (table, twin):
            table.update(frames[:half], levels=levels[:half])
            table.update(frames[half:], levels=levels[half:])
            state = M.apply({}, frames, levels, 0, SPS)
            recs, before = _check(table, state)
            cut = float(frames[half]["offset"]) * SPS
            table.expire(cut)
            after_recs, after = _check(table, state)                   # survivors: unchanged and still aligned
            gone = set(int(x) for x in recs["icao"]) - set(int(x) for x in after_recs["icao"])
            assert gone == quiet and len(after_recs) == len(icaos) - len(quiet)
            for icao in gone:
                del state[icao]
            # an evicted aircraft heard again starts empty (one frame of it, with an invalid level), then counts anew
            back = sorted(gone)[0]
            again = frames[:half][fi[:half] == back][:3].copy()
            again["offset"] += np.uint64(int(frames[-1]["offset"]) + 10)
            lv = _levels(3, seed=73)
            lv["flags"] = [0, 1, 1]
            table.update(again[:1], levels=lv[:1])
            recs, got = _check(table, state)
            k = list(recs["icao"]).index(back)
            assert got[k].tobytes() == EMPTY and recs[k]["n_frames"] == 1
            table.update(again[1:], levels=lv[1:])
            _, got = _check(table, M.apply(state, again[1:], lv[1:], 0, SPS))
            assert got[k]["n_levels"] == 2
            # reset: only the update after it counts
            table.reset()
            table.update(frames[half:], levels=levels[half:])
            _check(table, M.apply({}, frames[half:], levels[half:], 0, SPS))


# ---- 7: opt-in ---------------------------------------------------------------------------------------------------------
def test_opt_in(gpu, oracle):
    L = _lib.load()
    frames = _traffic(oracle, seed=81, n_aircraft=8, n_frames=200)
    levels = _levels(len(frames), seed=82)
    out = (_lib.AdsbAircraftLevel * 16)()
    n, dev = C.c_size_t(), C.c_void_p()
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        with _tables(d, max_frames=256) as (table, plain):
            # an unreserved table
            h = plain._h
            assert L.adsb_track_table_update_levels(h, frames.ctypes.data, levels.ctypes.data, 10, 0) == A.ADSB_E_STATE
            assert L.adsb_track_table_fetch_levels(h, out, 16, C.byref(n)) == A.ADSB_E_STATE
            assert L.adsb_track_table_levels_device(h, C.byref(dev)) == A.ADSB_E_STATE
            assert len(plain.aircraft()[0]) == 0
            # a reserved one: arguments
            h = table._h
            assert L.adsb_track_table_update_levels(h, frames.ctypes.data, None, 10, 0) == A.ADSB_E_ARG
            assert L.adsb_track_table_update_levels(h, None, levels.ctypes.data, 10, 0) == A.ADSB_E_ARG
            assert L.adsb_track_table_update_levels(h, frames.ctypes.data, levels.ctypes.data, 257, 0) == A.ADSB_E_CAPACITY
            assert L.adsb_track_table_update_levels(h, None, None, 0, 0) == A.ADSB_OK
            assert L.adsb_track_table_fetch_levels(h, None, 4, C.byref(n)) == A.ADSB_E_ARG
            table.levels_reserve()                                      # a second reserve changes nothing
            assert table.levels_device() == table.levels_device() != 0
            # a plain update on a reserved table leaves the level records alone
            table.update(frames[:100], levels=levels[:100])
            state = M.apply({}, frames[:100], levels[:100], 0, SPS)
            before_recs, before = _check(table, state)
            table.update(frames[100:])
            plain.update(frames[:100])
            plain.update(frames[100:])
            _twin_equal(table, plain)
            recs, got = _check(table, state)
            where = {int(x): k for k, x in enumerate(recs["icao"])}
            assert all(got[where[int(x)]].tobytes() == before[k].tobytes() for k, x in enumerate(before_recs["icao"]))
            # fetch_levels: *n = records held even when fewer are asked for
            assert L.adsb_track_table_fetch_levels(h, out, 3, C.byref(n)) == A.ADSB_OK and n.value == len(recs) > 3
            assert bytes(out)[:3 * 64] == got[:3].tobytes()
            # a reserve on a table that already holds aircraft: empty until their next counted frame
            plain.levels_reserve()
            lv = plain.levels()
            assert len(lv) == len(recs) and all(r.tobytes() == EMPTY for r in lv)
            plain.update(frames[:60], levels=levels[:60])
            _check(plain, M.apply({}, frames[:60], levels[:60], 0, SPS))


# ---- 8: a bank's receiver equals a table of its own --------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device", "frames_host_levels_device"])
def test_bank_equals_tables(gpu, oracle, where):
    R = 3
    shared = _traffic(oracle, seed=91, n_aircraft=10, n_frames=700)       # the same ICAOs active on all receivers
    rng = np.random.default_rng(92)
    hears = [np.nonzero(rng.random(len(shared)) < 0.7)[0] for _ in range(R)]
    lists = [shared[h] for h in hears]
    levels = [_levels(len(x), seed=93 + r) for r, x in enumerate(lists)]
    bases = [7, 1_000_003, 0]
    halves = [len(x) // 2 for x in lists]
    keep = []
    # (every store is closed before its ctx on every path, a failing assertion included: the ctx must outlive them)
    with A.AdsbDemod(max_samples=1024, max_out=16) as d, \
            A.TrackBank(d, R, max_frames=1 << 12, seconds_per_sample=SPS) as bank, contextlib.ExitStack() as stack:
        bank.levels_reserve()
        tables = [stack.enter_context(A.TrackTable(d, max_frames=1 << 12, seconds_per_sample=SPS)) for _ in range(R)]
        for t in tables:
            t.levels_reserve()
        for part in (0, 1):
            cut = [(slice(0, h) if part == 0 else slice(h, None)) for h in halves]
            fr = np.concatenate([x[c] for x, c in zip(lists, cut)])
            lv = np.concatenate([x[c] for x, c in zip(levels, cut)])
            counts = [len(x[c]) for x, c in zip(lists, cut)]
            if where == "host":
                bank.update(fr, counts, bases, levels=lv)
            else:
                dl = _dev(lv)
                keep.append(dl)
                if where == "device":
                    df = _dev(fr)
                    keep.append(df)
                    bank.update_device(df.data_ptr(), len(fr), counts, bases, levels_ptr=dl.data_ptr())
                else:
                    bank.update_device(fr.ctypes.data, len(fr), counts, bases, levels_ptr=dl.data_ptr())
            for r in range(R):
                tables[r].update(lists[r][cut[r]], bases[r], levels=levels[r][cut[r]])
            pts, pos = bank.points(), 0
            for r in range(R):
                assert pts[pos:pos + counts[r]].tobytes() == tables[r].points().tobytes()
                pos += counts[r]
        recs, got = bank.aircraft()[0], bank.levels()
        assert len(got) == R
        for r in range(R):
            assert recs[r].tobytes() == tables[r].aircraft()[0].tobytes()
            _same(got[r], tables[r].levels())
            _same(got[r], M.records(M.apply({}, lists[r], levels[r], bases[r], SPS), recs[r]["icao"]))
            assert len(got[r]) == 10 and (got[r]["n_levels"] > 10).all()
        assert got[0].tobytes() != got[1].tobytes()
        del keep


# ---- 9: from a launch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "rebuilt"])
def test_from_a_launch(gpu, dense):
    import torch
    nch, n = 3, 200_000
    stride = n + 8
    cfg = A.synth_default(seed=101, slot_len=700)
    chans = [A.synth_fill_host(cfg, A.ADSB_SAMPLE_I8, c, 0, n).copy() for c in range(nch)]
    if dense:
        chans[1][30_000:52_000] = (3, 4)      # constant: one frame per offset, tiles far over their 32 slots
        chans[1][120_000:120_300] = 0
    buf = np.zeros((nch * stride, 2), dtype=np.int8)
    for c in range(nch):
        buf[c * stride:c * stride + n] = chans[c]
    bases = [0, 5_000_000, 11]
    with A.AdsbDemod(max_samples=n, max_out=1 << 16, max_channels=nch, host_staging=False) as d, \
            A.TrackBank(d, nch, max_aircraft=1 << 12, max_frames=1 << 16, seconds_per_sample=SPS) as bank:
        with pytest.raises(A.AdsbError) as e:
            bank.update_launch(levels=True)                         # no reserve
        assert e.value.code == A.ADSB_E_STATE
        bank.levels_reserve()
        with pytest.raises(A.AdsbError) as e:
            bank.update_launch(levels=True)                         # no launch yet
        assert e.value.code == A.ADSB_E_STATE
        d.pool_limit(dense)
        dev = torch.from_numpy(buf).cuda()
        d.demod_device_async(dev.data_ptr(), n, n_channels=nch, channel_stride=stride)
        if dense:
            d.levels_async()      # enqueued on the list with holes: update_launch's wait rebuilds the list, and must
        bank.update_launch(bases, levels=True)                      # compute the levels again for the rebuilt one
        d.pool_limit(False)
        frames, counts, total, flags = d.fetch()
        assert flags == 0 and sum(counts) == len(frames) == total and min(counts) > 100
        if dense:
            assert counts[1] > 20_000
        recs, got = bank.aircraft()[0], bank.levels()
        pos = 0
        for c in range(nch):
            part = frames[pos:pos + counts[c]]
            pos += counts[c]
            lv = levels_model.levels(chans[c], part)
            assert (lv["flags"] == 1).all()
            want = M.apply({}, part, lv, bases[c], SPS)
            _same(got[c], M.records(want, recs[c]["icao"]))
            assert int(got[c]["n_levels"].sum()) == counts[c] == int(recs[c]["n_frames"].sum())
        del dev


# ---- 10: fused levels ---------------------------------------------------------------------------------------------------
def _hip_runtime():
    """The HIP runtime this process already holds (the one libadsb_hip.so is bound to), for a plain hipMemcpy."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path:
            return C.CDLL(path)
    raise RuntimeError("no HIP runtime mapped")


def _fused_model(bank, since=-math.inf):
    recs, _ = bank.aircraft()
    return M.fuse([x["icao"] for x in recs], bank.last_heard(), bank.levels(), since)


def test_fused_levels(gpu, oracle):
    R = 4
    shared = _traffic(oracle, seed=111, n_aircraft=16, n_frames=900)
    fi = M.frame_icaos(shared)
    icaos = sorted(set(int(x) for x in fi))
    rng = np.random.default_rng(112)
    lists, levels = [], []
    for r in range(R):
        hear = rng.random(len(shared)) < 0.6
        hear &= ~np.isin(fi, icaos[r::5])                             # some aircraft are not heard by every receiver
        lists.append(shared[hear])
        lv = _levels(int(hear.sum()), seed=113 + r)
        lv["flags"][np.isin(fi[hear], icaos[(r + 2) % 4::4])] = 0    # ... and some held with no level at all
        levels.append(lv)
    bases = [0, 100, 200_000_000, 3]                                  # receiver 2's clock is 100 s ahead
    fr, lv, counts = np.concatenate(lists), np.concatenate(levels), [len(x) for x in lists]
    with A.AdsbDemod(max_samples=1024, max_out=16) as d, \
            A.TrackBank(d, R, max_aircraft=64, max_frames=1 << 12, seconds_per_sample=SPS) as bank, \
            A.TrackBank(d, R, max_aircraft=64, max_frames=1 << 12, seconds_per_sample=SPS) as twin, \
            A.TrackBank(d, R, max_aircraft=64, max_frames=1 << 12, seconds_per_sample=SPS) as plain:
        # ADSB_E_STATE without either reserve
        bank.fuse_reserve(0)
        bank.update(fr, counts, bases)
        bank.fuse_async()
        with pytest.raises(A.AdsbError) as e:
            bank.fused_levels()                                       # no levels reserve
        assert e.value.code == A.ADSB_E_STATE
        twin.levels_reserve()
        with pytest.raises(A.AdsbError) as e:
            twin.fused_levels()                                       # no fuse reserve, no fuse
        assert e.value.code == A.ADSB_E_STATE
        bank.levels_reserve()                                         # the second reserve makes the output array
        with pytest.raises(A.AdsbError) as e:
            bank.fused_levels()                                       # the last fuse computed none
        assert e.value.code == A.ADSB_E_STATE
        bank.reset()
        bank.update(fr, counts, bases, levels=lv)
        twin.fuse_reserve(0)                                          # the other order of the two reserves
        twin.update(fr, counts, bases, levels=lv)
        plain.update(fr, counts, bases)
        for b in (bank, twin):
            fused, total, flags = b.fuse()
            want = _fused_model(b)
            got = b.fused_levels()
            assert got.dtype == A.FUSED_LEVEL_DTYPE and len(got) == len(fused) == total == len(icaos)
            _same(got, want)
            # the 128-byte fused records are what a bank without a levels reserve gives
            assert fused.tobytes() == plain.fuse()[0].tobytes()
            assert (fused["reserved"] == 0).all()
        assert len(set(got["strongest_receiver"])) >= 2 and (got["level_receivers"] < R).any()
        # two fuses give identical bytes
        bank.fuse_async()
        assert bank.fused_levels().tobytes() == got.tobytes()
        # since excludes every receiver but 2, whose clock is ahead of the others' whole span
        since = 200_000_000 * SPS
        fused, total, _ = bank.fuse(since)
        got2 = bank.fused_levels()
        _same(got2, _fused_model(bank, since))
        assert 0 < len(got2) == total == len(bank.aircraft()[0][2]) < len(icaos)
        assert set(got2["strongest_receiver"]) <= {2, M.NONE} and (got2["level_receivers"] <= 1).all()
        # truncation: only the written records get a level record
        fused, total, flags = bank.fuse(max_fused=5)
        got3 = bank.fused_levels()
        assert flags == A.ADSB_TRACK_FUSED_TRUNCATED and total == len(icaos) and len(fused) == 5
        _same(got3, _fused_model(bank)[:5])
        n = C.c_size_t()
        out = (_lib.AdsbFusedLevel * 2)()
        assert _lib.load().adsb_track_bank_fetch_fused_levels(bank._h, out, 2, C.byref(n)) == A.ADSB_OK
        assert n.value == 5 and bytes(out) == got3[:2].tobytes()
        assert _lib.load().adsb_track_bank_fetch_fused_levels(bank._h, None, 2, C.byref(n)) == A.ADSB_E_ARG


def test_fused_strongest_is_exact(gpu, oracle):
    """Means compared by cross-multiplication: exact ties go to the lowest receiver, and a difference far below what a
    double resolves still decides.  The small cases come through update; counts of 2^31 cannot, so those level records
    are written into the bank's side array (levels_device; one update admits in ascending ICAO, so place = receiver x
    max_aircraft + the aircraft's rank)."""
    R, MAXA = 3, 8
    icaos = [0x400001, 0x400002, 0x400003, 0x400004, 0x400005]
    fr, lv = [], []
    per = {  # icao -> per receiver, the signal_sums of its frames
        0x400001: ([4, 0], [2], [1]),                  # 4/2 = 2/1 > 1: tie, the lowest receiver (0)
        0x400002: ([1], [2], [3, 1]),                  # 1, 2, 4/2: tie of 1 and 2 -> 1
        0x400003: ([3, 4], [10, 0, 1], [7, 0]),        # 7/2, 11/3, 7/2: 11/3 is the greatest -> 1
        0x400004: ([(1 << 60) + 2] * 4, [(1 << 60) + 3] * 3, [1]),     # 2^60 + 2 against 2^60 + 3: one double
        0x400005: ([5], [5], [5]),                     # rewritten below
    }
    counts = []
    for r in range(R):
        items, rows = [], []
        for icao in icaos:
            for k, s in enumerate(per[icao][r]):
                items.append((1000 * (icao & 0xF) + k, position_frame(oracle, icao, k & 1, 11, 12)))
                rows.append(_level(s, 1, 1))
        order = sorted(range(len(items)), key=lambda k: items[k][0])
        fr.append(_frames([items[k] for k in order]))
        lv.append(np.concatenate([rows[k] for k in order]))
        counts.append(len(items))
    with A.AdsbDemod(max_samples=1024, max_out=16) as d, \
            A.TrackBank(d, R, max_aircraft=MAXA, max_frames=256, seconds_per_sample=SPS) as bank:
        bank.levels_reserve()
        bank.fuse_reserve(0)
        bank.update(np.concatenate(fr), counts, levels=np.concatenate(lv))
        bank.fuse_async()
        got = bank.fused_levels()
        _same(got, _fused_model(bank))
        assert list(got["strongest_receiver"][:4]) == [0, 1, 1, 1]
        assert float((1 << 60) + 2) == float((1 << 60) + 3)
        # totals near 2^62 with counts 2^31 - 1 and 2^31: the two means are one double
        assert float(1 << 62) / float((1 << 31) - 1) == float((1 << 62) + (1 << 31)) / float(1 << 31)
        hip = _hip_runtime()
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipMemcpy.restype = C.c_int
        hip.hipDeviceSynchronize.restype = C.c_int
        assert hip.hipDeviceSynchronize() == 0
        base = bank.levels_device()
        cases = [  # (receiver 0, receiver 1, receiver 2) as (signal_total, n_levels) -> strongest
            (((1 << 62) + (1 << 31), 1 << 31), ((1 << 62), (1 << 31) - 1), (1, 1), 1),     # greater by 1 / (2^31 - 1)
            (((1 << 62), (1 << 31) - 1), ((1 << 62) + (1 << 31), 1 << 31), (1, 1), 0),
            (((1 << 62) + (1 << 31), 1 << 31), ((1 << 62) - 1, (1 << 31) - 1), (1, 1), 0), # an exact tie
            (((1 << 62) - 1, (1 << 31) - 1), (1, 1), ((1 << 62) + (1 << 31), 1 << 31), 0), # the same tie, mirrored
            ((M.U64, M.U32), (M.U64 - 1, M.U32 - 1), (M.U64, M.U32 - 1), 2),               # 96-bit products
        ]
        slot = icaos.index(0x400005)
        for *recs, want_r in cases:
            for r, (total, n) in enumerate(recs):
                rec = M.records({}, [0])
                rec["signal_total"], rec["n_levels"], rec["last_time"], rec["peak"] = total, n, 1.5, r + 1
                place = base + 64 * (r * MAXA + slot)
                assert hip.hipMemcpy(place, rec.ctypes.data, 64, 1) == 0               # hipMemcpyHostToDevice
            bank.fuse_async()
            got = bank.fused_levels()
            _same(got, _fused_model(bank))
            assert got[slot]["strongest_receiver"] == want_r and got[slot]["strongest"]["peak"] == want_r + 1, recs
            assert got[slot]["n_levels"] == sum(n for _, n in recs) and got[slot]["level_receivers"] == 3


# ---- 11: tools/replay.py --aircraft --levels --------------------------------------------------------------------------
def test_replay_aircraft_levels(gpu, oracle, tmp_path):
    """--aircraft --levels appends RSSI and SNR to the rows --aircraft prints: each aircraft's mean signal power in dBFS
    over its 116 x n_levels pulse samples and that minus its mean noise power, from the model's totals in Python floats."""
    import importlib.util
    import os
    import subprocess
    import sys

    from tests.golden.make_golden import REF_FRAMES, modulate, place
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    chunk = 20_000
    items = [(chunk * (k // 3) + 300 + 2113 * (k % 3), modulate(bytes.fromhex(REF_FRAMES[k % 7]), (800 + 100 * k, 30), None))
             for k in range(12)]
    iq = place(chunk * 5, items, np.int16, floor=3, seed=5)        # (the fifth, frameless chunk is never sent)
    path = tmp_path / "capture.c16"
    iq.astype("<i2").tofile(path)
    frames = _frames([(o, bytes.fromhex(REF_FRAMES[k % 7])) for k, (o, _) in enumerate(items)])
    state = M.apply({}, frames, levels_model.levels(iq, frames), 0, SPS)
    assert 2 <= len(state) <= 7 and sum(a["n_levels"] for a in state.values()) == 12

    def db(total, n, full=2.0 ** 31):
        return -math.inf if total == 0 else 10 * math.log10(total / n / full)

    tool = os.path.join(root, "tools", "replay.py")
    spec = importlib.util.spec_from_file_location("replay_tool", tool)
    replay = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(replay)
    with A.AdsbDemod(sample_type=A.ADSB_SAMPLE_I16, max_samples=1024, max_out=64, host_staging=False) as d:
        plain = replay.aircraft_table(d, frames, 4 * chunk)         # what --aircraft alone prints
    assert plain.startswith("ICAO\tCallsign\tAltitude\tLatitude\tLongitude\tVelocity\tAge\n")
    want = ""
    for k, line in enumerate(plain.splitlines()):
        if k == 0:
            want += line + "\tRSSI\tSNR\n"
            continue
        a = state[int(line.split("\t")[0], 16)]
        sig, noise = db(a["signal_total"], 116 * a["n_levels"]), db(a["noise_total"], 124 * a["n_levels"])
        want += line + f"\t{sig:.1f}\t{sig - noise:.1f}\n"
    got = subprocess.run([sys.executable, tool, str(path), "--aircraft", "--levels"], capture_output=True, text=True,
                         timeout=300, check=True).stdout
    assert got == want and got.count("\n") == 1 + len(state)
    assert replay.level_columns(A.ADSB_SAMPLE_I16, M.records({}, [1])[0]) == ["n/a", "n/a"]
    big = M.records({1: dict(M.empty(), signal_total=M.U64, noise_total=1 << 40, n_levels=M.U32)}, [1])[0]
    sig, noise = db(M.U64, 116 * M.U32, 32768.0), db(1 << 40, 124 * M.U32, 32768.0)     # 116 x n_levels needs 39 bits
    assert replay.level_columns(A.ADSB_SAMPLE_I8, big) == [f"{sig:.1f}", f"{sig - noise:.1f}"]
