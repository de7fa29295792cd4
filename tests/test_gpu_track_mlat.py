"""Multilaterated positions per aircraft on the device (adsb_track_table_mlat_reserve / update_mlat / fetch_mlat /
fetch_frame_mlat) against the CPU mirror (adsb_host_track_mlat_of) plus a plain Python merge, with fixes the tests make
themselves: the merge does not care where a fix came from.  Lists are at most 5300 frames.

Tolerance where two math libraries meet: device and mirror compile one text with contraction off, so what can differ is
the last bit of sin / cos / asin in f64, some 1e-16 of the haversine's terms and below a nanometre on the ground; after
the one rounding to f32 the two values are equal or neighbours.  disagreement_m is therefore compared within ONE f32 STEP
of the mirror's value (0.03 m at 333 km, 5e-7 m at 5 m); every other field bit for bit.  Planted disagreements lie below
50 m or above 2 km against the 1000 m limit, so DISAGREE and n_disagree are compared exactly."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from tests import fix_model as F
from tests import track_mlat_cases as K
from tests import track_mlat_model as M

pytestmark = pytest.mark.gpu
SPS = 0.5e-6
LIMIT = 1000.0
BASE = 1_000_000
EMPTY = M.empty().tobytes()
TOL = M.f32_step


class Traffic:
    """A frame list with a fix per frame, and what the CPU mirror makes of each frame on its own."""

    def __init__(self, items, fixes, base=BASE):
        self.frames = M.frames_array(items, A.FRAME_DTYPE)
        self.fixes = np.ascontiguousarray(fixes, dtype=A.MLAT_FIX_DTYPE)
        self.base = base
        self.icaos = F.frame_icaos(self.frames)
        self.single = np.zeros(len(items), dtype=M.MODEL_DTYPE)
        self.frame = np.zeros(len(items), dtype=M.FRAME_DTYPE)
        self.frame["icao"] = self.icaos
        for k in range(len(items)):
            time = float(base + int(self.frames["offset"][k])) * SPS
            rec, flags, dis = A.host_track_mlat_of(LIMIT, self.frames["bytes"][k].tobytes(), self.fixes[k], time)
            self.single[k] = np.array([rec]).view(M.MODEL_DTYPE)[0]
            self.frame[k]["flags"], self.frame[k]["disagreement_m"] = flags, dis

    def state(self, lo=0, hi=None, state=None, untracked=None):
        """{icao: record} after the frames [lo, hi) in list order: the mirror's single-frame records combined by the
        header's rules (saturating add, max, newest by position)."""
        state = {} if state is None else state
        for k in range(lo, len(self.frames) if hi is None else hi):
            if untracked is not None and untracked[k - lo]:
                continue
            icao = int(self.icaos[k])
            state[icao] = _combine(state.get(icao, M.empty()), self.single[k])
        return state

    def frame_records(self, lo=0, hi=None, untracked=None):
        out = self.frame[lo:hi].copy()
        if untracked is not None:
            for name in ("flags", "disagreement_m"):
                out[name][untracked] = 0
        return out


def _combine(a, one):
    a = a.copy()
    for name in ("n_attempted", "n_valid", "n_checked", "n_disagree"):
        a[name] = min(int(a[name]) + int(one[name]), M.U32)
    if one["flags"] & M.VALID:
        for name in ("time", "latitude", "longitude", "height_m", "residual_rms_m", "pdop", "n_used"):
            a[name] = one[name]
        a["flags"] = (int(a["flags"]) & M.CHECKED) | (int(one["flags"]) & (M.VALID | M.ALTITUDE))
    if one["flags"] & M.CHECKED:
        a["last_disagreement_m"] = one["last_disagreement_m"]
        a["max_disagreement_m"] = max(a["max_disagreement_m"], one["max_disagreement_m"])
        a["flags"] = int(a["flags"]) | M.CHECKED
    return a


def _check(table, state, what=""):
    """table.mlat() == the expected records, aligned with aircraft()."""
    recs, _ = table.aircraft()
    got = table.mlat()
    assert got.dtype == A.AIRCRAFT_MLAT_DTYPE and len(got) == len(recs)
    M.assert_records_equal(got.view(M.MODEL_DTYPE), M.records(state, recs["icao"]), TOL, what)
    return recs, got


@contextlib.contextmanager
def _table(max_frames=1 << 13, limit=LIMIT, **kw):
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        with A.TrackTable(d, seconds_per_sample=SPS, max_frames=max_frames, **kw) as table:
            if limit is not None:
                table.mlat_reserve(limit)
            yield table


@pytest.fixture(scope="module")
def mixed():
    """4097 frames of 60 aircraft: the list most tests cut pieces from."""
    rng = np.random.default_rng(3)
    icaos = rng.choice(np.arange(0x400000, 0x800000), size=60, replace=False)
    return Traffic(*M.traffic(7, 4097, icaos))


# ---- (a) the smallest shapes where the scan and the merge can go wrong -------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4097])
def test_list_lengths(gpu, mixed, n):
    with _table() as table:
        table.update(mixed.frames[:n], mixed.base, mlat=mixed.fixes[:n])
        _, got = _check(table, mixed.state(0, n), n)
        fm = table.frame_mlat()
        assert fm.dtype == A.FRAME_MLAT_DTYPE and len(fm) == n
        M.assert_frames_equal(fm.view(M.FRAME_DTYPE), mixed.frame_records(0, n), TOL, n)
        if n == 4097:
            assert (got["n_disagree"] > 0).sum() > 30 and (got["n_checked"] > got["n_disagree"]).sum() > 30
            assert (got["n_attempted"] > got["n_valid"]).all() and (got["flags"] & M.ALTITUDE).any()


def test_one_aircraft_longer_than_a_scan_block_and_300_of_one_frame(gpu):
    rng = np.random.default_rng(5)
    big = 0x500000
    items, fixes = M.traffic(8, 5000, [big])
    others = sorted(int(x) for x in rng.choice(np.arange(0x400000, 0x600000), size=300, replace=False))
    o_items, o_fixes = [], []
    for k, icao in enumerate(others):                                   # one frame each, scattered through the big list
        it, fx = M.traffic(100 + k, 1, [icao])
        o_items.append((int(rng.integers(100, 40 * 5000)), it[0][1]))
        o_fixes.append(fx[0])
    both = sorted(zip(items + o_items, list(fixes) + o_fixes), key=lambda p: p[0][0])
    tr = Traffic([p[0] for p in both], np.array([p[1] for p in both]))
    state = tr.state()
    assert len(state) == 301 and state[big]["n_valid"] > 2500 and state[big]["n_disagree"] > 300
    with _table() as table:
        table.update(tr.frames, tr.base, mlat=tr.fixes)
        _, whole = _check(table, state, "one update")
        M.assert_frames_equal(table.frame_mlat().view(M.FRAME_DTYPE), tr.frame_records(), TOL)
        table.reset()
        for a, b in ((0, 1), (1, 2600), (2600, 5299), (5299, 5300)):
            table.update(tr.frames[a:b], tr.base, mlat=tr.fixes[a:b])
        _, cut = _check(table, state, "four updates")
        assert cut.tobytes() == whole.tobytes()


@pytest.mark.parametrize("newest_at", [3, 9])
def test_segment_straddles_the_256_thread_boundary(gpu, newest_at):
    """Aircraft `low` fills sorted positions 0-249, `t` 250-261; t's only valid fix is on its frame 3 (position 253) or
    9 (position 259)."""
    low, t = 0x400001, 0x400002
    place = (47.0, 8.0)
    t_frames = list(range(7, 240, 20))                                  # 12 of the 262
    items = [(100 + 40 * k, M.position_frame(t if k in t_frames else low, 11, k & 1, *place)) for k in range(262)]
    fixes = []
    for k in range(262):
        if k in t_frames and t_frames.index(k) != newest_at:
            fixes.append(M.fix(1.0, 2.0, flags=0x1 | 0x20))
        else:
            fixes.append(M.fix(*place, height_m=float(k)))
    tr = Traffic(items, np.array(fixes))
    with _table() as table:
        table.update(tr.frames, tr.base, mlat=tr.fixes)
        recs, got = _check(table, tr.state())
        assert list(recs["icao"]) == [low, t]
        k = t_frames[newest_at]
        assert got[1]["height_m"] == float(k) and got[1]["time"] == float(tr.base + 100 + 40 * k) * SPS
        assert (got[1]["n_attempted"], got[1]["n_valid"], got[1]["n_checked"]) == (12, 1, 1)
        assert got[0]["n_valid"] == 250 and got[0]["height_m"] == 261.0


# ---- (b) cut invariance ----------------------------------------------------------------------------------------------
def test_cuts_give_identical_bytes(gpu, mixed):
    n = len(mixed.frames)
    with _table() as table:
        table.update(mixed.frames, mixed.base, mlat=mixed.fixes)
        recs, whole = _check(table, mixed.state())
        whole_frames = table.frame_mlat()
        rest = (table.aircraft()[0].tobytes(), table.velocity().tobytes(), table.last_heard().tobytes())
        for name, edges in (("single frames, then 255 / 256 / 257", list(range(65)) + [319, 575, 832, n]),
                            ("255 / 256 / 257 / empty", [0, 255, 511, 768, 768, n])):
            table.reset()
            for a, b in zip(edges[:-1], edges[1:]):
                table.update(mixed.frames[a:b], mixed.base, mlat=mixed.fixes[a:b])
                assert table.frame_mlat().tobytes() == whole_frames[a:b].tobytes(), (name, a, b)
            assert table.mlat().tobytes() == whole.tobytes(), name
            assert (table.aircraft()[0].tobytes(), table.velocity().tobytes(), table.last_heard().tobytes()) == rest
        table.reset()                                                    # two runs give the same bytes
        table.update(mixed.frames, mixed.base, mlat=mixed.fixes)
        assert table.mlat().tobytes() == whole.tobytes() and table.frame_mlat().tobytes() == whole_frames.tobytes()


# ---- (c) host or device memory, each list on its own ------------------------------------------------------------------
def test_memory_sides(gpu, mixed):
    n = 1500
    frames, fixes = mixed.frames[:n].copy(), mixed.fixes[:n].copy()
    rng = np.random.default_rng(9)
    levels = np.zeros(n, dtype=A.LEVEL_DTYPE)
    levels["signal_sum"] = rng.integers(0, 1 << 38, size=n, dtype=np.uint64)
    levels["flags"] = 1
    host = {"frames": frames, "fixes": fixes, "levels": levels}
    first = None
    with _table() as table:
        table.levels_reserve()
        hip = _hip_runtime()
        hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        dev = {}
        for k, v in host.items():
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), v.nbytes) == 0 and hip.hipMemcpy(p, v.ctypes.data, v.nbytes, 1) == 0
            dev[k] = p.value
        for combo in range(8):
            where = {k: bool(combo >> b & 1) for b, k in enumerate(host)}
            ptr = {k: (dev[k] if where[k] else host[k].ctypes.data) for k in host}
            for with_levels in (True, False):
                table.reset()
                table.update_device(ptr["frames"], n, mixed.base, levels_ptr=ptr["levels"] if with_levels else None,
                                    mlat_ptr=ptr["fixes"])
                now = (table.mlat().tobytes(), table.frame_mlat().tobytes(), table.aircraft()[0].tobytes())
                first = now if first is None else first
                assert now == first, (where, with_levels)
                if with_levels:
                    lv = table.levels()
                    assert lv["n_levels"].sum() == n
        _check(table, mixed.state(0, n))
        table.reset()                                                    # waits: nothing reads the lists any more
        assert len(table.mlat()) == 0
        for p in dev.values():
            assert hip.hipFree(p) == 0


# ---- (d) newest wins -----------------------------------------------------------------------------------------------------
def test_newest_wins(gpu):
    a, b, c = 0x4B0001, 0x4B0002, 0x4B0003
    place = (47.0, 8.0)
    near = lambda icao, odd: M.position_frame(icao, 11, odd, *place)
    away = lambda icao: M.position_frame(icao, 11, 1, place[0] + 0.05, place[1])          # 5.56 km
    vel = lambda icao, k: M.raw_frame(icao, 19 << 51 | 1 << 48 | k)
    bad = M.fix(1.0, 2.0, flags=0x1 | 0x20)
    items = [(100, near(a, 0)), (100, away(a)), (100, near(a, 1)),       # a: equal offsets, applied in list order
             (200, near(b, 0)), (300, vel(b, 1)), (400, away(b)), (500, vel(b, 2)),   # b: a valid fix, then invalid ones
             (600, away(c)), (700, near(c, 0)), (800, vel(c, 3))]        # c: the kept fix is newer than the newest check
    fixes = [M.fix(*place, height_m=1.0), M.fix(*place, height_m=2.0), M.fix(*place, height_m=3.0),
             M.fix(*place, height_m=4.0, flags=0x1 | 0x2 | 0x4 | 0x100), bad, M.fix(3.0, 4.0, flags=0x8), bad,
             M.fix(*place, height_m=5.0), M.fix(*place, height_m=6.0), M.fix(*place, height_m=7.0)]
    tr = Traffic(items, np.array(fixes))
    with _table() as table:
        table.update(tr.frames, tr.base, mlat=tr.fixes)
        recs, got = _check(table, tr.state())
        assert list(recs["icao"]) == [a, b, c]
        ga, gb, gc = got
        assert ga["height_m"] == 3.0 and ga["last_disagreement_m"] < 10.0 and 5500 < ga["max_disagreement_m"] < 5620
        assert (ga["n_valid"], ga["n_checked"], ga["n_disagree"]) == (3, 3, 1)
        assert gb["height_m"] == 4.0 and gb["time"] == float(tr.base + 200) * SPS and gb["flags"] == M.VALID | M.ALTITUDE | M.CHECKED
        assert (gb["n_attempted"], gb["n_valid"], gb["n_checked"], gb["n_disagree"]) == (3, 1, 1, 0)
        assert gc["height_m"] == 7.0 and gc["time"] == float(tr.base + 800) * SPS and gc["last_disagreement_m"] < 10.0
        assert (gc["n_valid"], gc["n_checked"], gc["n_disagree"]) == (3, 2, 1) and gc["max_disagreement_m"] > 5500
        fm = table.frame_mlat()
        assert list(fm["flags"]) == [M.VALID | M.CHECKED, M.VALID | M.CHECKED | M.DISAGREE, M.VALID | M.CHECKED,
                                     M.VALID | M.CHECKED, 0, 0, 0, M.VALID | M.CHECKED | M.DISAGREE, M.VALID | M.CHECKED,
                                     M.VALID]
        # FAR: the reported position three degrees of latitude from the solved one
        table.update(M.frames_array([(900, M.cpr_frame(a, 11, 0, 0x10000, 0))], A.FRAME_DTYPE), tr.base,
                     mlat=np.array([M.fix(48.0, 0.0)]))
        fm = table.frame_mlat()
        assert fm[0]["flags"] == M.VALID | M.CHECKED | M.DISAGREE | M.FAR and fm[0]["disagreement_m"] == M.FAR_M
        ga = table.mlat()[0]
        assert ga["last_disagreement_m"] == ga["max_disagreement_m"] == M.FAR_M and ga["n_disagree"] == 2


# ---- (e) the store's life cycle ------------------------------------------------------------------------------------------
def test_full_table_expire_reset_and_held_from_before_the_reserve(gpu):
    rng = np.random.default_rng(13)
    icaos = sorted(int(x) for x in rng.choice(np.arange(0x400000, 0x800000), size=40, replace=False))
    tr = Traffic(*M.traffic(14, 2000, icaos))
    with _table(max_aircraft=16) as table:
        # 40 ICAOs into 16 places: the 24 turned away count nowhere
        table.update(tr.frames[:1000], tr.base, mlat=tr.fixes[:1000])
        away = (table.points()["flags"] & A.ADSB_TRACK_UNTRACKED) != 0
        recs, flags = table.aircraft()
        assert flags == A.ADSB_TRACK_TABLE_FULL and len(recs) == 16 and away.sum() > 400
        state = tr.state(0, 1000, untracked=away)
        assert sorted(state) == sorted(int(x) for x in recs["icao"])
        recs, before = _check(table, state, "full table")
        fm = table.frame_mlat()
        M.assert_frames_equal(fm.view(M.FRAME_DTYPE), tr.frame_records(0, 1000, untracked=away), TOL)
        assert not fm["flags"][away].any() and np.array_equal(fm["icao"], tr.icaos[:1000])
        # expire: the survivors' records move with them, bit for bit
        held = [int(x) for x in recs["icao"]]
        quiet = set(held[1::3])
        later = np.array([int(x) not in quiet for x in tr.icaos[1000:]])
        table.update(tr.frames[1000:][later], tr.base, mlat=tr.fixes[1000:][later])
        away2 = (table.points()["flags"] & A.ADSB_TRACK_UNTRACKED) != 0
        idx = np.nonzero(later)[0] + 1000
        for k, u in zip(idx, away2):
            if not u:
                state[int(tr.icaos[k])] = _combine(state.get(int(tr.icaos[k]), M.empty()), tr.single[k])
        recs, before = _check(table, state, "second update")
        where = {int(x): k for k, x in enumerate(recs["icao"])}
        table.expire(float(tr.base + int(tr.frames["offset"][1000])) * SPS)
        after_recs, after = _check(table, state, "after expire")
        assert set(where) - set(int(x) for x in after_recs["icao"]) == quiet
        for k, icao in enumerate(after_recs["icao"]):
            assert after[k].tobytes() == before[where[int(icao)]].tobytes()
        # an evicted aircraft heard again starts empty (an identification message with a fix that is not valid)
        back = next(i for i in sorted(quiet) if before[where[i]]["n_valid"] > 0)
        last = int(tr.frames["offset"][-1])
        table.update(M.frames_array([(last + 10, M.raw_frame(back, 4 << 51))], A.FRAME_DTYPE), tr.base,
                     mlat=np.array([M.fix(0.0, 0.0, flags=0x8)]))
        recs = table.aircraft()[0]
        got = table.mlat()[list(recs["icao"]).index(back)]
        assert got.tobytes() == EMPTY and math.isnan(got["time"])
        # a plain update leaves the records alone, apart from admission emptying a place
        now = table.mlat().tobytes()
        table.update(tr.frames[:300], tr.base + 2 * last)
        kept = {int(i): r.tobytes() for i, r in zip(table.aircraft()[0]["icao"], table.mlat())}
        for i, r in zip(recs["icao"], np.frombuffer(now, dtype=A.AIRCRAFT_MLAT_DTYPE)):
            assert kept[int(i)] == r.tobytes()
        assert all(v == EMPTY for i, v in kept.items() if i not in set(int(x) for x in recs["icao"]))
        assert len(table.frame_mlat()) == 1                              # still the last update_mlat's list
        # reset: nothing held, and the side array itself is empty again
        table.reset()
        assert len(table.mlat()) == 0
        with pytest.raises(A.AdsbError) as e:
            table.frame_mlat()
        assert e.value.code == A.ADSB_E_STATE
        raw = np.zeros(64 * 16, dtype=np.uint8)
        hip = _hip_runtime()
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipMemcpy.restype = C.c_int
        assert hip.hipMemcpy(raw.ctypes.data, table.mlat_device(), raw.nbytes, 2) == 0     # device to host
        assert raw.tobytes() == EMPTY * 16
    # held from before the reserve: empty until the next counted frame
    with _table(limit=None) as table:
        table.update(tr.frames[:500], tr.base)
        table.mlat_reserve(LIMIT)
        got = table.mlat()
        assert len(got) == 40 and got.tobytes() == EMPTY * 40
        table.update(tr.frames[500:900], tr.base, mlat=tr.fixes[500:900])
        _check(table, tr.state(500, 900), "held from before the reserve")


def _hip_runtime():
    """The HIP runtime this process already holds (the one libadsb_hip.so is bound to), for a plain hipMemcpy."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path:
            return C.CDLL(path)
    raise RuntimeError("no HIP runtime mapped")


# ---- (f) the reserve and update_mlat change nothing else -------------------------------------------------------------------
def test_everything_else_is_byte_identical(gpu, mixed):
    n = 2500
    frames, fixes = mixed.frames[:n], mixed.fixes[:n]
    rng = np.random.default_rng(21)
    levels = np.zeros(n, dtype=A.LEVEL_DTYPE)
    levels["signal_sum"] = rng.integers(0, 1 << 38, size=n, dtype=np.uint64)
    levels["noise_sum"] = rng.integers(0, 1 << 38, size=n, dtype=np.uint64)
    levels["flags"] = (rng.random(n) >= 0.2).astype(np.uint16)
    site = (47.0, 8.0, 180.0)
    kw = dict(seconds_per_sample=SPS, max_frames=1 << 12, max_aircraft=40)     # 60 aircraft: twenty are turned away
    with A.AdsbDemod(max_samples=1024, max_out=16) as d, A.TrackTable(d, **kw) as table, A.TrackTable(d, **kw) as twin, \
            A.TrackTable(d, **kw) as bare:
        for t in (table, twin):
            t.summaries_reserve()
            t.levels_reserve()
            t.fixes_reserve(site)
        table.mlat_reserve(LIMIT)
        table.mlat_reserve(5.0)                                          # a second reserve changes nothing
        for a, b in ((0, 900), (900, 900), (900, n)):
            with_levels = a == 0
            table.update(frames[a:b], mixed.base, levels=levels[a:b] if with_levels else None, mlat=fixes[a:b])
            twin.update(frames[a:b], mixed.base, levels=levels[a:b] if with_levels else None)
            assert table.points().tobytes() == twin.points().tobytes()
            assert table.summaries().tobytes() == twin.summaries().tobytes()
            (x, fx), (y, fy) = table.aircraft(), twin.aircraft()
            assert x.tobytes() == y.tobytes() and fx == fy == A.ADSB_TRACK_TABLE_FULL
            assert table.velocity().tobytes() == twin.velocity().tobytes()
            assert table.levels().tobytes() == twin.levels().tobytes()
            assert table.fixes().tobytes() == twin.fixes().tobytes()
            assert table.frame_fixes().tobytes() == twin.frame_fixes().tobytes()
            assert table.last_heard().tobytes() == twin.last_heard().tobytes()
            assert all(p.tobytes() == q.tobytes() for p, q in zip(table.changed(), twin.changed()))
            assert len(table.frame_mlat()) == b - a
        away = np.zeros(n, dtype=bool)
        held = set(int(i) for i in table.aircraft()[0]["icao"])
        away[:] = [int(i) not in held for i in mixed.icaos[:n]]
        _check(table, mixed.state(0, n, untracked=away), "the first limit stays")
        # the plain forms on the reserved table: the mlat records stay
        now = table.mlat().tobytes()
        table.update(frames[:200], 10 ** 9)
        table.update(frames[:200], 2 * 10 ** 9, levels=levels[:200])
        assert table.mlat().tobytes() == now
        # without the reserve: every mlat entry point says so, and the rest is what it was
        bare.update(frames[:900], 5)
        twin.reset()
        twin.update(frames[:900], 5)
        assert bare.aircraft()[0].tobytes() == twin.aircraft()[0].tobytes() and bare.points().tobytes() == twin.points().tobytes()
        L = _lib.load()
        for call in (lambda: bare.mlat(), lambda: bare.frame_mlat(), lambda: bare.mlat_device(),
                     lambda: bare.update(frames[:10], 5, mlat=fixes[:10]), lambda: bare.update(frames[:0], 5, mlat=fixes[:0])):
            with pytest.raises(A.AdsbError) as e:
                call()
            assert e.value.code == A.ADSB_E_STATE
        bare.mlat_reserve(LIMIT)
        with pytest.raises(A.AdsbError) as e:
            bare.frame_mlat()                                            # no update_mlat yet
        assert e.value.code == A.ADSB_E_STATE
        with pytest.raises(A.AdsbError) as e:
            bare.update(frames[:10], 5, levels=levels[:10], mlat=fixes[:10])    # levels without a levels reserve
        assert e.value.code == A.ADSB_E_STATE
        assert L.adsb_track_table_update_mlat(bare._h, frames.ctypes.data, fixes.ctypes.data, None, (1 << 12) + 1,
                                              0) == A.ADSB_E_CAPACITY
        assert L.adsb_track_table_mlat_reserve(bare._h, math.nan) == A.ADSB_E_ARG
        bare.update(frames[:0], 5, mlat=fixes[:0])                       # n = 0 is fine, and an empty list
        assert len(bare.frame_mlat()) == 0


# ---- (g) correlate -> clock sync -> multilaterate -> update_mlat, all on the device ------------------------------------------
def test_network_end_to_end_on_the_device(gpu, oracle):
    sc = K.network(oracle)
    lst = sc["lst"]
    with A.AdsbDemod(max_samples=1024, max_out=16, host_staging=False) as d, \
            A.TrackTable(d, max_frames=1 << 10, seconds_per_sample=sc["spt"]) as table:
        table.mlat_reserve(LIMIT)
        d.correlate_of_async(lst["frames"], lst["counts"], 4_000_000)   # 4 ms of 1 ns ticks: the clocks are up to 2 ms apart
        # the sync's second pass drops the rows of the aircraft that lies (it would pull every clock by microseconds)
        n_msgs, _ = d.multilaterate_clocks_async(sc["rcv"], lst["rx"], dict(seconds_per_time=sc["spt"], max_residual_s=1e-6),
                                                 use_altitude=True,
                                                 **{k: sc["cfg"][k] for k in ("time_source", "seconds_per_tick")})
        assert n_msgs == 160
        frames_dev, fixes_dev = d.correlated_device()[1], d.mlat_device()[0]
        table.update_device(frames_dev, n_msgs, 0, mlat_ptr=fixes_dev)
        recs, _ = table.aircraft()
        got = table.mlat()
        assert list(recs["icao"]) == [0x400000 + k for k in range(16)]
        # the same lists fetched, through the mirror and the Python merge
        fixes, hdr = d.fetch_mlat()
        frames = d.fetch_correlated()[1]
        assert int(hdr["n_valid"]) >= 150 and len(fixes) == len(frames) == 160
        want = {}
        for k in range(160):
            time = float(int(frames["offset"][k])) * sc["spt"]
            one = A.host_track_mlat_of(LIMIT, frames["bytes"][k].tobytes(), fixes[k], time)[0]
            icao = int(F.frame_icaos(frames[k:k + 1])[0])
            want[icao] = _combine(want.get(icao, M.empty()), np.array([one]).view(M.MODEL_DTYPE)[0])
        M.assert_records_equal(got.view(M.MODEL_DTYPE), M.records(want, recs["icao"]), TOL, "end to end")
        for r, g in zip(recs, got):
            icao = int(r["icao"])
            assert g["flags"] & M.VALID and g["n_valid"] >= 8, hex(icao)
            if icao == 0x400003:
                assert g["n_disagree"] == g["n_checked"] == g["n_valid"] > 0 and 5000 < g["max_disagreement_m"] < 6200
            elif icao in (0x400007, 0x400008):
                assert g["n_checked"] == 0 and not g["flags"] & M.CHECKED and r["has_position"] == 0
            else:
                assert g["n_disagree"] == 0 and g["n_checked"] == g["n_valid"], hex(icao)
