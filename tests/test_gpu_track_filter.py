"""The filter behind a table's multilaterated fixes on the device (adsb_track_table_filter_reserve / fetch_filter /
fetch_frame_filter / adsb_debug_track_filter_operands) against the CPU mirror and the independent model, with fixes the
tests make themselves (tests/track_filter_cases.py).  Lists are at most 5 000 frames.

Three comparisons per update (_verify):
  OPERANDS  device against mirror: time, latitude, longitude, height_m and flags bit for bit; rn, re and the variances by
            the largest |a - b| / max(|a|, |b|, 1).  Two math libraries meet here (sin, cos, sqrt), nowhere else.
  WALK      the device's records and per-frame outputs against the mirror's step FED THE DEVICE'S OWN OPERANDS: bit for
            bit.  The walk has no library call; any difference is a bug.
  END TO END  against the NumPy model: flags and counts exactly, f32 fields equal or neighbours, f64 fields by the same
            relative measure.
MEASURED on an MI355X (every test prints its own): operands 4.18e-16 at most (the 5 000-frame list); end to end 1.51e-15
at most (the update_modes list; 4.7e-16 elsewhere).  The bounds are one order of magnitude above: OPERAND_BOUND =
4.2e-15, MODEL_BOUND = 1.5e-14, both far below the 1e-12 the definition allows.  No decision sits near its threshold
(tests/test_track_filter_host.py checks that in the model), so flags are comparable bit for bit."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from air_rs_amd import demod as D
from tests import modes_model as MD
from tests import track_filter_cases as K
from tests import track_filter_model as M

pytestmark = pytest.mark.gpu
OPERAND_BOUND = 4.2e-15
MODEL_BOUND = 1.5e-14
assert OPERAND_BOUND <= 1e-12 and MODEL_BOUND <= 1e-12
LIMIT = 1000.0
EMPTY = M.empty().tobytes()


def mirror_step(c, a, o):
    return D.host_track_filter_step(a, o, **c)


@contextlib.contextmanager
def _table(max_frames=1 << 13, cfg=None, mlat=True, **kw):
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        with A.TrackTable(d, seconds_per_sample=K.SPS, max_frames=max_frames, **kw) as table:
            if mlat:
                table.mlat_reserve(LIMIT)
            if cfg is not None:
                table.filter_reserve(**cfg)
            yield table


class Expect:
    """What the mirror (fed the device's operands) and the model make of the updates so far."""

    def __init__(self, cfg=None):
        self.c = M.config(**(cfg or {}))
        self.mirror, self.model = {}, {}
        self.worst_op = self.worst = 0.0

    def reset(self):
        self.mirror, self.model = {}, {}

    def update(self, table, case, base=K.BASE, what="", **more):
        """table.update on the case's list, then the three comparisons."""
        frames = K.frames(case)
        table.update(frames, base, mlat=case["fixes"], **more)
        return self.verify(table, case, base, what)

    def verify(self, table, case, base=K.BASE, what="", icaos=None):
        icaos = case["icaos"] if icaos is None else icaos
        n, times = len(icaos), K.times(case, base)
        away = (table.points()["flags"] & (A.ADSB_TRACK_UNTRACKED | A.ADSB_TRACK_UNADDRESSED)) != 0
        order = M.sorted_order(icaos)
        dev_sorted = table.filter_operands()
        assert dev_sorted.dtype == A.FILTER_OPERAND_DTYPE and len(dev_sorted) == n, what
        # OPERANDS
        want = np.zeros(n, dtype=M.OPERAND_DTYPE)
        for s, k in enumerate(order):
            want[s] = D.host_track_filter_operand(case["fixes"][k], times[k], not away[k], **self.c)
        self.worst_op = max(self.worst_op, M.compare_operands(dev_sorted.view(M.OPERAND_DTYPE), want, what))
        # WALK
        dev = np.zeros(n, dtype=M.OPERAND_DTYPE)
        dev[order] = dev_sorted.view(M.OPERAND_DTYPE)
        fr_mirror, _ = M.apply(self.c, self.mirror, icaos, case["fixes"], times, untracked=away, operands=dev,
                               step_fn=mirror_step)
        got_fr = table.frame_filter()
        assert got_fr.dtype == A.FRAME_FILTER_DTYPE and len(got_fr) == n
        bad = np.nonzero(got_fr.view(np.uint8).reshape(n, 32) != fr_mirror.view(np.uint8).reshape(n, 32))[0]
        assert len(bad) == 0, (what, "frames differ from the mirror's at", bad[:5])
        recs = table.aircraft()[0]
        got = table.filter()
        assert got.dtype == A.AIRCRAFT_FILTER_DTYPE and len(got) == len(recs)
        want_recs = M.records(self.mirror, recs["icao"])
        bad = [hex(int(i)) for i, g, w in zip(recs["icao"], got, want_recs) if g.tobytes() != w.tobytes()]
        assert not bad, (what, "records differ from the mirror's for", bad[:5])
        # END TO END
        fr_model, _ = M.apply(self.c, self.model, icaos, case["fixes"], times, untracked=away)
        self.worst = max(self.worst, M.compare_frames(got_fr.view(M.FRAME_DTYPE), fr_model, what),
                         M.compare_records(got.view(M.RECORD_DTYPE), M.records(self.model, recs["icao"]), what))
        return got, got_fr

    def close(self, capsys, what):
        with capsys.disabled():
            print(f"\n{what}: operands {self.worst_op:.3g} (bound {OPERAND_BOUND:.3g}), end to end {self.worst:.3g} "
                  f"(bound {MODEL_BOUND:.3g})")
        assert self.worst_op <= OPERAND_BOUND and self.worst <= MODEL_BOUND


@pytest.fixture(scope="module")
def mixed():
    """5 000 frames of 40 aircraft: the list most tests cut pieces from."""
    rng = np.random.default_rng(3)
    icaos = sorted(int(x) for x in rng.choice(np.arange(0x400000, 0x800000), size=40, replace=False))
    return K.traffic(7, 5000, icaos)


# ---- shapes where the walk can go wrong ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_list_lengths(gpu, mixed, capsys, n):
    ex = Expect()
    with _table(cfg={}) as table:
        got, fr = ex.update(table, K.cut(mixed, 0, n), what=n)
        if n == 5000:
            assert ((got["flags"] & M.VELOCITY) != 0).sum() > 25 and (got["n_outlier"] > 0).sum() > 20
            assert (got["n_reset"] > 0).sum() > 10 and ((fr["flags"] & M.USABLE) == 0).sum() > 300
            assert ((got["flags"] & M.RUNNING) != 0).all() and len(set(mixed["icaos"])) == len(got) == 40
    ex.close(capsys, f"{n} frames")


@pytest.mark.parametrize("name", ["straddle", "one aircraft of 600", "no usable frame", "rules"])
def test_shapes_and_rules(gpu, capsys, name):
    case = {"straddle": K.straddle, "one aircraft of 600": lambda: K.one_aircraft(9, 600), "no usable frame": K.no_usable,
            "rules": K.rules}[name]()
    ex = Expect(case["cfg"])
    with _table(cfg=case["cfg"]) as table:
        got, fr = ex.update(table, case, what=name)
        if name == "straddle":
            assert list(got["n_applied"]) == [249, 11] and (got["flags"] == M.RUNNING | M.VELOCITY | M.HEIGHT).all()
        elif name == "one aircraft of 600":
            assert len(got) == 1 and got[0]["n_applied"] > 400 and got[0]["n_outlier"] > 10
        elif name == "no usable frame":
            assert got.tobytes() == EMPTY * len(got) and fr.tobytes() == bytes(32 * len(fr)) and len(got) == 7
        else:
            assert np.array_equal(fr["flags"], case["flags"])
            assert len(got) == 13 and (fr["flags"] == 0).sum() > 20
    ex.close(capsys, name)


def test_untracked_frames_only_from_a_full_table(gpu, mixed, capsys):
    ex = Expect()
    first = K.traffic(15, 300, [0x400010, 0x400020])
    with _table(cfg={}, max_aircraft=2) as table:
        before, _ = ex.update(table, first, what="fills the table")
        assert len(before) == 2
        later = dict(mixed, offsets=mixed["offsets"] + np.uint64(10 ** 9))
        got, fr = ex.update(table, K.cut(later, 0, 700), what="turned away")
        assert table.aircraft()[1] == A.ADSB_TRACK_TABLE_FULL
        assert got.tobytes() == before.tobytes() and fr.tobytes() == bytes(32 * 700)
        assert table.filter_operands().tobytes() == bytes(64 * 700)
    ex.close(capsys, "full table")


# ---- cut invariance ------------------------------------------------------------------------------------------------------
def test_cuts_give_identical_bytes(gpu, mixed, capsys):
    rules = K.rules()
    rng = np.random.default_rng(41)
    seeded = [0] + sorted(int(x) for x in rng.choice(np.arange(1, 5000), size=12, replace=False)) + [5000]
    ex = Expect()
    with _table(cfg={}) as table:
        for name, case, cuts in (("rules, every boundary", rules, [list(range(len(rules["icaos"]) + 1))]),
                                 ("5 000 frames", mixed, [seeded, [0, 255, 511, 768, 768, 5000]])):
            table.reset()
            ex.reset()
            whole, whole_fr = ex.update(table, case, what=name)
            rest = (table.aircraft()[0].tobytes(), table.mlat().tobytes(), table.last_heard().tobytes())
            frames = K.frames(case)
            for edges in cuts:
                table.reset()
                for a, b in zip(edges[:-1], edges[1:]):
                    table.update(frames[a:b], K.BASE, mlat=case["fixes"][a:b])
                    assert table.frame_filter().tobytes() == whole_fr[a:b].tobytes(), (name, a, b)
                assert table.filter().tobytes() == whole.tobytes(), (name, edges[:4])
                assert (table.aircraft()[0].tobytes(), table.mlat().tobytes(), table.last_heard().tobytes()) == rest
            table.reset()                                                    # two runs give the same bytes
            table.update(frames, K.BASE, mlat=case["fixes"])
            assert table.filter().tobytes() == whole.tobytes() and table.frame_filter().tobytes() == whole_fr.tobytes()
        # max_outliers reached exactly at a cut: the third outlier of 0x4D0003 is the first frame of an update
        third = int(np.nonzero(rules["flags"] == M.USABLE | M.OUTLIER | M.RESET | M.INIT)[0][0])
        table.reset()
        ex.reset()
        ex.update(table, K.cut(rules, 0, third), what="before the third outlier")
        mid = table.filter()[list(table.aircraft()[0]["icao"]).index(0x4D0003)]
        assert (mid["outliers_run"], mid["n_outlier"], mid["n_reset"]) == (2, 2, 0)
        _, fr = ex.update(table, K.cut(rules, third, len(rules["icaos"])), what="from the third outlier on")
        assert fr["flags"][0] == M.USABLE | M.OUTLIER | M.RESET | M.INIT
    ex.close(capsys, "cuts")


# ---- entry points ----------------------------------------------------------------------------------------------------------
def test_update_modes_commb_and_es_filter_as_update_mlat_does(gpu, capsys):
    """DF17 aircraft and one that only answers interrogations (an all-call reply makes its address known, DF4 replies
    follow), each with a fix per frame, through update_modes / update_commb / update_es given fixes."""
    squitters, mode_s = [0x4B1001, 0x4B1002, 0x4B1003], 0x3C4A5B
    base = K.traffic(17, 900, squitters + [mode_s])
    ident = (4 << 51).to_bytes(7, "big")
    seen, msgs = False, []
    for icao in base["icaos"]:
        if int(icao) != mode_s:
            msgs.append(MD.squitter(int(icao), me=ident))
        else:
            msgs.append(MD.reply(4, mode_s, field=MD.field_of(Q=1) | 0x20) if seen else MD.all_call(mode_s))
            seen = True
    frames = MD.frame_list(msgs, base["offsets"]).view(A.FRAME_DTYPE)
    recs = A.host_modes(frames)[0]
    assert np.array_equal(recs["address"], base["icaos"]) and (recs["kind"] <= 1).all() and (recs["df"] == 4).sum() > 50
    commb, es = A.host_commb(frames)[0], A.host_es(frames)[0]
    with _table(cfg={}) as plain:
        plain.update(frames, K.BASE, mlat=base["fixes"])
        keyed = {int(i): r.tobytes() for i, r in zip(plain.aircraft()[0]["icao"], plain.filter())}
    for name, more in (("update_modes", dict(modes=recs)), ("update_commb", dict(modes=recs, commb=commb)),
                       ("update_es", dict(modes=recs, commb=commb, es=es)), ("update_es alone", dict(es=es))):
        ex = Expect()
        with _table(cfg={}) as table:
            table.modes_reserve()
            table.commb_reserve()
            table.es_reserve()
            for lo, hi in ((0, 400), (400, 900)):
                part = K.cut(base, lo, hi)
                table.update(frames[lo:hi], K.BASE, mlat=part["fixes"], **{k: v[lo:hi] for k, v in more.items()})
                icaos = part["icaos"] if "modes" in more else frames_icaos(frames[lo:hi])
                got, _ = ex.verify(table, part, what=name, icaos=icaos)
            held = {int(i): r for i, r in zip(table.aircraft()[0]["icao"], got)}
            for icao in squitters:
                assert held[icao].tobytes() == keyed[icao], (name, hex(icao))
            if "modes" in more:
                s = held[mode_s]
                assert s["flags"] & M.VELOCITY and s["n_applied"] > 50 and table.aircraft()[0]["has_position"].sum() == 0
                speed = D.filter_physical(np.array([s]))[0]["ground_speed_kt"]
                assert 150.0 < speed < 600.0
        ex.close(capsys, name)


def frames_icaos(frames):
    b = frames["bytes"].astype(np.uint32)
    return b[:, 1] << 16 | b[:, 2] << 8 | b[:, 3]


# ---- nothing else moves, and the store's life cycle -------------------------------------------------------------------------
def _everything_else(t):
    return [t.aircraft()[0].tobytes(), t.aircraft()[1], t.points().tobytes(), t.mlat().tobytes(), t.frame_mlat().tobytes(),
            t.velocity().tobytes(), t.fixes().tobytes(), t.frame_fixes().tobytes(), t.levels().tobytes(),
            t.last_heard().tobytes(), [x.tobytes() for x in t.changed()], t.summaries().tobytes()]


def test_everything_else_is_byte_identical_and_the_life_cycle(gpu, mixed, capsys):
    n = 3000
    frames = K.frames(mixed)
    rng = np.random.default_rng(21)
    levels = np.zeros(n, dtype=A.LEVEL_DTYPE)
    levels["signal_sum"] = rng.integers(0, 1 << 38, size=n, dtype=np.uint64)
    levels["flags"] = 1
    kw = dict(seconds_per_sample=K.SPS, max_frames=1 << 12, max_aircraft=30)       # 40 aircraft: ten are turned away
    ex = Expect(dict(gate=5.0))
    with A.AdsbDemod(max_samples=1024, max_out=16) as d, A.TrackTable(d, **kw) as table, A.TrackTable(d, **kw) as twin, \
            A.TrackTable(d, **kw) as bare:
        for t in (table, twin):
            t.summaries_reserve()
            t.levels_reserve()
            t.fixes_reserve((47.0, 8.0, 180.0))
            t.mlat_reserve(LIMIT)
        table.filter_reserve(gate=5.0)
        table.filter_reserve(gate=2.0, accel_h=50.0)                         # a second reserve changes nothing
        for a, b in ((0, 900), (900, 900), (900, n)):
            part = K.cut(mixed, a, b)
            more = dict(levels=levels[a:b]) if a == 0 else {}
            ex.update(table, part, what=(a, b), **more)
            twin.update(frames[a:b], K.BASE, mlat=part["fixes"], **more)
            assert _everything_else(table) == _everything_else(twin), (a, b)
            assert len(table.frame_filter()) == b - a
        assert table.aircraft()[1] == A.ADSB_TRACK_TABLE_FULL
        # a plain update, and one with levels, leave the filter records alone (apart from admission emptying a place)
        recs = table.aircraft()[0]
        now = table.filter()
        table.update(frames[:200], 10 ** 10)
        table.update(frames[:200], 2 * 10 ** 10, levels=levels[:200])
        assert table.filter().tobytes() == now.tobytes() and len(table.frame_filter()) == n - 900
        # expire: the survivors' records move with them, bit for bit
        held = [int(x) for x in recs["icao"]]
        drop = set(held[1::3])                                               # these stay silent, as do those whose part is over
        sel = np.array([k for k in range(n, 5000) if int(mixed["icaos"][k]) not in drop])
        stay = set(int(i) for i in mixed["icaos"][sel]) & set(held)
        quiet = set(held) - stay
        assert len(stay) >= 2 and len(quiet) >= 10
        cut_time = float(3 * 10 ** 10) * K.SPS
        table.update(frames[sel], 3 * 10 ** 10 + 1, mlat=mixed["fixes"][sel])
        before = {int(i): r.tobytes() for i, r in zip(table.aircraft()[0]["icao"], table.filter())}
        table.expire(cut_time)
        after_recs, after = table.aircraft()[0], table.filter()
        assert set(int(x) for x in after_recs["icao"]) == stay and len(after) == len(after_recs)
        assert all(r.tobytes() == before[int(i)] for i, r in zip(after_recs["icao"], after))
        # an evicted aircraft heard again starts empty (its fix is not valid), then starts over at its next usable frame
        back = next(i for i in sorted(quiet) if np.frombuffer(before[i], dtype=A.AIRCRAFT_FILTER_DTYPE)[0]["n_applied"] > 0)
        one = K.frames(dict(icaos=[back], offsets=[5]))
        table.update(one, 4 * 10 ** 10, mlat=np.array([M.fix(0.0, 0.0, flags=0x8)]))
        got = table.filter()[list(table.aircraft()[0]["icao"]).index(back)]
        assert got.tobytes() == EMPTY and math.isnan(got["time"])
        table.update(one, 4 * 10 ** 10 + 10, mlat=np.array([M.fix(47.0, 8.0)]))
        got = table.filter()[list(table.aircraft()[0]["icao"]).index(back)]
        assert (got["run"], got["n_applied"], got["n_reset"], got["flags"]) == (1, 0, 0, M.RUNNING | M.HEIGHT)
        # reset: nothing held, the side array itself is empty again, and the per-frame fetches have no list
        table.reset()
        assert len(table.filter()) == 0
        for call in (table.frame_filter, table.filter_operands):
            with pytest.raises(A.AdsbError) as e:
                call()
            assert e.value.code == A.ADSB_E_STATE
        raw = np.zeros(192 * 30, dtype=np.uint8)
        hip = _hip_runtime()
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipMemcpy.restype = C.c_int
        assert hip.hipMemcpy(raw.ctypes.data, table.filter_device(), raw.nbytes, 2) == 0     # device to host
        assert raw.tobytes() == EMPTY * 30
        # without the reserves: every entry point says so
        for call in (bare.filter, bare.frame_filter, bare.filter_device, bare.filter_operands, bare.filter_reserve):
            with pytest.raises(A.AdsbError) as e:
                call()
            assert e.value.code == A.ADSB_E_STATE                            # filter_reserve: no mlat reserve
        bare.mlat_reserve(LIMIT)
        bare.update(frames[:50], K.BASE, mlat=mixed["fixes"][:50])           # held from before the filter reserve
        bare.filter_reserve()
        assert bare.filter().tobytes() == EMPTY * len(bare.aircraft()[0])
        with pytest.raises(A.AdsbError) as e:
            bare.frame_filter()                                              # no update given fixes since the reserve
        assert e.value.code == A.ADSB_E_STATE
        bare.update(frames[:0], K.BASE, mlat=mixed["fixes"][:0])             # n = 0 is fine, and an empty list
        assert len(bare.frame_filter()) == 0 and len(bare.filter_operands()) == 0
        L = _lib.load()
        n_out = C.c_size_t()
        assert L.adsb_track_table_fetch_filter(bare._h, None, 1, C.byref(n_out)) == A.ADSB_E_ARG
        assert L.adsb_track_table_fetch_frame_filter(bare._h, None, 1, C.byref(n_out)) == A.ADSB_E_ARG
        assert L.adsb_debug_track_filter_operands(bare._h, None, 1, C.byref(n_out)) == A.ADSB_E_ARG
        bad = D._filter_cfg(gate=-1.0)
        assert L.adsb_track_table_filter_reserve(bare._h, C.byref(bad)) == A.ADSB_E_ARG
        assert L.adsb_track_table_filter_device(bare._h, None) == A.ADSB_OK
    ex.close(capsys, "beside a twin, the first cfg stays")


def _hip_runtime():
    """The HIP runtime this process already holds (the one libadsb_hip.so is bound to), for a plain hipMemcpy."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path:
            return C.CDLL(path)
    raise RuntimeError("no HIP runtime mapped")
