"""The device memory behind a track table and a track bank (air_rs_amd/csrc/adsb_track_api.cpp: the store's own arrays
and those of the summaries, levels, fixes and fuse reserves) under every order of the reserves, a fuse reserve repeated
behind a fuse in flight, lists and tables filled to the last place, and twenty stores created and destroyed beside a
survivor.  Expected values: a store that reserved everything before its first update, and the models of the tracker
tests (the oracle tracker, tests/track_levels_model.py, tests/fix_model.py, tests/fuse_model.py,
tests/velocity_traffic.py).  Nothing here depends on how the arrays are allocated: the tests hold for any library that
keeps the public contract."""
import itertools

import numpy as np
import pytest

import air_rs_amd as A
from tests import fix_model as FM
from tests import fuse_model
from tests import track_levels_model as LM
from tests.test_gpu_track_expire import Model, _check_points
from tests.test_gpu_track_summaries import _empty, _same_summary
from tests.test_gpu_track_velocity import _same_velocity
from tests.traffic import ident_frame, position_frame
from tests.velocity_traffic import last_velocity, random_velocity_frame, velocity_traffic

pytestmark = pytest.mark.gpu
SPS = 1e-3
R = 3
SITES = [(47.45, 8.56, 150.0), (47.0, 9.0, 180.0), (48.0, 8.0, 60.0)]
BASES = [7, 1000, 250]
FULL, TRUNCATED = A.ADSB_TRACK_TABLE_FULL, A.ADSB_TRACK_FUSED_TRUNCATED


def _frames(items):
    """[(offset, 14 frame bytes)] -> FRAME_DTYPE array."""
    out = np.zeros(len(items), dtype=A.FRAME_DTYPE)
    for k, (off, b) in enumerate(items):
        out[k]["offset"] = off
        out[k]["bytes"] = np.frombuffer(bytes(b), dtype=np.uint8)
        out[k]["fixed_bit"] = 0xFF
    return out


def _levels(n, seed):
    """Synthetic adsb_frame_level records: sums below 2^38, about one in five invalid."""
    rng = np.random.default_rng(seed)
    lv = np.zeros(n, dtype=A.LEVEL_DTYPE)
    lv["signal_sum"] = rng.integers(0, 1 << 38, size=n, dtype=np.uint64)
    lv["noise_sum"] = rng.integers(0, 1 << 38, size=n, dtype=np.uint64)
    lv["peak"] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    lv["weak_bits"] = rng.integers(0, 113, size=n)
    lv["flags"] = (rng.random(n) >= 0.2).astype(np.uint16)
    return lv


def _bytes(x):
    """What a fetch returned (an array, a list per receiver, a tuple with flags or counts) as one bytes value."""
    if isinstance(x, np.ndarray):
        return x.tobytes()
    if isinstance(x, (list, tuple)):
        return b"|".join(_bytes(v) for v in x)
    return repr(x).encode()


def _same(got, want, what):
    assert got.dtype.itemsize == want.dtype.itemsize and len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():                      # say where, then fail
        for k in range(len(got)):
            assert got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])


class _Store:
    """A table (receiver 0's lists) or a bank of R receivers behind one interface, for the tests of both."""

    def __init__(self, d, kind, max_aircraft, max_frames):
        self.kind = kind
        if kind == "table":
            self.s = A.TrackTable(d, max_aircraft=max_aircraft, max_frames=max_frames, seconds_per_sample=SPS)
        else:
            self.s = A.TrackBank(d, R, max_aircraft=max_aircraft, max_frames=max_frames, seconds_per_sample=SPS)
        self.has = set()

    def close(self):
        self.s.close()

    def reserve(self, what):
        """S summaries, L levels, F fixes, U fuse (a bank's)"""
        if what == "S":
            self.s.summaries_reserve()
        elif what == "L":
            self.s.levels_reserve()
        elif what == "F":
            self.s.fixes_reserve(SITES[0] if self.kind == "table" else SITES)
        else:
            self.s.fuse_reserve(0)
        self.has.add(what)

    def update(self, lists, levels):
        """One update; the levels go with it once the levels reserve is there."""
        if self.kind == "table":
            self.s.update(lists[0], BASES[0], levels=levels[0] if "L" in self.has else None)
        else:
            self.s.update(np.concatenate(lists), [len(x) for x in lists], BASES,
                          levels=np.concatenate(levels) if "L" in self.has else None)

    def views(self):
        """name -> bytes of every fetch the store's reserves allow"""
        names = ["aircraft", "last_heard", "velocity", "points"]
        names += ["summaries", "changed"] if "S" in self.has else []
        names += ["levels"] if "L" in self.has else []
        names += ["fixes", "frame_fixes"] if "F" in self.has else []
        out = {name: _bytes(getattr(self.s, name)()) for name in names}
        if "U" in self.has:
            out["fused"] = _bytes(self.s.fuse())
            if "L" in self.has:
                out["fused_levels"] = _bytes(self.s.fused_levels())
        return out

    def level_records(self):
        """[per receiver: (the records' ICAOs, their level records)]"""
        if self.kind == "table":
            return [(self.s.aircraft()[0]["icao"], self.s.levels())]
        return [(recs["icao"], lv) for recs, lv in zip(self.s.aircraft()[0], self.s.levels())]


# ---- reserve orders ---------------------------------------------------------------------------------------------------
N_PARTS = 6
AFTER_LEVELS = ("levels", "fused_levels")                     # what depends on when the levels reserve came


@pytest.fixture(scope="module")
def parts(oracle):
    """Six updates' worth of one fleet of 20 aircraft (positions, identifications, TC 19) heard by three receivers, 70 %
    of it each: parts[u] = (per-receiver FRAME_DTYPE lists, per-receiver level records)."""
    rng = np.random.default_rng(3)
    traffic = velocity_traffic(oracle, seed=3, n_aircraft=20, n_frames=720, span_s=60.0)
    out = []
    for u in range(N_PARTS):
        mine = [(t, fr) for t, fr in traffic if 10.0 * u <= t < 10.0 * (u + 1)]
        lists = [_frames([(round(t / SPS), fr) for t, fr in mine if rng.random() < 0.7]) for _ in range(R)]
        out.append((lists, [_levels(len(x), seed=100 * u + r) for r, x in enumerate(lists)]))
    assert all(60 < len(x) < 120 for lists, _ in out for x in lists)
    return out


@pytest.fixture(scope="module")
def up_front(gpu, parts):
    """kind -> per update the views of a store that made every reserve before its first update: computed once."""
    out = {}
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        for kind, reserves in (("table", "SLF"), ("bank", "SLFU")):
            store = _Store(d, kind, max_aircraft=32, max_frames=512)
            try:
                for what in reserves:
                    store.reserve(what)
                out[kind] = []
                for lists, levels in parts:
                    store.update(lists, levels)
                    out[kind].append(store.views())
            finally:
                store.close()
    return out


def _run_order(gpu, parts, up_front, kind, order):
    """The reserves of `order` up to and with F (fixes: before the first aircraft) come before the first update, the
    others one by one between the updates that follow; after the fifth update every reserve is made a second time."""
    first = order[:order.index("F") + 1]
    later = {u + 1: what for u, what in enumerate(order[len(first):])}        # before update u
    want = up_front[kind]
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        store = _Store(d, kind, max_aircraft=32, max_frames=512)
        try:
            for what in first:
                store.reserve(what)
            if "F" in first:
                store.reserve("F")                            # no aircraft yet: allowed, copies the sites again
            levels_state = [{} for _ in range(R)]
            for u, (lists, levels) in enumerate(parts):
                if u in later:
                    store.reserve(later[u])
                if u == N_PARTS - 1:                          # everything a second time: nothing changes
                    before = store.views()
                    for what in "SLU" if kind == "bank" else "SL":
                        store.reserve(what)
                    with pytest.raises(A.AdsbError) as e:
                        store.reserve("F")                    # it holds aircraft
                    assert e.value.code == A.ADSB_E_STATE
                    assert store.views() == before
                store.update(lists, levels)
                got = store.views()
                for name, value in got.items():
                    if name not in AFTER_LEVELS:
                        assert value == want[u][name], (order, u, name)
                if "L" in store.has:                          # the levels of the frames heard since their reserve
                    for r, (icaos, lv) in enumerate(store.level_records()):
                        LM.apply(levels_state[r], lists[r], levels[r], BASES[r], SPS)
                        _same(lv, LM.records(levels_state[r], icaos), (order, u, r))
                    if "U" in store.has:
                        recs, heard = store.s.aircraft()[0], store.s.last_heard()
                        _same(store.s.fused_levels(),
                              LM.fuse([x["icao"] for x in recs], heard, store.s.levels()), (order, u, "fused levels"))
            assert store.has == set(order) and u == N_PARTS - 1
            if "L" in first:                                  # reserved before the first update: the up-front bytes
                for name in AFTER_LEVELS:
                    if name in got:
                        assert got[name] == want[-1][name], (order, name)
        finally:
            store.close()


@pytest.mark.parametrize("order", ["".join(p) for p in itertools.permutations("SLF")])
def test_table_reserve_orders(gpu, parts, up_front, order):
    _run_order(gpu, parts, up_front, "table", order)


@pytest.mark.parametrize("order", ["FUSL", "FLSU", "SLUF", "UFLS", "LFUS", "FSUL"])
def test_bank_reserve_orders(gpu, parts, up_front, order):
    """U: the fuse reserve, before the levels reserve (which then makes the fused levels' array) and after it (then the
    fuse reserve does)."""
    _run_order(gpu, parts, up_front, "bank", order)


# ---- the fuse reserve repeated behind a fuse in flight ------------------------------------------------------------------
def test_fuse_reserved_again_behind_a_fuse_in_flight(gpu, parts):
    lists = [np.concatenate([p[0][r] for p in parts[:3]]) for r in range(R)]
    levels = [np.concatenate([p[1][r] for p in parts[:3]]) for r in range(R)]
    with A.AdsbDemod(max_samples=1024, max_out=16) as d, \
            A.TrackBank(d, R, max_aircraft=32, max_frames=1024, seconds_per_sample=SPS) as bank:
        bank.levels_reserve()
        bank.fuse_reserve(8)
        bank.update(np.concatenate(lists), [len(x) for x in lists], BASES, levels=np.concatenate(levels))
        recs, _ = bank.aircraft()
        want = fuse_model.fuse(recs, bank.last_heard(), bank.velocity())
        want_levels = LM.fuse([x["icao"] for x in recs], bank.last_heard(), bank.levels())
        assert len(want) == len(want_levels) == 20

        def fused(n):
            got, total, flags = bank.fuse()
            assert total == 20 and flags == (TRUNCATED if n < 20 else 0), (n, total, flags)
            _same(got, want[:n], ("fused", n))
            _same(bank.fused_levels(), want_levels[:n], ("fused levels", n))

        fused(8)
        bank.fuse_async()                                     # reads the small reserve's arrays ...
        bank.fuse_reserve(0)                                  # ... which go here
        fused(20)
        bank.fuse_async()
        bank.fuse_reserve(8)                                  # and back, large to small
        fused(8)
        bank.fuse_async()
        bank.fuse_reserve(20)                                 # exactly enough
        fused(20)


# ---- lists and tables filled to the last place ---------------------------------------------------------------------------
def _near(site, rng):
    return site[0] + float(rng.uniform(-0.4, 0.4)), site[1] + float(rng.uniform(-0.4, 0.4))


def _full_list(oracle, rng, where, first, rest, n, t0):
    """n frames from t0 on, 7 samples apart: an even and an odd position of every aircraft of `first`, then the aircraft
    of `rest` in turn with an identification, a TC 19 frame, an even and an odd position, and so on."""
    items, k = [], 0
    for icao in first:
        for odd in (False, True):
            items.append((icao, ("pos", odd)))
    while len(items) < n:
        kind = (k // len(rest)) % 4
        items.append((rest[k % len(rest)], ("ident",) if kind == 0 else ("vel",) if kind == 1 else ("pos", kind == 3)))
        k += 1
    assert len(items) == n
    out = []
    for j, (icao, what) in enumerate(items):
        if what[0] == "pos":
            lat, lon = where[icao]
            fr = position_frame(oracle, icao, what[1], *FM.cpr_encode(lat, lon, what[1], False))
        elif what[0] == "ident":
            fr = ident_frame(oracle, icao, list(rng.integers(1, 27, size=8)))
        else:
            fr = random_velocity_frame(oracle, rng, icao)
        out.append((t0 + 7 * j, fr))
    return _frames(out)


class _BankModel:
    """Per receiver: the oracle tracker's table, running frame counts, the timed frames of the aircraft held, the level
    and the fix model's states."""

    def __init__(self, oracle, max_aircraft):
        self.table = [Model(oracle, SPS, max_aircraft) for _ in range(R)]
        self.count = [{} for _ in range(R)]
        self.timed = [[] for _ in range(R)]
        self.lvl = [{} for _ in range(R)]
        self.fix = [{} for _ in range(R)]

    def expire(self, cuts):
        for r in range(R):
            self.table[r].expire(cuts[r])
            held = set(self.table[r].ac)
            self.timed[r] = [(t, fr) for t, fr in self.timed[r] if int.from_bytes(fr[1:4], "big") in held]
            for state in (self.count[r], self.lvl[r], self.fix[r]):
                for icao in [i for i in state if i not in held]:
                    del state[icao]

    def check_update(self, bank, lists, levels, what):
        """Every fetch of the bank after update(lists, levels) against its model."""
        pts, sums, ff = bank.points(), bank.summaries(), bank.frame_fixes()
        (recs, flags), heard, vel = bank.aircraft(), bank.last_heard(), bank.velocity()
        lv, fx = bank.levels(), bank.fixes()
        assert len(pts) == len(sums) == len(ff) == sum(len(x) for x in lists)
        pos, touched = 0, []
        for r in range(R):
            frames, n = lists[r], len(lists[r])
            want = self.table[r].update(frames, BASES[r])
            _check_points(pts[pos:pos + n], want)
            away = np.array([new is None for _, new, _ in want])
            for k, (icao, new, s) in enumerate(want):
                if new is None:                               # turned away: the empty record with its ICAO
                    assert sums[pos + k].tobytes() == _empty(icao).tobytes(), (what, r, k)
                    continue
                self.count[r][icao] = self.count[r].get(icao, 0) + 1
                _same_summary(sums[pos + k], s, self.count[r][icao], (what, r, k))
                self.timed[r].append((float(BASES[r] + int(frames[k]["offset"])) * SPS, bytes(frames[k]["bytes"])))
            self.table[r].check(recs[r], heard[r], flags[r])
            _same_velocity(vel[r], recs[r], last_velocity(self.timed[r]))
            LM.apply(self.lvl[r], frames, levels[r], BASES[r], SPS, untracked=away)
            _same(lv[r], LM.records(self.lvl[r], recs[r]["icao"]), (what, r, "levels"))
            FM.apply(self.fix[r], SITES[r], frames, BASES[r], SPS, untracked=away)
            FM.assert_fixes_equal(fx[r], FM.records(self.fix[r], recs[r]["icao"]), (what, r, "fixes"))
            FM.assert_frame_fixes_equal(ff[pos:pos + n], FM.frame_records(SITES[r], frames, untracked=away), (what, r))
            touched.append(sorted({icao for icao, new, _ in want if new is not None}))
            pos += n
        # the changed list: the rows of the aircraft this update touched
        crecs, cheard, cvel, ccounts = bank.changed()
        assert ccounts == [len(x) for x in touched], what
        rows = [np.isin(recs[r]["icao"], touched[r]) for r in range(R)]
        assert crecs.tobytes() == b"".join(recs[r][rows[r]].tobytes() for r in range(R)), what
        assert cheard.tobytes() == b"".join(heard[r][rows[r]].tobytes() for r in range(R)), what
        assert cvel.tobytes() == b"".join(vel[r][rows[r]].tobytes() for r in range(R)), what
        self.check_fused(bank, what)
        return recs, flags, fx

    def check_fused(self, bank, what):
        (recs, _), heard = bank.aircraft(), bank.last_heard()
        got, total, flags = bank.fuse()
        want = fuse_model.fuse(recs, heard, bank.velocity())
        _same(got, want, (what, "fused"))
        assert total == len(want) and flags == 0, what
        _same(bank.fused_levels(), LM.fuse([x["icao"] for x in recs], heard, bank.levels()), (what, "fused levels"))


def test_lists_and_tables_filled_to_the_last_place(gpu, oracle):
    """max_frames = 256 and max_aircraft = 16, every reserve.  Both updates are 256 frames long and leave every receiver
    with exactly 16 aircraft, receiver 1 having turned some away; between them an expire evicts half of each table.
    Every array of every reserve is used up to its last record, and every fetch equals its model."""
    rng = np.random.default_rng(17)
    icaos = sorted(int(x) for x in rng.choice(np.arange(1, 1 << 24), size=40, replace=False))
    where = {icao: _near(SITES[0], rng) for icao in icaos}
    offered = [icaos[:16], icaos[:24], icaos[8:24]]           # receiver 1 holds its lowest 16 of 24
    n_frames = [80, 96, 80]
    first = [_full_list(oracle, rng, where, offered[r], offered[r][::2], n_frames[r], 100) for r in range(R)]
    cut_at = [float(BASES[r] + 100 + 7 * 2 * len(offered[r])) * SPS for r in range(R)]   # the second phase's first frame
    with A.AdsbDemod(max_samples=1024, max_out=16) as d, \
            A.TrackBank(d, R, max_aircraft=16, max_frames=256, seconds_per_sample=SPS) as bank:
        bank.fixes_reserve(SITES)
        bank.summaries_reserve()
        bank.levels_reserve()
        bank.fuse_reserve(0)
        model = _BankModel(oracle, 16)
        levels = [_levels(len(x), seed=40 + r) for r, x in enumerate(first)]
        assert sum(len(x) for x in first) == bank.max_frames
        bank.update(np.concatenate(first), n_frames, BASES, levels=np.concatenate(levels))
        recs, flags, fx = model.check_update(bank, first, levels, "first")
        assert [len(x) for x in recs] == [16, 16, 16] and flags == [0, FULL, 0]
        assert all((x["n_fixes"] > 0).sum() >= 4 for x in fx)
        # half of every table has been silent since cut_at
        bank.expire(cut_at)
        model.expire(cut_at)
        recs, flags = bank.aircraft()
        assert [len(x) for x in recs] == [8, 8, 8]
        for r in range(R):
            model.table[r].check(recs[r], bank.last_heard()[r], flags[r])
            _same(bank.levels()[r], LM.records(model.lvl[r], recs[r]["icao"]), ("expired", r, "levels"))
            FM.assert_fixes_equal(bank.fixes()[r], FM.records(model.fix[r], recs[r]["icao"]), ("expired", r, "fixes"))
        model.check_fused(bank, "expired")
        # the survivors and as many new aircraft as fill the tables again (receiver 1: more than that)
        held = [[int(x) for x in recs[r]["icao"]] for r in range(R)]
        again = [held[0] + icaos[24:32], held[1] + icaos[24:40], held[2] + icaos[32:40]]
        second = [_full_list(oracle, rng, where, again[r], again[r], n_frames[r], 5000) for r in range(R)]
        levels = [_levels(len(x), seed=50 + r) for r, x in enumerate(second)]
        bank.update(np.concatenate(second), n_frames, BASES, levels=np.concatenate(levels))
        recs, flags, fx = model.check_update(bank, second, levels, "second")
        assert [len(x) for x in recs] == [16, 16, 16] and flags == [0, FULL, 0]
        assert [model.table[r].n_partial for r in range(R)] == [0, 2, 0]


# ---- life cycle ------------------------------------------------------------------------------------------------------------
def test_twenty_stores_come_and_go_beside_a_survivor(gpu, parts):
    """Twenty rounds of create, every reserve, one update, destroy, for a table and a bank on the context of a bank that
    lives throughout.  The survivor's fetches do not change, and the device's free memory afterwards is within one
    store's size of what it was before: the larger store's, a table's, which by the public header's formula is 64 MiB
    of ICAO index + 136 bytes per aircraft + about 100 bytes per frame.  A store that leaked would take twenty times
    that."""
    import torch
    max_aircraft, max_frames = 64, 1024
    one_store = (64 << 20) + 136 * max_aircraft + 100 * max_frames
    lists, levels = parts[0]
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        survivor = _Store(d, "bank", max_aircraft, max_frames)
        try:
            for what in "FSLU":
                survivor.reserve(what)
            survivor.update(lists, levels)
            before = survivor.views()
            torch.cuda.synchronize()
            free_before = torch.cuda.mem_get_info()[0]
            for _ in range(20):
                for kind in ("table", "bank"):
                    store = _Store(d, kind, max_aircraft, max_frames)
                    try:
                        for what in "FSLU" if kind == "bank" else "FSL":
                            store.reserve(what)
                        store.update(lists, levels)
                        assert len(store.s.points()) == (len(lists[0]) if kind == "table" else sum(map(len, lists)))
                    finally:
                        store.close()
            torch.cuda.synchronize()
            free_after = torch.cuda.mem_get_info()[0]
            print(f"free device memory: {free_before} before, {free_after} after, one store {one_store}")
            assert free_before - free_after <= one_store
            assert survivor.views() == before
        finally:
            survivor.close()
