"""Expiry of the device track table and bank (adsb_track_table_expire / adsb_track_bank_expire, TrackTable.expire /
TrackBank.expire, last_heard()).  Aircraft are independent in aircraft.rs, so the model is one oracle tracker per
aircraft LIFETIME: the model evicts an ICAO by the same rule (last_heard < before, from the times it fed), drops its
tracker, and the next frame of that ICAO starts a fresh one.  Admission follows the table's rule: the new ICAOs of one
update in ascending order while there is room."""
import contextlib
import math

import numpy as np
import pytest

import air_rs_amd as A
from tests.traffic import ident_frame, position_frame, random_traffic

NEW, UNTRACKED, FULL = A.ADSB_TRACK_NEW_POSITION, A.ADSB_TRACK_UNTRACKED, A.ADSB_TRACK_TABLE_FULL


def _frames(items):
    """[(offset, 14 frame bytes)] -> FRAME_DTYPE array."""
    out = np.zeros(len(items), dtype=A.FRAME_DTYPE)
    for k, (off, b) in enumerate(items):
        out[k]["offset"] = off
        out[k]["bytes"] = np.frombuffer(bytes(b), dtype=np.uint8)
        out[k]["fixed_bit"] = 0xFF
    return out


def _concat(lists):
    return np.concatenate(lists) if lists else np.zeros(0, dtype=A.FRAME_DTYPE)


def _icao(fr):
    return _icao_of(fr["bytes"])


def _icao_of(b):
    return (int(b[1]) << 16) | (int(b[2]) << 8) | int(b[3])


def _even_odd(oracle, icao, odd):
    # the CPR halves of the reference pair (aircraft.rs:201-212), under another ICAO: every such pair decodes
    return position_frame(oracle, icao, odd, 74158 if odd else 93000, 50194 if odd else 51372)


class Model:
    """One table: ICAO -> [oracle tracker of this lifetime, frames, last heard]."""

    def __init__(self, oracle, sps, max_aircraft=65536):
        self.oracle, self.sps, self.max = oracle, sps, max_aircraft
        self.ac, self.full = {}, 0
        self.max_size = self.n_partial = 0      # largest size seen; updates that admitted only some new ICAOs

    def update(self, frames, base):
        """Feeds one list; returns (icao, new position?, summary) per frame, new = None for an UNTRACKED frame."""
        icaos = [_icao(fr) for fr in frames]
        new = sorted({i for i in icaos if i not in self.ac})
        admitted = new[:max(self.max - len(self.ac), 0)]
        if len(admitted) < len(new):
            self.full = FULL
            self.n_partial += len(admitted) > 0
        for i in admitted:
            self.ac[i] = [self.oracle.tracker(), 0, None]
        out = []
        for fr, icao in zip(frames, icaos):
            a = self.ac.get(icao)
            if a is None:
                out.append((icao, None, None))
                continue
            t = float(base + int(fr["offset"])) * self.sps
            is_new, s = a[0].update(bytes(fr["bytes"]), t)
            a[1] += 1
            a[2] = t
            out.append((icao, is_new, s))
        self.max_size = max(self.max_size, len(self.ac))
        return out

    def expire(self, before):
        for icao in [i for i, a in self.ac.items() if a[2] < before]:
            del self.ac[icao]

    def check(self, recs, last_heard, flags):
        """The whole table as fetch / fetch_last_heard return it (ascending ICAO) and the table flags."""
        want = sorted(self.ac.items())
        assert [int(r["icao"]) for r in recs] == [i for i, _ in want]
        assert len(last_heard) == len(recs) and flags == self.full
        for rec, lh, (icao, (tr, n, last)) in zip(recs, last_heard, want):
            s = tr.aircraft()[0]
            assert rec["n_frames"] == n and lh == last, hex(icao)
            assert rec["callsign"].decode() == s.callsign.decode() and rec["altitude"] == s.altitude
            assert bool(rec["has_position"]) == bool(s.has_position)
            if s.has_position:
                assert (rec["latitude"], rec["longitude"]) == pytest.approx((s.latitude, s.longitude), abs=1e-9)
            assert (math.isnan(rec["last_contact"]) and math.isnan(s.last_contact)) or \
                rec["last_contact"] == pytest.approx(s.last_contact, abs=1e-9)


def _check_points(pts, want):
    assert len(pts) == len(want)
    for k, (p, (icao, new, s)) in enumerate(zip(pts, want)):
        assert int(p["icao"]) == icao, k
        if new is None:
            assert int(p["flags"]) == UNTRACKED, k
            continue
        assert int(p["flags"]) == (NEW if new else 0), k
        if new:
            assert (p["latitude"], p["longitude"]) == pytest.approx((s.latitude, s.longitude), abs=1e-9)


def _check_table(t, model):
    recs, flags = t.aircraft()
    model.check(recs, t.last_heard(), flags)
    return recs


def _relay(oracle, seed, n_icaos, start_every, life, rate, icaos=None):
    """Aircraft k is heard from k x start_every for `life` seconds, about `rate` frames a second (even / odd position
    halves that always pair, some identification frames); ICAOs in random order.  -> time-ordered [(t, frame)]."""
    rng = np.random.default_rng(seed)
    if icaos is None:
        icaos = [int(x) for x in rng.choice(np.arange(0x100000, 0xF00000), size=n_icaos, replace=False)]
    out = []
    for k, icao in enumerate(icaos):
        t, odd = k * start_every + rng.uniform(0, 1.0 / rate), bool(rng.integers(0, 2))
        while t < k * start_every + life:
            if rng.random() < 0.15:
                out.append((t, ident_frame(oracle, icao, list(rng.integers(1, 27, size=8)))))
            else:
                out.append((t, _even_odd(oracle, icao, odd)))
                odd = not odd
            t += rng.uniform(0.5, 1.5) / rate
    out.sort(key=lambda x: x[0])
    return out


def _windows(traffic, sps, window):
    """time-ordered [(t, frame)] -> [(FRAME_DTYPE list, sample_base)] of `window` samples each."""
    samples = [round(t / sps) for t, _ in traffic]
    out, a = [], 0
    for u in range(samples[-1] // window + 1):
        items = []
        while a < len(traffic) and samples[a] < (u + 1) * window:
            items.append((samples[a] - u * window, traffic[a][1]))
            a += 1
        out.append((_frames(items), u * window))
    return out


# ---- 1. an expire that evicts nothing ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_expire_below_every_last_heard_changes_nothing(gpu, oracle):
    sps, window = 1e-3, 500
    lists = _windows(_relay(oracle, 5, 40, 0.5, 6.0, 4.0), sps, window)
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_frames=1 << 10, seconds_per_sample=sps) as t, \
            A.TrackTable(d, max_frames=1 << 10, seconds_per_sample=sps) as twin:
        for u, (frames, base) in enumerate(lists):
            for x in (t, twin):
                x.update(frames, base)
            assert t.points().tobytes() == twin.points().tobytes()
            if u % 3 == 2:
                lh = t.last_heard()
                t.expire(float(lh.min()) if len(lh) else 0.0)    # strict: the oldest survives
                t.expire(-math.inf)
                recs, flags = t.aircraft()
                wrecs, wflags = twin.aircraft()
                assert recs.tobytes() == wrecs.tobytes() and flags == wflags == 0
                assert t.last_heard().tobytes() == twin.last_heard().tobytes()
        assert len(t.aircraft()[0]) >= 10


# ---- 2. streaming through the feed, against the oracle ---------------------------------------------------------
def _coming_and_going(oracle, seed, span_s):
    """random_traffic whose aircraft are heard in two spells with a gap between them (a return after 3-25 s)."""
    traffic = random_traffic(oracle, seed=seed, n_aircraft=40, n_frames=5000, span_s=span_s)
    rng = np.random.default_rng(seed + 1)
    spells = {}
    for icao in sorted({_icao_of(fr) for _, fr in traffic}):
        a = rng.uniform(-0.2, 0.6) * span_s
        b = a + rng.uniform(0.1, 0.4) * span_s
        c = b + rng.uniform(3.0, 25.0)
        spells[icao] = ((a, b), (c, c + rng.uniform(0.1, 0.4) * span_s))
    return [(t, fr) for t, fr in traffic
            if any(lo <= t < hi for lo, hi in spells[_icao_of(fr)])]


@pytest.mark.gpu
def test_streaming_expire_equals_oracle(gpu, oracle):
    """Modulated traffic through the per-buffer feed in 20 000-sample buffers (1 s each); every 3 buffers an expire
    with before = now - max_age.  Every point and, after every expire, the whole table equal the model; with 2 s, pairs
    that the never-expiring table completes are lost."""
    from tests.golden.make_golden import modulate, place
    chunk, span = 20_000, 60.0
    sps = 1.0 / chunk
    traffic = _coming_and_going(oracle, 51, span)
    at, last = [], -400
    for t, _ in traffic:                                 # the traffic's own times, 400 samples apart at least
        last = max(300 + round(t / sps), last + 400)
        if last % chunk > chunk - 300:                   # no frame across a buffer edge (per-buffer feed)
            last += chunk - last % chunk + 50
        at.append(last)
    n = at[-1] + 600
    iq = place(n, [(s, modulate(fr, (80, 30), None)) for s, (_, fr) in zip(at, traffic)], np.int8, floor=3, seed=51)
    popped = []
    with A.AdsbDemod(max_samples=chunk, max_out=1 << 12) as d, A.Feed(d, max_chunk=chunk, carry=False) as f:
        for a in range(0, n, chunk):
            b = min(a + chunk, n)
            if b - a < A.WINDOW:
                break
            f.push(iq[a:b])
            if f.in_flight == 2:
                popped.append(f.pop())
        while f.in_flight:
            popped.append(f.pop())
        assert all(flags == 0 for _, flags, _ in popped)
        assert sum(len(fr) for fr, _, _ in popped) >= len(traffic) - 5
        ages = (None, 2.0, 12.0, 60.0)
        models = [Model(oracle, sps) for _ in ages]
        pts_of = {m: [] for m in ages}
        with contextlib.ExitStack() as es:
            tables = [es.enter_context(A.TrackTable(d, max_frames=1 << 12, seconds_per_sample=sps)) for _ in ages]
            for k, (frames, _, first) in enumerate(popped):
                for age, t, m in zip(ages, tables, models):
                    t.update(frames, first)
                    pts = t.points()
                    _check_points(pts, m.update(frames, first))
                    pts_of[age].append(pts)
                    if age is not None and k % 3 == 2:
                        before = (first + chunk) * sps - age
                        t.expire(before)
                        m.expire(before)
                        _check_table(t, m)
            for t, m in zip(tables, models):
                _check_table(t, m)
    never = np.concatenate(pts_of[None])["flags"] & NEW != 0
    lost = {age: int((never & (np.concatenate(pts_of[age])["flags"] & NEW == 0)).sum()) for age in ages[1:]}
    assert int(never.sum()) > 300 and lost[2.0] >= 1, lost
    assert lost[12.0] == lost[60.0] == 0, lost          # an aircraft silent for > 10 s has no partner to lose
    assert len(models[0].ac) > len(models[1].ac)


# ---- 3. capacity ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_expiry_keeps_a_small_table_open(gpu, oracle):
    """max_aircraft = 16 and 220 ICAOs, at most about 12 heard in any 2.5 s: with an expire (max_age 2 s) after every
    0.5 s update nobody is turned away; a twin without expiry fills up."""
    sps, window, age = 1e-3, 500, 2.0
    lists = _windows(_relay(oracle, 9, 220, 0.5, 4.0, 4.0), sps, window)
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_aircraft=16, max_frames=1 << 10, seconds_per_sample=sps) as t, \
            A.TrackTable(d, max_aircraft=16, max_frames=1 << 10, seconds_per_sample=sps) as twin:
        m, mt = Model(oracle, sps, 16), Model(oracle, sps, 16)
        n_untracked = 0
        for frames, base in lists:
            t.update(frames, base)
            twin.update(frames, base)
            pts = t.points()
            assert not (pts["flags"] & UNTRACKED).any()
            _check_points(pts, m.update(frames, base))
            tp = twin.points()
            _check_points(tp, mt.update(frames, base))
            n_untracked += int((tp["flags"] & UNTRACKED != 0).sum())
            before = (base + window) * sps - age
            t.expire(before)
            m.expire(before)
            _check_table(t, m)
        assert t.aircraft()[1] == 0 and m.max_size <= 16
        recs = _check_table(twin, mt)
        assert twin.aircraft()[1] == FULL and len(recs) == 16 and n_untracked > 100


@pytest.mark.gpu
def test_admission_after_expire_takes_the_lowest_new_icaos(gpu, oracle):
    """About 20 aircraft live at once for 16 places: after each expire the next update admits its lowest new ICAOs
    while there is room, as the capacity model over the oracle trackers does."""
    sps, window, age = 1e-3, 500, 1.0
    lists = _windows(_relay(oracle, 13, 150, 0.2, 4.0, 4.0), sps, window)
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_aircraft=16, max_frames=1 << 10, seconds_per_sample=sps) as t:
        m = Model(oracle, sps, 16)
        for u, (frames, base) in enumerate(lists):
            t.update(frames, base)
            _check_points(t.points(), m.update(frames, base))
            if u % 2 == 1:
                before = (base + window) * sps - age
                t.expire(before)
                m.expire(before)
                _check_table(t, m)
        assert m.full == FULL and m.n_partial >= 5, m.n_partial


# ---- 4. cuts ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cuts_between_expires_give_the_same_result(gpu, oracle):
    sps, age = 1e-3, 0.25                               # frames 0.1-0.3 s apart: live aircraft get evicted too
    traffic = _relay(oracle, 17, 60, 0.5, 5.0, 5.0)
    whole = _frames([(round(t / sps), fr) for t, fr in traffic])
    cut_at = list(range(2000, round(traffic[-1][0] / sps) + 2000, 2000))   # an expire every 2 s
    rng = np.random.default_rng(3)
    results = []
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_frames=1 << 12, seconds_per_sample=sps) as t:
        for rep in range(3):
            t.reset()
            pts, tables, a = [], [], 0
            for edge in cut_at:
                b = int(np.searchsorted(whole["offset"], edge))
                while a < b:                                  # rep 0: one update per interval; else random pieces
                    sz = b - a if rep == 0 else int(rng.integers(1, 40))
                    part = whole[a:min(a + sz, b)].copy()
                    base = int(part["offset"][0])
                    part["offset"] -= base
                    t.update(part, base)
                    pts.append(t.points())
                    a += len(part)
                t.expire(edge * sps - age)
                recs, flags = t.aircraft()
                tables.append((recs.tobytes(), t.last_heard().tobytes(), flags))
            results.append((np.concatenate(pts).tobytes(), tables))
    assert results[1] == results[0] and results[2] == results[0]


# ---- 5. edges ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_expire_edges(gpu, oracle):
    sps = 1e-3
    A_, B_, C_ = 0x123456, 0x234567, 0x345678
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_aircraft=2, max_frames=16, seconds_per_sample=sps) as t:
        t.expire(1e9)                                         # an empty table
        t.expire(-math.inf)
        assert len(t.aircraft()[0]) == 0 and len(t.last_heard()) == 0
        t.update(_frames([(0, _even_odd(oracle, A_, False)), (500, ident_frame(oracle, B_, [1] * 8))]), 1000)
        assert list(t.last_heard()) == [1000 * sps, 1500 * sps]
        recs, _ = t.aircraft()
        assert math.isnan(recs[1]["last_contact"])           # identification only: no last_contact, still heard
        t.expire(1500 * sps)                                  # exactly at last_heard: survives; A (1.0 s) goes
        recs, flags = t.aircraft()
        assert [int(x) for x in recs["icao"]] == [B_] and flags == 0 and list(t.last_heard()) == [1500 * sps]
        t.expire(np.nextafter(1500 * sps, 2.0))               # the ID-only aircraft expires
        assert len(t.aircraft()[0]) == 0
        # everything expired: re-admission starts afresh, the even half from before is gone
        t.update(_frames([(0, _even_odd(oracle, A_, False))]), 3000)
        t.expire(math.inf)
        assert len(t.aircraft()[0]) == 0
        t.update(_frames([(0, _even_odd(oracle, A_, True))]), 3500)
        assert int(t.points()[0]["flags"]) == 0               # no pair with the evicted even half 0.5 s earlier
        recs, _ = t.aircraft()
        assert len(recs) == 1 and recs[0]["n_frames"] == 1 and not recs[0]["has_position"]
        # TABLE_FULL is kept by expire, cleared by reset; fetch_points is not touched by expire
        t.update(_frames([(0, _even_odd(oracle, B_, False)), (1, _even_odd(oracle, C_, False))]), 4000)
        pts_before = t.points()
        assert int(pts_before[1]["flags"]) == UNTRACKED and t.aircraft()[1] == FULL
        t.expire(math.inf)
        assert t.points().tobytes() == pts_before.tobytes()
        recs, flags = t.aircraft()
        assert len(recs) == 0 and flags == FULL
        t.update(_frames([(0, _even_odd(oracle, C_, False))]), 5000)
        t.expire(4.0)
        t.reset()                                             # reset after an expire
        recs, flags = t.aircraft()
        assert len(recs) == 0 and flags == 0
        t.update(_frames([(0, _even_odd(oracle, C_, True))]), 5100)
        assert int(t.points()[0]["flags"]) == 0 and list(t.last_heard()) == [5100 * sps]
        with pytest.raises(A.AdsbError) as e:
            t.expire(math.nan)
        assert e.value.code == A.ADSB_E_ARG
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, A.TrackBank(d, 3, max_frames=16) as bank:
        with pytest.raises(A.AdsbError) as e:
            bank.expire([0.0, math.nan, 0.0])
        assert e.value.code == A.ADSB_E_ARG
        with pytest.raises(ValueError):
            bank.expire([0.0, 1.0])
        bank.expire(-math.inf)
        assert [len(x) for x in bank.last_heard()] == [0, 0, 0]


# ---- 6. the bank ------------------------------------------------------------------------------------------------
SHARED = [0x3ABCDE, 0xA00011, 0xC0FFEE]


@pytest.mark.gpu
@pytest.mark.parametrize("n_receivers,seed", [(1, 1), (3, 2), (8, 3), (64, 4)])
def test_bank_expire_equals_tables_and_model(gpu, oracle, n_receivers, seed):
    """Per-receiver cuts (some -inf) and the same ICAOs on every receiver with other fates: receiver r is bit-identical
    to table r given the same updates and expire calls, and equal to the model."""
    R, sps, window = n_receivers, 1e-3, 500
    streams = []
    for r in range(R):
        rng = np.random.default_rng(100 * seed + r)
        icaos = [int(x) for x in rng.choice(np.arange(0x100000, 0xF00000), size=12 if R == 64 else 30, replace=False)]
        icaos[1:1 + len(SHARED) * 2:2] = SHARED               # the shared ICAOs start at other times per receiver
        streams.append(_windows(_relay(oracle, 100 * seed + r, 0, 0.4 + 0.1 * (r % 3), 3.0, 3.0 + r % 4,
                                       icaos=icaos), sps, window))
    n_upd = max(len(s) for s in streams)
    ages = [-1.0 if r % 4 == 3 else 0.5 + 0.75 * (r % 4) for r in range(R)]   # -1: never (-inf)
    models = [Model(oracle, sps) for _ in range(R)]
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackBank(d, R, max_frames=1 << 12, seconds_per_sample=sps) as bank, contextlib.ExitStack() as es:
        tables = [es.enter_context(A.TrackTable(d, max_frames=1 << 10, seconds_per_sample=sps)) for _ in range(R)]
        n_evicted = 0
        for u in range(n_upd):
            lists = [s[u][0] if u < len(s) else _frames([]) for s in streams]
            bases = [u * window + 7 * r for r in range(R)]
            bank.update(_concat(lists), [len(x) for x in lists], bases)
            pts = bank.points()
            a = 0
            for r in range(R):
                tables[r].update(lists[r], bases[r])
                want = tables[r].points()
                assert pts[a:a + len(want)].tobytes() == want.tobytes(), r
                if R <= 8 or r % 8 == 0:
                    _check_points(want, models[r].update(lists[r], bases[r]))
                else:
                    models[r].update(lists[r], bases[r])
                a += len(want)
            if u % 2 == 1:
                now = (u + 1) * window * sps
                before = [-math.inf if ages[r] < 0 else now - ages[r] for r in range(R)]
                bank.expire(before)
                for r in range(R):
                    tables[r].expire(before[r])
                    n_evicted += len(models[r].ac)
                    models[r].expire(before[r])
                    n_evicted -= len(models[r].ac)
                recs, flags = bank.aircraft()
                lh = bank.last_heard()
                for r in range(R):
                    trecs, tflags = tables[r].aircraft()
                    assert recs[r].tobytes() == trecs.tobytes() and flags[r] == tflags, r
                    assert lh[r].tobytes() == tables[r].last_heard().tobytes(), r
                    if R <= 8 or r % 8 == 0:
                        models[r].check(recs[r], lh[r], flags[r])
        assert n_evicted > 5 * R
        recs, _ = bank.aircraft()
        lh = bank.last_heard()
        for r in range(R):
            models[r].check(recs[r], lh[r], 0)


def _bank_hash(key):
    """fmix64, as adsb_track.hip's bank_hash"""
    m = (1 << 64) - 1
    x = key
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & m
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & m
    x ^= x >> 33
    return x


@pytest.mark.gpu
def test_bank_hash_survives_churn(gpu, oracle):
    """max_aircraft = 4 on 2 receivers: a 16-entry hash.  600 cycles of updates and expires over recurring ICAOs whose
    keys share a few home buckets: a stale or broken probe chain would lose or duplicate an aircraft."""
    R, sps, cap = 2, 1e-3, 16
    cands = range(0x400000, 0x400000 + 4000)
    pools = [[i for i in cands if _bank_hash(r << 24 | i) & (cap - 1) in (3, 4)][:7] for r in range(R)]
    assert all(len(p) == 7 for p in pools)
    rng = np.random.default_rng(77)
    models = [Model(oracle, sps, 4) for _ in range(R)]
    n_readmit, seen = 0, [set() for _ in range(R)]
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackBank(d, R, max_aircraft=4, max_frames=64, seconds_per_sample=sps) as bank:
        for u in range(600):
            lists = []
            for r in range(R):
                pick = rng.choice(pools[r], size=int(rng.integers(0, 4)), replace=False)
                items = []
                for k, icao in enumerate(pick):
                    fr = ident_frame(oracle, int(icao), [5] * 8) if rng.random() < 0.2 else \
                        _even_odd(oracle, int(icao), bool(rng.integers(0, 2)))
                    items.append((k, fr))
                    n_readmit += int(icao) in seen[r] and int(icao) not in models[r].ac
                    seen[r].add(int(icao))
                lists.append(_frames(items))
            bases = [u * 100] * R
            bank.update(_concat(lists), [len(x) for x in lists], bases)
            pts = bank.points()
            a = 0
            for r in range(R):
                _check_points(pts[a:a + len(lists[r])], models[r].update(lists[r], bases[r]))
                a += len(lists[r])
            before = [u * 100 * sps - float(rng.integers(0, 4)) * 0.1 for _ in range(R)]
            bank.expire(before)
            for r in range(R):
                models[r].expire(before[r])
            recs, flags = bank.aircraft()
            lh = bank.last_heard()
            for r in range(R):
                models[r].check(recs[r], lh[r], flags[r])
    assert n_readmit >= 300, n_readmit


@pytest.mark.gpu
def test_update_launch_then_expire(gpu, oracle):
    """A 3-channel launch per step through update_launch, then an expire: the same as a bank fed the fetched host
    lists with the same expire calls, and equal to the model per receiver."""
    import torch

    from tests.golden.make_golden import modulate, place
    C_, n, stride, R = 3, 20_000, 20_480, 3
    sps = 1.0 / n                                    # a launch spans 1 s
    streams = [iter(random_traffic(oracle, seed=300 + c, n_aircraft=30, n_frames=2000)) for c in range(C_)]
    models = [Model(oracle, sps) for _ in range(R)]
    n_evicted = 0
    with A.AdsbDemod(max_samples=n, max_out=512, max_channels=C_, host_staging=False) as d, \
            A.TrackBank(d, R, max_frames=512, seconds_per_sample=sps) as bank, \
            A.TrackBank(d, R, max_frames=512, seconds_per_sample=sps) as host_bank:
        for launch in range(12):
            host = np.full((C_, stride, 2), 77, dtype=np.int8)
            for c in range(C_):
                k_frames = 10 if c == 1 and launch % 3 == 0 else 30
                items = [(300 + 600 * k, modulate(next(streams[c])[1], (80, 30), None)) for k in range(k_frames)]
                host[c, :n] = place(n, items, np.int8, floor=3, seed=100 * launch + c)
            buf = torch.from_numpy(host).cuda()
            d.demod_device_async(buf.data_ptr(), n, C_, stride)
            bases = [launch * n + r for r in range(R)]
            bank.update_launch(bases)
            frames, counts, _, flags = d.fetch(n_channels=C_)
            assert flags == 0
            host_bank.update(frames, [int(x) for x in counts], bases)
            pts = bank.points()
            assert pts.tobytes() == host_bank.points().tobytes()
            a = 0
            for r in range(R):
                _check_points(pts[a:a + int(counts[r])], models[r].update(frames[a:a + int(counts[r])], bases[r]))
                a += int(counts[r])
            before = [(launch + 1) * n * sps - age for age in (1.5, 3.0, math.inf)]
            before[2] = -math.inf
            bank.expire(before)
            host_bank.expire(before)
            for r in range(R):
                n_evicted += len(models[r].ac)
                models[r].expire(before[r])
                n_evicted -= len(models[r].ac)
            recs, bflags = bank.aircraft()
            hrecs, _ = host_bank.aircraft()
            assert all(x.tobytes() == y.tobytes() for x, y in zip(recs, hrecs))
            lh = bank.last_heard()
            assert all(x.tobytes() == y.tobytes() for x, y in zip(lh, host_bank.last_heard()))
            for r in range(R):
                models[r].check(recs[r], lh[r], bflags[r])
    assert n_evicted > 20
