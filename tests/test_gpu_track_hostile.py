"""The device tracker (adsb_track_device, TrackTable, TrackBank: air_rs_amd/csrc/adsb_track.hip) on hostile traffic
(tests/hostile_traffic.py): CPR pairs chosen for every branch of cpr.rs, partners exactly at the 10 s window at the
radio's real sample periods and at stream positions up to beyond 2^53, every kind of message, the segment shapes of the
sort by ICAO, and one launch-sized list.  The yardstick is the oracle's sequential restatement of aircraft.rs fed the
same frames at the same times, float(sample_base + offset) * seconds_per_sample; tests/test_hostile_traffic.py holds the
census conditions that prove the cases are reached.

Flags, ICAOs, counts, callsigns, altitudes and has_position compare exactly; positions and stored times within the 1e-9
of the other device-versus-oracle tests (device libm against host libm); "the same bytes" is tobytes() equality."""
import contextlib
import math

import numpy as np
import pytest

import air_rs_amd as A
from tests import fuse_model
from tests import hostile_traffic as H
from tests import velocity_traffic
from tests.test_gpu_track_expire import Model
from tests.test_gpu_track_table import _same_table
from tests.traffic import position_frame

SEED = 101                                       # tests/test_hostile_traffic.py checks the census of this seed
SPS = 0.5e-6                                     # 2 MSPS, the value in use
TOL = 1e-9
NEW, UNTRACKED = A.ADSB_TRACK_NEW_POSITION, A.ADSB_TRACK_UNTRACKED


def _case(traffic, k):
    return H.CASES[int(traffic.case[k])]


def _replay(oracle, frames, times):
    """The oracle over one list: (new flags, AIRCRAFT_DTYPE summaries with the running frame count, point
    latitudes / longitudes (0 unless new), the tracker)."""
    n = len(frames)
    new = np.zeros(n, dtype=bool)
    sums = np.zeros(n, dtype=A.AIRCRAFT_DTYPE)
    pos = np.zeros((n, 2))
    ot, count = oracle.tracker(), {}
    rows = []
    for k, (fr, t) in enumerate(zip(frames, times.tolist())):
        got, s = ot.update(bytes(fr), t)
        count[s.icao] = count.get(s.icao, 0) + 1
        new[k] = got
        if got:
            pos[k] = (s.latitude, s.longitude)
        rows.append((s.latitude, s.longitude, s.last_contact, s.icao, s.altitude, s.has_position, count[s.icao],
                     s.callsign))
    if rows:
        sums[:] = rows
    return new, sums, pos, ot


def _first_bad(ok):
    return int(np.flatnonzero(~ok)[0])


def _close(a, b):
    return (np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= TOL)


def _same_points(pts, icao, new, pos, name):
    """Device points against the oracle's: ICAO and flags exactly, positions within TOL; a failure names the case."""
    assert len(pts) == len(new)
    ok = (pts["icao"] == icao) & (pts["flags"] == np.where(new, NEW, 0)) & \
        _close(pts["latitude"], pos[:, 0]) & _close(pts["longitude"], pos[:, 1])
    assert ok.all(), (_first_bad(ok), name(_first_bad(ok)), pts[_first_bad(ok)], new[_first_bad(ok)],
                      pos[_first_bad(ok)], int((~ok).sum()))


def _same_summaries(got, want, name):
    assert len(got) == len(want)
    ok = np.ones(len(got), dtype=bool)
    for f in ("icao", "callsign", "altitude", "has_position", "n_frames"):
        ok &= got[f] == want[f]
    for f in ("latitude", "longitude", "last_contact"):
        ok &= _close(got[f], want[f])
    assert ok.all(), (_first_bad(ok), name(_first_bad(ok)), got[_first_bad(ok)], want[_first_bad(ok)], int((~ok).sum()))


def _counts(icao):
    return dict(zip(*(x.tolist() for x in np.unique(icao, return_counts=True))))


@pytest.fixture(scope="module")
def traffic(oracle):
    return H.hostile_traffic(oracle, SEED, SPS)


@pytest.fixture(scope="module")
def replayed(oracle, traffic):
    return _replay(oracle, traffic.frames, traffic.times())


# ---- 1. one update against the oracle, frame by frame ------------------------------------------------------------------
@pytest.mark.gpu
def test_one_update_equals_oracle(gpu, oracle, traffic, replayed):
    new, sums, pos, ot = replayed
    assert int(new.sum()) > 2000
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_frames=1 << 14, seconds_per_sample=SPS) as t:
        t.summaries_reserve()
        t.update(traffic.frame_array(A.FRAME_DTYPE))
        _same_points(t.points(), traffic.icao, new, pos, lambda k: _case(traffic, k))
        _same_summaries(t.summaries(), sums, lambda k: _case(traffic, k))
        recs, flags = t.aircraft()
        assert flags == 0 and recs[0]["icao"] == 0 and recs[-1]["icao"] == 0xFFFFFF
        _same_table(recs, sorted(ot.aircraft(), key=lambda s: s.icao), _counts(traffic.icao))
        last = {int(i): k for k, i in enumerate(traffic.icao)}               # the last frame's summary is the record
        rows = np.array([last[int(i)] for i in recs["icao"]])
        assert t.summaries()[rows].tobytes() == recs.tobytes()


@pytest.mark.gpu
def test_cpr_sweep_equals_oracle(gpu, oracle, traffic):
    """The device twin of test_host_cpr_equals_oracle: 20 000 aircraft with one even and one odd message each, uniform
    17-bit fields, both orders, plus the field sets the generator chose (refused pairs, the exact latitudes, folds,
    one- and two-zone latitudes, quirk hits, wrapped longitudes) in both orders, in ONE update; every flag and position
    against oracle.geographic_position."""
    rng = np.random.default_rng(5)
    fields = [tuple(int(x) for x in rng.integers(0, 1 << 17, size=4)) for _ in range(20000)]
    odd_first = [bool(x) for x in rng.integers(0, 2, size=20000)]
    for _, i, j in traffic.cpr_pairs[::2]:                                 # every chosen set once, then both orders
        pi, pj = oracle.packet_new(bytes(traffic.frames[i])), oracle.packet_new(bytes(traffic.frames[j]))
        e, o = (pj, pi) if pi.cpr_odd else (pi, pj)
        for order in (False, True):
            fields.append((e.cpr_latitude, e.cpr_longitude, o.cpr_latitude, o.cpr_longitude))
            odd_first.append(order)
    n = len(fields)
    f = np.array(fields, dtype=np.uint32)
    of = np.array(odd_first)
    icao = (np.arange(n, dtype=np.uint32) * 419 + 7) & 0xFFFFFF           # distinct (419 is odd), spread over the keys
    fr = np.zeros((2 * n, 14), dtype=np.uint8)
    fr[:, 0] = 0x8D
    both = np.repeat(icao, 2)
    fr[:, 1], fr[:, 2], fr[:, 3] = (both >> 16) & 0xFF, (both >> 8) & 0xFF, both & 0xFF
    odd = np.stack([of, ~of], axis=1).reshape(-1)                          # the first message's format, then the other
    lat = np.where(odd, np.repeat(f[:, 2], 2), np.repeat(f[:, 0], 2))
    lon = np.where(odd, np.repeat(f[:, 3], 2), np.repeat(f[:, 1], 2))
    fr[:, 4] = 11 << 3
    fr[:, 5] = 0x3A
    fr[:, 6] = 0x80 | (odd.astype(np.uint8) << 2) | ((lat >> 15) & 0x3)
    fr[:, 7] = (lat >> 7) & 0xFF
    fr[:, 8] = ((lat & 0x7F) << 1) | ((lon >> 16) & 0x1)
    fr[:, 9], fr[:, 10] = (lon >> 8) & 0xFF, lon & 0xFF
    H.seal(fr)
    p = oracle.packet_new(bytes(fr[1]))
    assert (p.cpr_latitude, p.cpr_longitude, p.cpr_odd) == (int(lat[1]), int(lon[1]), int(odd[1])) and p.msg_kind == 1
    frames = np.zeros(2 * n, dtype=A.FRAME_DTYPE)
    frames["bytes"], frames["fixed_bit"] = fr, 0xFF
    frames["offset"] = np.arange(2 * n, dtype=np.uint64) * 50             # 2 MSPS: the whole list spans 2 s
    new = np.zeros(2 * n, dtype=bool)
    pos = np.zeros((2 * n, 2))
    n_refused = 0
    for k in range(n):
        want = oracle.geographic_position(*fields[k], first_is_odd=odd_first[k])
        n_refused += want is None
        if want is not None:
            new[2 * k + 1], pos[2 * k + 1] = True, want
    assert n_refused >= 200 and int(new.sum()) >= 19000
    assert int((pos[:, 0] == 0.0).sum() - (~new).sum()) >= 20 and int((np.abs(pos[:, 0]) == 87.0).sum()) >= 40
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_frames=2 * n, seconds_per_sample=SPS) as t:
        t.update(frames)
        _same_points(t.points(), both, new, pos, lambda k: (fields[k // 2], odd_first[k // 2]))
        recs, flags = t.aircraft()
        assert flags == 0 and len(recs) == n and int(recs["has_position"].sum()) == int(new.sum())


@pytest.mark.gpu
def test_equal_offsets_apply_in_list_order(gpu, oracle):
    """What the header says of frames with equal offsets: list order.  An even and an odd message of one aircraft at
    the SAME offset, in both list orders (the newer format decides the latitude, so the two orders give other
    positions), four aircraft sharing each offset: the oracle fed in list order, in one update and frame by frame."""
    rng = np.random.default_rng(9)
    items = []
    for k in range(200):
        f = H.draw_fields(rng)
        while not H.decodes_both_orders(oracle, f):
            f = H.draw_fields(rng)
        pair = [position_frame(oracle, 0x600000 + k, False, f[0], f[1]),
                position_frame(oracle, 0x600000 + k, True, f[2], f[3])]
        items += [(1000 * (k // 4), fr) for fr in (pair[::-1] if k & 1 else pair)]
    items.sort(key=lambda x: x[0])                                         # stable: the pairs stay as written
    frames = np.zeros(len(items), dtype=A.FRAME_DTYPE)
    frames["offset"], frames["fixed_bit"] = [o for o, _ in items], 0xFF
    frames["bytes"] = np.frombuffer(b"".join(fr for _, fr in items), dtype=np.uint8).reshape(-1, 14)
    icao = np.array([int.from_bytes(fr[1:4], "big") for _, fr in items], dtype=np.uint32)
    new, sums, pos, _ = _replay(oracle, frames["bytes"], frames["offset"].astype(np.float64) * SPS)
    assert int(new.sum()) == 200 and len({(round(a, 6), round(b, 6)) for a, b in pos[new]}) == 200
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_frames=1 << 10, seconds_per_sample=SPS) as t:
        t.summaries_reserve()
        t.update(frames)
        _same_points(t.points(), icao, new, pos, lambda k: k)
        _same_summaries(t.summaries(), sums, lambda k: k)
        whole = (t.points().tobytes(), _state(t))
        t.reset()
        parts = []
        for k in range(len(frames)):
            t.update(frames[k:k + 1])
            parts.append(t.points())
        assert (np.concatenate(parts).tobytes(), _state(t)) == whole


# ---- 2. any cut gives the same bytes -----------------------------------------------------------------------------------
def _state(t):
    recs, flags = t.aircraft()
    return recs.tobytes(), flags, t.last_heard().tobytes(), t.velocity().tobytes()


def _run_cuts(t, traffic, edges, rebase):
    """The list in the pieces [edges[k], edges[k + 1]); offsets absolute, or relative to each piece's first sample."""
    t.reset()
    pts, sums = [], []
    for a, b in zip(edges[:-1], edges[1:]):
        base = int(traffic.samples[a]) if rebase else 0
        t.update(traffic.frame_array(A.FRAME_DTYPE, a, b, base), base)
        pts.append(t.points())
        sums.append(t.summaries())
    return np.concatenate(pts).tobytes(), np.concatenate(sums).tobytes(), _state(t)


@pytest.mark.gpu
def test_any_cut_gives_the_same_bytes(gpu, oracle, traffic):
    n = len(traffic)
    rng = np.random.default_rng(7)
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_frames=1 << 14, seconds_per_sample=SPS) as t:
        t.summaries_reserve()
        whole = _run_cuts(t, traffic, [0, n], rebase=False)
        for rep in range(3):                                               # random cuts
            edges = sorted({0, n} | {int(x) for x in rng.integers(1, n, size=n // 100)})
            assert _run_cuts(t, traffic, edges, rebase=bool(rep & 1)) == whole, rep
        # exactly between the two halves of every window pair, and around every frame inside such a pair
        edges = {0, n}
        for p in traffic.window_pairs:
            edges |= {p["second"], p["first"] + 1} | set(p["inside"])
        assert len(edges) > 500
        assert _run_cuts(t, traffic, sorted(edges), rebase=False) == whole
        assert _run_cuts(t, traffic, sorted(edges), rebase=True) == whole
        # single frames: every pair of the CPR, window and message-mix cases is cut
        few = traffic.select(np.isin(traffic.case, [H.CASES.index(c) for c in H.CPR_CASES + H.WIN_CASES + ("mix",)]))
        assert 3000 <= len(few) <= 6000
        whole_few = _run_cuts(t, few, [0, len(few)], rebase=False)
        assert _run_cuts(t, few, list(range(len(few) + 1)), rebase=True) == whole_few


# ---- 3. the window at real sample periods ------------------------------------------------------------------------------
def _window_report(traffic, pts_of_second, sps):
    """{(case, region): disagreements} of the device's flag at the newer half of every window pair with
    not (abs(float(x_i) * sps - float(x_j) * sps) > 10.0) -- every pair's fields decode, so that is the whole flag."""
    bad = {}
    for p in traffic.window_pairs:
        want = not H.too_old(int(traffic.samples[p["second"]]), int(traffic.samples[p["first"]]), sps)
        if bool(pts_of_second[p["second"]] & NEW) != want:
            key = (p["case"], p["region"])
            bad[key] = bad.get(key, 0) + 1
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("sps", H.SAMPLE_PERIODS, ids=lambda s: f"{s:.4g}")
def test_window_at_real_sample_periods(gpu, oracle, sps):
    """Every window case (partners at round(10 / sps) samples and one less and more, near 0, across 2^40 and above
    2^53, bare and with other frames of the aircraft inside the window): both partners in one update, split across two
    updates with sample_base carrying the difference, and through a bank with one stream position per receiver.  The
    flag is the oracle's: the difference of the two ROUNDED times against 10.0.  On the parent of the commit that
    added this test (the walk's product contracted into a fused multiply-add) 44 / 45 / 45 / 0 of the 255 pairs
    disagreed at 0.5e-6 / 1/2.4e6 / 1e-3 / 2^-20 in one update and through the bank, none when split."""
    full = H.hostile_traffic(oracle, SEED, sps)
    tr = full.select(np.isin(full.case, [H.CASES.index(c) for c in H.WIN_CASES]))
    where = np.cumsum(np.isin(full.case, [H.CASES.index(c) for c in H.WIN_CASES])) - 1
    tr.window_pairs = [dict(p, first=int(where[p["first"]]), second=int(where[p["second"]]),
                            inside=[int(where[i]) for i in p["inside"]]) for p in full.window_pairs]
    n = len(tr)
    assert len(tr.window_pairs) >= 250 and n >= 900
    new, _, pos, ot = _replay(oracle, tr.frames, tr.times())
    exact = [p for p in tr.window_pairs if p["delta"] == 0]
    assert sum(bool(new[p["second"]]) for p in exact) >= 80               # the oracle accepts them (census: >= 40 bare)
    for p in tr.window_pairs:                                              # and the flag the test states is the oracle's
        assert bool(new[p["second"]]) == (not H.too_old(int(tr.samples[p["second"]]), int(tr.samples[p["first"]]), sps))
    # the three stream positions are three stretches of the list; each splits before its first newer half
    region_of = {}
    for p in tr.window_pairs:
        for k in [p["first"], p["second"]] + p["inside"]:
            region_of[k] = H.REGIONS.index(p["region"])
    region = np.array([region_of[k] for k in range(n)])
    assert (np.diff(region) >= 0).all()
    lo = [int(np.searchsorted(region, r)) for r in range(4)]
    cut = [min(p["second"] for p in tr.window_pairs if p["region"] == H.REGIONS[r]) for r in range(3)]
    assert all(max(p["first"] for p in tr.window_pairs if p["region"] == H.REGIONS[r]) < cut[r] for r in range(3))
    report, got = {}, {}
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_frames=1 << 12, seconds_per_sample=sps) as t, \
            A.TrackBank(d, 3, max_frames=1 << 12, seconds_per_sample=sps) as bank:
        t.update(tr.frame_array(A.FRAME_DTYPE))
        got["one update"] = (t.points(), _state(t))
        t.reset()
        parts = []
        for a, b in sorted(zip(lo[:3] + cut, cut + lo[1:])):
            base = int(tr.samples[a])
            t.update(tr.frame_array(A.FRAME_DTYPE, a, b, base), base)
            parts.append(t.points())
        got["split"] = (np.concatenate(parts), _state(t))
        bases = [int(tr.samples[lo[r]]) for r in range(3)]
        lists = [tr.frame_array(A.FRAME_DTYPE, lo[r], lo[r + 1], bases[r]) for r in range(3)]
        bank.update(np.concatenate(lists), [len(x) for x in lists], bases)
        got["bank"] = (bank.points(), None)
        bank.reset()
        parts = [[], [], []]
        for half in (0, 1):
            lists = [tr.frame_array(A.FRAME_DTYPE, (lo[r], cut[r])[half], (cut[r], lo[r + 1])[half],
                                    int(tr.samples[(lo[r], cut[r])[half]])) for r in range(3)]
            bank.update(np.concatenate(lists), [len(x) for x in lists],
                        [int(tr.samples[(lo[r], cut[r])[half]]) for r in range(3)])
            pts, a = bank.points(), 0
            for r in range(3):
                parts[r].append(pts[a:a + len(lists[r])])
                a += len(lists[r])
        got["bank split"] = (np.concatenate([np.concatenate(x) for x in parts]), None)
    for mode, (pts, _) in got.items():
        report[mode] = _window_report(tr, pts["flags"], sps)
    print(f"\nwindow pairs whose flag is not the oracle's, sps = {sps!r}, of {len(tr.window_pairs)}: " +
          "; ".join(f"{mode}: {sum(bad.values())} {bad}" for mode, bad in report.items()))
    assert all(not bad for bad in report.values()), report
    for mode, (pts, state) in got.items():
        _same_points(pts, tr.icao, new, pos, lambda k: (mode, _case(tr, k)))
    assert got["split"][1] == got["one update"][1]
    _same_table(np.frombuffer(got["split"][1][0], dtype=A.AIRCRAFT_DTYPE),
                sorted(ot.aircraft(), key=lambda s: s.icao), _counts(tr.icao))


# ---- 4. the per-launch tracker over the demodulator's own list ---------------------------------------------------------
@pytest.mark.gpu
def test_per_launch_tracker_equals_oracle(gpu, oracle, traffic):
    """The DF 17 part of the CPR, window and message-mix cases, modulated and demodulated as
    test_device_tracker_equals_oracle does: d.track(sps) against the oracle, and a table's update_device the same
    bytes."""
    from tests.golden.make_golden import modulate, place
    pick = np.isin(traffic.case, [H.CASES.index(c) for c in H.CPR_CASES + H.WIN_CASES + ("mix",)]) & \
        (traffic.frames[:, 0] >> 3 == 17)
    sent = traffic.frames[pick]
    assert 4000 <= len(sent) <= 6000 and len({int(b) for b in sent[:, 0]}) >= 3    # 0x8D and other capabilities
    gap = 400
    n = 300 + gap * len(sent) + 600
    sps = 80.0 / (gap * len(sent))                                         # 10 s = 1/8 of the list
    items = [(300 + gap * k, modulate(bytes(fr), (80, 30), None)) for k, fr in enumerate(sent)]
    iq = place(n, items, np.int8, floor=3, seed=SEED)
    with A.AdsbDemod(max_samples=n, max_out=1 << 13) as d:
        frames, flags = d.demod(iq)
        assert flags == 0 and len(frames) >= len(sent)
        points, aircraft = d.track(sps)
        n_out, _, _ = d.fetch_counts()
        frames_dev, _ = d.result_device()
        with A.TrackTable(d, max_frames=1 << 13, seconds_per_sample=sps) as t:
            t.update_device(frames_dev, n_out)
            assert t.points().tobytes() == points.tobytes()
            recs, tflags = t.aircraft()
            assert tflags == 0 and recs.tobytes() == aircraft.tobytes()
    icao = (frames["bytes"][:, 1].astype(np.uint32) << 16) | (frames["bytes"][:, 2].astype(np.uint32) << 8) | \
        frames["bytes"][:, 3]
    times = frames["offset"].astype(np.float64) * sps
    assert H.largest_window_count(icao, times) <= H.MAX_IN_WINDOW
    new, _, pos, ot = _replay(oracle, frames["bytes"], times)
    tc = frames["bytes"][:, 4] >> 3
    assert int(new.sum()) > 500 and int((~new & (tc >= 9) & (tc <= 18)).sum()) > 1000    # first halves, refused pairs
    _same_points(points, icao, new, pos, lambda k: bytes(frames["bytes"][k]).hex())
    _same_table(aircraft, sorted(ot.aircraft(), key=lambda s: s.icao), _counts(icao))


# ---- 5. a bank's receiver = a table of its own -------------------------------------------------------------------------
def _deal(traffic, n_receivers):
    """One index array per receiver: every ICAO on one receiver by a hash, the special ICAOs (000000, FFFFFF, 7FFFFF,
    800000) on receiver 0 and on the last one, the message-mix aircraft on every receiver."""
    r_of = ((traffic.icao.astype(np.uint64) * np.uint64(2654435761)) >> np.uint64(11)) % np.uint64(n_receivers)
    special, mix = traffic.case == H.CASES.index("seg_special"), traffic.case == H.CASES.index("mix")
    return [np.flatnonzero(mix | (special & (r in (0, n_receivers - 1))) | (~mix & ~special & (r_of == r)))
            for r in range(n_receivers)]


def _lists(traffic, deal, a, b, bases):
    """Receiver r's frames with list index in [a, b), offsets relative to bases[r]"""
    out = []
    for idx, base in zip(deal, bases):
        idx = idx[(idx >= a) & (idx < b)]
        fr = np.zeros(len(idx), dtype=A.FRAME_DTYPE)
        fr["offset"], fr["bytes"], fr["fixed_bit"] = traffic.samples[idx] - np.uint64(base), traffic.frames[idx], 0xFF
        out.append(fr)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n_receivers", [1, 3, 8, 64])
def test_bank_equals_separate_tables(gpu, oracle, traffic, n_receivers):
    R, n = n_receivers, len(traffic)
    deal = _deal(traffic, R)
    assert all(len(x) >= 1440 for x in deal) and sum(len(x) for x in deal) >= n
    edges = [0, n // 5, n // 5 + 1, n // 2, n - 300, n]                    # the last update holds the 2^40 and 2^53 parts
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackBank(d, R, max_frames=1 << 17, seconds_per_sample=SPS) as bank, contextlib.ExitStack() as es:
        tables = [es.enter_context(A.TrackTable(d, max_frames=1 << 14, seconds_per_sample=SPS)) for _ in range(R)]
        for a, b in zip(edges[:-1], edges[1:]):
            bases = [max(int(traffic.samples[a]) - 3 * r, 0) for r in range(R)]
            lists = _lists(traffic, deal, a, b, bases)
            bank.update(np.concatenate(lists), [len(x) for x in lists], bases)
            pts, at = bank.points(), 0
            for r, t in enumerate(tables):
                t.update(lists[r], bases[r])
                want = t.points()
                assert pts[at:at + len(want)].tobytes() == want.tobytes(), r
                at += len(want)
            assert at == len(pts)
        recs, flags = bank.aircraft()
        heard, vel = bank.last_heard(), bank.velocity()
        for r, t in enumerate(tables):
            trecs, tflags = t.aircraft()
            assert recs[r].tobytes() == trecs.tobytes() and flags[r] == tflags == 0, r
            assert heard[r].tobytes() == t.last_heard().tobytes() and vel[r].tobytes() == t.velocity().tobytes(), r
        assert recs[0][0]["icao"] == recs[-1][0]["icao"] == 0 and recs[0][-1]["icao"] == recs[-1][-1]["icao"] == 0xFFFFFF
        assert all(int((v["subtype"] != 0).sum()) >= 8 for v in vel)         # the mix aircraft, on every receiver


# ---- 6. summaries, changed list, velocity, expire and fuse in one streaming run ----------------------------------------
@pytest.mark.gpu
def test_streaming_summaries_velocity_expire_fuse(gpu, oracle, traffic):
    """A 3-receiver bank with a summaries reserve over the dealt traffic in 24 updates, an expire (max age 15 s, on
    receiver 2 never) after every second one: points and summaries against the expire model over oracle trackers after
    every frame, the changed list = the touched records, velocity = velocity_traffic.decode of each aircraft's last
    TC 19 message of its lifetime, fuse() = tests/fuse_model.py, the table against the model after every expire."""
    R, n, age = 3, len(traffic), 15.0
    deal = _deal(traffic, R)
    models = [Model(oracle, SPS) for _ in range(R)]
    counts, vel_of = [{} for _ in range(R)], [{} for _ in range(R)]
    edges = [int(x) for x in np.linspace(0, n - 600, 22)] + [n - 300, n - 299, n]
    n_vel = n_evicted = n_frames = 0
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackBank(d, R, max_frames=1 << 15, seconds_per_sample=SPS) as bank:
        bank.summaries_reserve()
        for u, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
            bases = [max(int(traffic.samples[a]) - 5 * r, 0) for r in range(R)]
            lists = _lists(traffic, deal, a, b, bases)
            bank.update(np.concatenate(lists), [len(x) for x in lists], bases)
            pts, sums = bank.points(), bank.summaries()
            crecs, cheard, cvel, ccounts = bank.changed()
            recs, flags = bank.aircraft()
            heard, vel = bank.last_heard(), bank.velocity()
            at = cat = 0
            for r in range(R):
                fr = lists[r]
                want = models[r].update(fr, bases[r])
                new = np.array([w[1] for w in want], dtype=bool)
                pos = np.array([(w[2].latitude, w[2].longitude) if w[1] else (0.0, 0.0) for w in want]).reshape(-1, 2)
                rows = []
                for k, (icao, _, s) in enumerate(want):
                    counts[r][icao] = counts[r].get(icao, 0) + 1
                    rows.append((s.latitude, s.longitude, s.last_contact, s.icao, s.altitude, s.has_position,
                                 counts[r][icao], s.callsign))
                    v = velocity_traffic.decode(bytes(fr[k]["bytes"]), float(bases[r] + int(fr[k]["offset"])) * SPS)
                    if v is not None:
                        vel_of[r][icao] = v
                        n_vel += 1
                wsum = np.zeros(len(fr), dtype=A.AIRCRAFT_DTYPE)
                if rows:
                    wsum[:] = rows
                icao = np.array([w[0] for w in want], dtype=np.uint32)
                _same_points(pts[at:at + len(fr)], icao, new, pos, lambda k: (u, r, hex(int(icao[k]))))
                _same_summaries(sums[at:at + len(fr)], wsum, lambda k: (u, r, hex(int(icao[k]))))
                at += len(fr)
                n_frames += len(fr)
                touched = np.unique(icao)                                  # the changed list: the touched records
                assert ccounts[r] == len(touched) and list(crecs["icao"][cat:cat + ccounts[r]]) == list(touched)
                rows_of = np.searchsorted(recs[r]["icao"], touched)
                assert crecs[cat:cat + ccounts[r]].tobytes() == recs[r][rows_of].tobytes()
                assert cheard[cat:cat + ccounts[r]].tobytes() == heard[r][rows_of].tobytes()
                assert cvel[cat:cat + ccounts[r]].tobytes() == vel[r][rows_of].tobytes()
                cat += ccounts[r]
                models[r].check(recs[r], heard[r], flags[r])
                for rec, v in zip(recs[r], vel[r]):                        # velocity, per lifetime
                    want_v = vel_of[r].get(int(rec["icao"]), velocity_traffic.empty())
                    assert v.tobytes() == want_v.tobytes(), (u, r, hex(int(rec["icao"])), v, want_v)
            assert at == len(pts) == len(sums) and cat == len(crecs)
            got, total, fflags = bank.fuse()                               # the fused view of what the bank holds now
            want_f = fuse_model.fuse(recs, heard, vel)
            assert total == len(got) and fflags == 0 and got.tobytes() == want_f.tobytes(), u
            if u % 2 == 1:
                now = float(int(traffic.samples[b - 1])) * SPS
                before = [now - age, now - age, -math.inf]
                bank.expire(before)
                for r in range(R):
                    size = len(models[r].ac)
                    models[r].expire(before[r])
                    n_evicted += size - len(models[r].ac)
                    for gone in set(counts[r]) - set(models[r].ac):
                        del counts[r][gone]
                        vel_of[r].pop(gone, None)
                recs, flags = bank.aircraft()
                heard = bank.last_heard()
                for r in range(R):
                    models[r].check(recs[r], heard[r], flags[r])
                cut = now - 2 * age
                got, _, _ = bank.fuse(since=cut)
                assert got.tobytes() == fuse_model.fuse(recs, heard, bank.velocity(), cut).tobytes(), u
    assert n_frames >= n and n_vel >= 3 * 100 and n_evicted >= 1000, (n_frames, n_vel, n_evicted)
    assert len(models[2].ac) > len(models[0].ac)


# ---- 7. a launch-sized list --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_launch_sized_list(gpu, oracle):
    """At least 2^18 frames from at least 4096 aircraft in ONE update of a table with a summaries reserve (one segment
    of 2^15 frames, 1000 aircraft heard once, 1900 in a Zipf-like spread, the named cases, at most 256 frames of one
    aircraft in any 10 s window): points and summaries against the oracle frame by frame; the same list in cuts of
    1 << 12, 1 << 16 and the rest, the same bytes; dealt to an 8-receiver bank, the bytes of 8 tables.  Results only."""
    big = H.hostile_traffic(oracle, SEED + 1, SPS, span_s=2400.0, n_single=1000, n_big=1 << 15, n_zipf_aircraft=1900,
                            n_zipf_frames=223_100)
    n = len(big)
    lengths = np.unique(big.icao, return_counts=True)[1]
    assert n >= 1 << 18 and len(lengths) >= 4096 and lengths.max() >= 1 << 15 and int((lengths == 1).sum()) >= 1000
    new, sums, pos, ot = _replay(oracle, big.frames, big.times())
    assert int(new.sum()) > 30_000
    frames = big.frame_array(A.FRAME_DTYPE)
    with A.AdsbDemod(max_samples=4096, max_out=64) as d:
        with A.TrackTable(d, max_frames=n, seconds_per_sample=SPS) as t:
            t.summaries_reserve()
            t.update(frames)
            pts, got = t.points(), t.summaries()
            _same_points(pts, big.icao, new, pos, lambda k: _case(big, k))
            _same_summaries(got, sums, lambda k: _case(big, k))
            recs, flags = t.aircraft()
            assert flags == 0 and len(recs) == len(lengths)
            _same_table(recs, sorted(ot.aircraft(), key=lambda s: s.icao), _counts(big.icao))
            assert len(t.changed()[0]) == len(recs) and t.changed()[0].tobytes() == recs.tobytes()
            whole = (pts.tobytes(), got.tobytes(), _state(t))
            assert _run_cuts(t, big, [0, 1 << 12, (1 << 12) + (1 << 16), n], rebase=False) == whole
        R = 8
        deal = _deal(big, R)
        lists = _lists(big, deal, 0, n, [0] * R)
        with A.TrackBank(d, R, max_frames=sum(len(x) for x in lists), seconds_per_sample=SPS) as bank:
            bank.summaries_reserve()
            bank.update(np.concatenate(lists), [len(x) for x in lists])
            bpts, bsums = bank.points(), bank.summaries()
            brecs, bflags = bank.aircraft()
            bheard, bvel = bank.last_heard(), bank.velocity()
            at = 0
            for r in range(R):
                with A.TrackTable(d, max_frames=len(lists[r]), seconds_per_sample=SPS) as t:
                    t.summaries_reserve()
                    t.update(lists[r])
                    assert bpts[at:at + len(lists[r])].tobytes() == t.points().tobytes(), r
                    assert bsums[at:at + len(lists[r])].tobytes() == t.summaries().tobytes(), r
                    assert (brecs[r].tobytes(), bflags[r], bheard[r].tobytes(), bvel[r].tobytes()) == _state(t), r
                at += len(lists[r])
            assert at == len(bpts)
