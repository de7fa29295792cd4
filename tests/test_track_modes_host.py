"""The CPU mirror of a modes reserve's per-frame step and combine (adsb_host_track_modes_of, adsb_host_track_modes_merge:
the text the device compiles too) against tests/track_modes_model.py, a sequential model: every record the Mode S cases
produce, every DF 0..31 x kind x flags word seen in them, folds of random runs, saturation, and "later wins" at equal
times.  Everything is integers and copied times, so every comparison is byte for byte.  CPU tier."""
import itertools

import numpy as np
import pytest

from tests import modes_cases as K
from tests import modes_model as MM
from tests import track_modes_model as M


@pytest.fixture(scope="module")
def case_recs():
    """Every record of every Mode S case, by the Mode S model (no library call)."""
    recs = [MM.modes(frames, known)["recs"] for _, frames, known in K.all_cases()]
    return np.concatenate(recs)


@pytest.fixture(scope="module")
def grid(case_recs):
    """DF 0..31 x kind x every flags word the cases produce, with the fields of a case record that has those flags"""
    by_flags = {}
    for r in case_recs:
        by_flags.setdefault(int(r["flags"]), r)
    assert len(by_flags) >= 12 and all(any(f & bit for f in by_flags) for bit in MM.ALL_FLAGS)
    out = []
    for df, kind, (flags, r) in itertools.product(range(32), range(5), sorted(by_flags.items())):
        g = r.copy()
        g["df"], g["kind"] = df, kind
        out.append(g)
    return np.array(out, dtype=MM.REC_DTYPE)


def _one(lib, rec, time):
    got, ok = lib.host_track_modes_of(rec, time)
    assert got.dtype == lib.AIRCRAFT_MODES_DTYPE
    return got, ok


def _want_one(rec, time):
    return M.record(M.count(M.empty(), rec, time)) if M.accepted(rec) else M.record(M.empty())


def test_single_frames_of_the_cases(lib, case_recs):
    kinds = set()
    for j, r in enumerate(case_recs):
        t = 0.25 + j * 1e-3
        got, ok = _one(lib, r, t)
        assert ok == M.accepted(r) and got.tobytes() == _want_one(r, t).tobytes(), (j, r, got)
        kinds.add((int(r["df"]), int(r["kind"])))
    assert len(kinds) > 40


def test_every_df_kind_and_flags(lib, grid):
    for j, r in enumerate(grid):
        got, ok = _one(lib, r, 7.5)
        assert ok == (int(r["kind"]) in (0, 1)) and got.tobytes() == _want_one(r, 7.5).tobytes(), (r, got)
        if not ok:
            assert got.tobytes() == M.record(M.empty()).tobytes()


def test_empty_record(lib):
    rec = np.zeros(1, dtype=MM.REC_DTYPE)[0]
    rec["kind"] = MM.PARITY
    got, ok = _one(lib, rec, 1.0)
    assert not ok and np.isnan([got["altitude_time"], got["squawk_time"], got["callsign_time"]]).all()
    z = got.copy()
    z["altitude_time"] = z["squawk_time"] = z["callsign_time"] = 0.0
    assert z.tobytes() == bytes(64)


def test_folds_against_the_sequential_model(lib, grid):
    """Runs of accepted records folded with the merge, left to right and in random groupings, against the model's loop"""
    rng = np.random.default_rng(11)
    ok = grid[(grid["kind"] <= 1)]
    for trial in range(60):
        run = ok[rng.integers(0, len(ok), size=int(rng.integers(1, 12)))]
        times = np.sort(rng.integers(0, 4, size=len(run))) * 0.5          # equal times on purpose
        want = M.empty()
        for r, t in zip(run, times):
            M.count(want, r, float(t))
        singles = [_one(lib, r, float(t))[0] for r, t in zip(run, times)]
        acc = np.array([M.record(M.empty())]).view(lib.AIRCRAFT_MODES_DTYPE)[0]
        for s in singles:
            acc = lib.host_track_modes_merge(acc, s)
        assert acc.tobytes() == M.record(want).tobytes(), (trial, acc, M.record(want))
        cut = int(rng.integers(0, len(run) + 1))                           # (a b ..)(.. z): the combine is associative
        left, right = singles[0] if cut else None, None
        for s in singles[1:cut]:
            left = lib.host_track_modes_merge(left, s)
        for s in singles[cut:]:
            right = s if right is None else lib.host_track_modes_merge(right, s)
        both = right if left is None else left if right is None else lib.host_track_modes_merge(left, right)
        assert both.tobytes() == M.record(want).tobytes(), (trial, cut)


def test_empty_is_the_identity(lib, grid):
    e = np.array([M.record(M.empty())]).view(lib.AIRCRAFT_MODES_DTYPE)[0]
    for r in grid[grid["kind"] <= 1][::37]:
        one = _one(lib, r, 3.0)[0]
        assert lib.host_track_modes_merge(e, one).tobytes() == one.tobytes()
        assert lib.host_track_modes_merge(one, e).tobytes() == one.tobytes()


@pytest.mark.parametrize("start", [2 ** 32 - 2, 2 ** 32 - 1])
def test_counts_saturate(lib, start):
    into = M.empty()
    for k in M.COUNTS:
        into[k] = start
    rec = np.zeros(1, dtype=MM.REC_DTYPE)[0]
    rec["kind"] = MM.KNOWN
    a = np.array([M.record(into)]).view(lib.AIRCRAFT_MODES_DTYPE)[0]
    for df, also in ((11, "n_allcall"), (4, "n_surveillance"), (0, "n_airair"), (24, None)):
        rec["df"] = df
        want = dict(into)
        got = a
        for step in range(3):
            got = lib.host_track_modes_merge(got, _one(lib, rec, 1.0)[0])
            M.count(want, rec, 1.0)
            assert got.tobytes() == M.record(want).tobytes(), (df, step)
        assert got["n_replies"] == M.U32 and (also is None or got[also] == M.U32)
        for k in M.COUNTS:
            assert got[k] == (M.U32 if k in ("n_replies", also) else start)


def test_later_wins_at_equal_times(lib):
    """Two frames at one time: the one later in list order is the newest, field by field"""
    def rec(df, flags, alt=0, squawk=0, fs=0, call=b""):
        r = np.zeros(1, dtype=MM.REC_DTYPE)[0]
        r["kind"], r["df"], r["flags"], r["altitude_ft"], r["squawk"], r["fs"], r["callsign"] = MM.KNOWN, df, flags, alt, squawk, fs, call
        return r
    first = rec(20, MM.ALT | MM.CALLSIGN | MM.GROUND | MM.ALERT, alt=1000, fs=3, call=b"FIRST___")
    second = rec(21, MM.SQUAWK | MM.CALLSIGN | MM.SPI, squawk=7700, fs=5, call=b"SECOND__")
    for a, b in ((first, second), (second, first)):
        got = lib.host_track_modes_merge(_one(lib, a, 2.0)[0], _one(lib, b, 2.0)[0])
        want = M.count(M.count(M.empty(), a, 2.0), b, 2.0)
        assert got.tobytes() == M.record(want).tobytes()
        assert got["callsign"] == bytes(b["callsign"]) and got["fs"] == b["fs"] and got["last_df"] == b["df"]
        assert got["altitude_ft"] == 1000 and got["squawk"] == 7700
        assert bool(got["flags"] & M.GROUND) == bool(b["flags"] & MM.GROUND)
        assert bool(got["flags"] & M.SPI) == bool(b["flags"] & MM.SPI) and got["flags"] & M.STATUS
    third = rec(11, 0)                                                    # no source of status or ground: both stay
    got = lib.host_track_modes_merge(_one(lib, first, 2.0)[0], _one(lib, third, 2.0)[0])
    assert got["flags"] & M.GROUND and got["flags"] & M.ALERT and got["fs"] == 3 and got["last_df"] == 11
    sq = rec(17, 0)
    sq["kind"] = MM.SELF
    got = lib.host_track_modes_merge(got, _one(lib, sq, 2.0)[0])
    assert got["flags"] & M.SQUITTER and got["n_replies"] == 2 and got["last_df"] == 17


def test_bad_arguments(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    some = np.zeros(64, dtype=np.uint8)
    one = _lib.AdsbAircraftModes()
    assert L.adsb_host_track_modes_of(None, 0.0, one, None) == lib.ADSB_E_ARG
    assert L.adsb_host_track_modes_of(some.ctypes.data, 0.0, None, None) == lib.ADSB_E_ARG
    assert L.adsb_host_track_modes_merge(None, one) == lib.ADSB_E_ARG
    assert L.adsb_host_track_modes_merge(one, None) == lib.ADSB_E_ARG
