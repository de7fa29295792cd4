"""The single-message position decode ON THE DEVICE (track_fix_decode_kernel, adsb_track.hip) on every case of
tests/fix_cases.py: zone, pole and meridian edges, negative and subnormal sites, half-zone and range limits, every field
value.  One TrackBank with one receiver per distinct site takes the whole list in updates of at most 4096 frames; its
per-frame fixes and its per-aircraft records are held against the CPU mirror (flags, and latitude and longitude BIT FOR
BIT: nothing before NL uses a math library and NL is an integer) and against the exact reference (flags; latitude and
longitude within 1e-12 degree; range and bearing within half an f32 step of the 50-digit value, the rule and the
helpers of tests/test_fix_cases.py).  Ties are compared with the mirror only.  Three tables at edge sites give the bank's
bytes."""
import numpy as np
import pytest

import air_rs_amd as A
from tests import fix_cases as FC
from tests import fix_model as M
from tests import test_fix_cases as T

pytestmark = pytest.mark.gpu
SPS = 0.5e-6
MAX_FRAMES = 1 << 12
MAX_AIRCRAFT = 2048                  # the fullest site holds 1,307 cases
BASE = 1000


class Run:
    """The case list in receiver-major order (`order`: case index of each sorted frame), its frames and what the bank
    said of them."""


@pytest.fixture(scope="module")
def layout(oracle):
    cases = FC.cases(oracle)
    sites, where = FC.sites_of(cases)
    run = Run()
    run.cases, run.reference, run.sites, run.where = cases, FC.reference(oracle), sites, np.array(where)
    run.order = np.argsort(run.where, kind="stable")
    run.frames = np.zeros(len(cases), dtype=A.FRAME_DTYPE)
    for at, k in enumerate(run.order):
        run.frames[at]["offset"] = 10 + 3 * at
        run.frames[at]["bytes"] = np.frombuffer(cases[k].frame, dtype=np.uint8)
    run.frames["fixed_bit"] = 0xFF
    run.times = np.zeros(len(cases))
    run.times[run.order] = (BASE + run.frames["offset"]).astype(np.float64) * SPS
    assert len(sites) <= FC.MAX_SITES and np.bincount(run.where).max() <= MAX_AIRCRAFT
    return run


@pytest.fixture(scope="module")
def bank_run(gpu, layout):
    """Every case through one bank: frame_fixes() of each update, back in case order, and the records at the end."""
    run, R = layout, len(layout.sites)
    got = np.zeros(len(run.cases), dtype=A.FRAME_FIX_DTYPE)
    with A.AdsbDemod(max_samples=1024, max_out=16) as d, \
            A.TrackBank(d, R, max_aircraft=MAX_AIRCRAFT, max_frames=MAX_FRAMES, seconds_per_sample=SPS) as bank:
        bank.fixes_reserve(run.sites)
        for a in range(0, len(run.frames), MAX_FRAMES):
            part = slice(a, min(a + MAX_FRAMES, len(run.frames)))
            counts = np.bincount(run.where[run.order[part]], minlength=R)
            bank.update(run.frames[part], counts, BASE)
            ff = bank.frame_fixes()
            assert ff.dtype == A.FRAME_FIX_DTYPE and len(ff) == part.stop - part.start
            got[run.order[part]] = ff
        run.frame_fixes = got
        run.aircraft, run.flags = bank.aircraft()
        run.fixes = bank.fixes()
    return run


@pytest.fixture(scope="module")
def mirror(lib, layout):
    fixes = np.zeros(len(layout.cases), dtype=lib.FIX_DTYPE)
    flags = np.zeros(len(layout.cases), dtype=np.uint32)
    for k, c in enumerate(layout.cases):
        fixes[k], flags[k] = lib.host_fix_of(c.site, c.frame, layout.times[k])
    return fixes, flags


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_every_frame_against_the_mirror_and_the_reference(bank_run, mirror):
    run, (want, want_flags) = bank_run, mirror
    got = run.frame_fixes
    icaos = np.array([int.from_bytes(c.frame[1:4], "big") for c in run.cases], dtype=np.uint32)
    assert np.array_equal(got["icao"], icaos)
    # flags: the mirror's on every case, ties included
    assert np.array_equal(got["flags"], want_flags), np.flatnonzero(got["flags"] != want_flags)[:10]
    # latitude and longitude: the mirror's bits, ties included (a rejected frame's are the bits of +0.0)
    for name in ("latitude", "longitude"):
        differ = np.flatnonzero(_bits(got[name]) != _bits(want[name]))
        print(f"{name}: {len(differ)} of {len(got)} frames differ from the mirror in a bit")
        assert len(differ) == 0, (name, [(run.cases[k], got[name][k], want[name][k]) for k in differ[:5]])
    # the reference: flags, positions, range and bearing; zeros for rejected and non-position frames
    T.check_against_reference(run.cases, run.reference, got["latitude"], got["longitude"], got["range_nm"], got["bearing_deg"],
                              got["flags"], "device")
    ok = (got["flags"] & M.VALID) != 0
    for name in ("latitude", "longitude", "range_nm", "bearing_deg"):
        assert not got[name][~ok].view(np.uint8).any(), name
    assert np.all((got["bearing_deg"] >= 0) & (got["bearing_deg"] < 360))
    dr = np.abs(got["range_nm"].astype(np.float64) - want["range_nm"])[ok]
    db = np.abs(got["bearing_deg"].astype(np.float64) - want["bearing_deg"])[ok]
    print(f"device against mirror: range_nm differs on {int((dr > 0).sum())} frames (largest {dr.max():.3g} NM), bearing_deg "
          f"on {int((db > 0).sum())} (largest {db.max():.3g} degree)")


def test_per_aircraft_records(bank_run, mirror):
    """fixes(): one frame per aircraft, so every record is its frame's decode with counts 1 / 0, 0 / 1 or 0 / 0."""
    run, (want, want_flags) = bank_run, mirror
    assert not any(run.flags)
    recs = np.zeros(len(run.cases), dtype=A.FIX_DTYPE)
    seen = 0
    by_icao = {int.from_bytes(c.frame[1:4], "big"): k for k, c in enumerate(run.cases)}
    for r in range(len(run.sites)):
        assert len(run.aircraft[r]) == len(run.fixes[r]) == int((run.where == r).sum()), r
        assert np.all(run.aircraft[r]["n_frames"] == 1)
        for icao, fix in zip(run.aircraft[r]["icao"], run.fixes[r]):
            k = by_icao[int(icao)]
            assert run.where[k] == r
            recs[k] = fix
            seen += 1
    assert seen == len(run.cases)
    # against the mirror: everything but range and bearing bit for bit, the time and the padding included
    for name in M.EXACT + ("time", "latitude", "longitude"):
        assert recs[name].tobytes() == want[name].tobytes(), name
    # ... and the same values as the frame's own record
    ff = run.frame_fixes
    for name in ("latitude", "longitude", "range_nm", "bearing_deg"):
        assert recs[name].tobytes() == ff[name].tobytes(), name
    assert np.array_equal(recs["flags"], np.where(ff["flags"] & M.VALID, ff["flags"], 0).astype(np.uint8))
    T.check_fields(run.cases, run.reference, recs, "device records")
    T.check_against_reference(run.cases, run.reference, recs["latitude"], recs["longitude"], recs["range_nm"],
                              recs["bearing_deg"], ff["flags"], "device records")


EDGE_SITES = ((90.0, 180.0), (48.0, -180.0), (FC.MIN_SUBNORMAL, FC.MIN_SUBNORMAL))


def _same_site(a, b):
    return all(x == y and np.signbit(x) == np.signbit(y) for x, y in zip(a, b))


@pytest.mark.parametrize("edge", EDGE_SITES, ids=["polar", "-180", "subnormal"])
def test_bank_equals_a_table_at_an_edge_site(bank_run, edge):
    run = bank_run
    r = [k for k, s in enumerate(run.sites) if _same_site(s[:2], edge)]
    assert len(r) == 1
    r = r[0]
    mine = run.where[run.order] == r
    frames, cases = run.frames[mine], run.order[mine]
    assert len(frames) == 36
    with A.AdsbDemod(max_samples=1024, max_out=16) as d, \
            A.TrackTable(d, max_aircraft=64, max_frames=MAX_FRAMES, seconds_per_sample=SPS) as table:
        table.fixes_reserve(run.sites[r])
        table.update(frames, BASE)
        assert table.frame_fixes().tobytes() == run.frame_fixes[cases].tobytes()
        assert table.aircraft()[0].tobytes() == run.aircraft[r].tobytes()
        assert table.fixes().tobytes() == run.fixes[r].tobytes()
        assert (table.fixes()["n_fixes"] == 1).sum() >= 24
