"""Positions from single messages on the device (adsb_track_*_fixes_reserve / fetch_fixes / fetch_frame_fixes): the
per-frame decode against the CPU mirror (adsb_host_fix_of) and tests/fix_model.py, the merge against the model and
against itself under cuts, a twin store without the reserve for everything the reserve must not change, expire and
reset, a bank against separate tables, a device launch against a host-fed bank, and tools/replay.py --site.  Lists are
at most 4000 frames at 2 MSPS.  Tolerances where two math libraries meet (tests/fix_model.py, assert_fixes_equal):
latitude and longitude equal as doubles (no library call decides them), range 1e-4 NM, bearing 1e-4 degree from 1 NM on;
everything else bit for bit."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from tests import fix_model as M

pytestmark = pytest.mark.gpu
SPS = 0.5e-6
SITE = (47.45, 8.56, 150.0)
EMPTY = M.records({}, [0])[0].tobytes()


def _frames(items):
    """[(offset, 14 frame bytes)] -> FRAME_DTYPE array."""
    out = np.zeros(len(items), dtype=A.FRAME_DTYPE)
    for k, (off, b) in enumerate(items):
        out[k]["offset"] = off
        out[k]["bytes"] = np.frombuffer(bytes(b), dtype=np.uint8)
        out[k]["fixed_bit"] = 0xFF
    return out


def _same(got, want, what=""):
    assert got.dtype.itemsize == want.dtype.itemsize and len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():                      # say where, then fail
        for k in range(len(got)):
            assert got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])


def _check(table, state, what=""):
    """table.fixes() == the model's records, aligned with aircraft()."""
    recs, _ = table.aircraft()
    got = table.fixes()
    assert got.dtype == A.FIX_DTYPE and len(got) == len(recs)
    M.assert_fixes_equal(got, M.records(state, recs["icao"]), what)
    return recs, got


@contextlib.contextmanager
def _tables(d, site=SITE, **kw):
    """A table with a fixes reserve and a twin without one, both closed before the ctx on every path."""
    kw.setdefault("max_frames", 1 << 12)
    with A.TrackTable(d, seconds_per_sample=SPS, **kw) as table, A.TrackTable(d, seconds_per_sample=SPS, **kw) as twin:
        table.fixes_reserve(site)
        yield table, twin


@pytest.fixture(scope="module")
def mixed(oracle):
    """2500 frames of 50 aircraft around SITE: surface, airborne, velocity, identification and other messages."""
    return M.mixed_traffic(oracle, seed=11, site=SITE, n_aircraft=50, n_frames=2500).astype(A.FRAME_DTYPE)


# ---- (a) one frame per aircraft: the device's decode against the CPU mirror and the model -------------------------------
def test_every_frame_equals_the_host_mirror(gpu, oracle):
    rng = np.random.default_rng(5)
    site = M.SITES[5]                                                   # beside the antimeridian
    icaos = np.sort(rng.choice(np.arange(1, 1 << 24), size=4000, replace=False))
    order = rng.permutation(4000)                                       # list order is not ICAO order
    frames = _frames([(100 + 37 * k, M.random_frame(oracle, rng, int(icaos[a]))) for k, a in enumerate(order)])
    base = 1_000_000
    want = np.zeros(4000, dtype=A.FIX_DTYPE)
    want_flags = np.zeros(4000, dtype=np.uint32)
    for k in range(4000):
        time = float(base + int(frames[k]["offset"])) * SPS
        want[k], want_flags[k] = A.host_fix_of(site, frames[k]["bytes"].tobytes(), time)
        model, model_flags = M.fix_of(site, frames[k]["bytes"].tobytes(), time)
        assert model_flags == want_flags[k] and model["time"].tobytes() == want[k]["time"].tobytes()
    assert (want_flags == 0).sum() > 500 and ((want_flags & M.REJECTED) != 0).sum() > 300
    assert ((want_flags & M.SURFACE) != 0).sum() > 200 and ((want_flags & M.VALID) != 0).sum() > 1000
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        with _tables(d, site=site, max_aircraft=4096) as (table, twin):
            table.update(frames, base)
            recs, _ = table.aircraft()
            assert np.array_equal(recs["icao"], icaos)
            by_icao = np.argsort(M.frame_icaos(frames), kind="stable")
            M.assert_fixes_equal(table.fixes(), want[by_icao], "fixes")
            got = table.frame_fixes()
            assert got.dtype == A.FRAME_FIX_DTYPE and len(got) == 4000
            assert np.array_equal(got["flags"], want_flags)
            M.assert_frame_fixes_equal(got, M.frame_records(site, frames), "frame fixes")
            ok = (want_flags & M.VALID) != 0
            assert np.all(got["latitude"][~ok] == 0.0) and np.all(got["range_nm"][~ok] == 0.0)
            assert np.array_equal(got["latitude"][ok], want["latitude"][ok])


# ---- (b) any cutting of a list gives the same bytes ----------------------------------------------------------------------
def test_cuts_give_identical_bytes(gpu, mixed):
    frames = mixed
    state = M.apply({}, SITE, frames, 77, SPS)
    flags = M.records(state, sorted(state))["flags"]
    assert len(state) == 50 and (flags & M.SURFACE).any() and ((flags & (M.VALID | M.SURFACE)) == M.VALID).any()
    rng = np.random.default_rng(12)
    cuts = {"whole": []}
    for name in ("cut 1", "cut 2"):
        edges = sorted(int(x) for x in rng.choice(np.arange(1, len(frames)), size=10, replace=False))
        cuts[name] = edges[:4] + [edges[3]] + edges[4:] + [edges[-1]]   # 12 edges: two empty updates in between
    first = None
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        with _tables(d) as (table, twin):
            for name, cut in cuts.items():
                table.reset()
                edges = [0] + cut + [len(frames)]
                for a, b in zip(edges[:-1], edges[1:]):
                    table.update(frames[a:b], 77)
                    assert len(table.frame_fixes()) == b - a
                recs, got = _check(table, state, name)
                now = (got.tobytes(), recs.tobytes(), table.velocity().tobytes(), table.last_heard().tobytes())
                first = now if first is None else first
                assert now == first, name
            assert (got["n_fixes"] > 0).sum() > 30 and (got["n_rejected"] > 0).any()


# ---- (c) the reserve changes nothing else ----------------------------------------------------------------------------------
def test_everything_else_is_byte_identical_to_a_store_without_the_reserve(gpu, mixed):
    frames = mixed
    rng = np.random.default_rng(21)
    levels = np.zeros(len(frames), dtype=A.LEVEL_DTYPE)
    levels["signal_sum"] = rng.integers(0, 1 << 38, size=len(frames), dtype=np.uint64)
    levels["noise_sum"] = rng.integers(0, 1 << 38, size=len(frames), dtype=np.uint64)
    levels["flags"] = (rng.random(len(frames)) >= 0.2).astype(np.uint16)
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        with _tables(d, max_aircraft=40) as (table, twin):             # 50 aircraft: ten are turned away
            for t in (table, twin):
                t.summaries_reserve()
                t.levels_reserve()
            for a, b in ((0, 900), (900, 900), (900, 2500)):
                table.update(frames[a:b], 5, levels=levels[a:b])
                twin.update(frames[a:b], 5, levels=levels[a:b])
                assert table.points().tobytes() == twin.points().tobytes()
                assert table.summaries().tobytes() == twin.summaries().tobytes()
                (x, fx), (y, fy) = table.aircraft(), twin.aircraft()
                assert x.tobytes() == y.tobytes() and fx == fy == A.ADSB_TRACK_TABLE_FULL
                assert table.velocity().tobytes() == twin.velocity().tobytes()
                assert table.levels().tobytes() == twin.levels().tobytes()
                assert table.last_heard().tobytes() == twin.last_heard().tobytes()
                assert all(p.tobytes() == q.tobytes() for p, q in zip(table.changed(), twin.changed()))
            # the aircraft the full table turned away: only their icao in the per-frame fixes, nothing in the records
            away = (table.points()["flags"] & A.ADSB_TRACK_UNTRACKED) != 0
            got = table.frame_fixes()
            assert away.sum() > 50 and np.all(got["flags"][away] == 0) and np.all(got["latitude"][away] == 0.0)
            M.assert_frame_fixes_equal(got, M.frame_records(SITE, frames[900:], untracked=away), "turned away")
            with pytest.raises(A.AdsbError) as e:
                twin.fixes()
            assert e.value.code == A.ADSB_E_STATE
            with pytest.raises(A.AdsbError) as e:
                twin.frame_fixes()
            assert e.value.code == A.ADSB_E_STATE


# ---- (d) reset, expire, re-admission, and the reserve's own state checks ------------------------------------------------
def test_reset_expire_and_reserve_state(gpu, mixed):
    frames = mixed
    fi = M.frame_icaos(frames)
    icaos = sorted(set(int(x) for x in fi))
    quiet = set(icaos[1::3])                                         # silent in the second half: evicted
    half_at = len(frames) // 2
    keep = np.array([k < half_at or int(fi[k]) not in quiet for k in range(len(frames))])
    frames, fi = frames[keep], fi[keep]
    half = int(keep[:half_at].sum())
    L = _lib.load()
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        with _tables(d) as (table, twin):
            table.update(frames[:half])
            table.update(frames[half:])
            state = M.apply({}, SITE, frames, 0, SPS)
            recs, before = _check(table, state)
            where = {int(x): k for k, x in enumerate(recs["icao"])}
            table.expire(float(frames[half]["offset"]) * SPS)
            after_recs, after = _check(table, state)                   # survivors: still aligned
            gone = set(where) - set(int(x) for x in after_recs["icao"])
            assert gone == quiet and len(after_recs) == len(icaos) - len(quiet)
            for k, icao in enumerate(after_recs["icao"]):               # ... and bit for bit what they were
                assert after[k].tobytes() == before[where[int(icao)]].tobytes()
            assert table.fixes_device() != 0
            for icao in gone:
                del state[icao]
            # an evicted aircraft heard again starts empty
            back = next(i for i in sorted(gone) if before[where[i]]["n_fixes"] > 0)
            ident = frames[:half][(fi[:half] == back)][:1].copy()
            ident["bytes"][0][4] = 4 << 3                               # an identification message (the CRC is not read)
            ident["offset"] += np.uint64(int(frames[-1]["offset"]) + 10)
            table.update(ident)
            recs, got = _check(table, state)
            k = list(recs["icao"]).index(back)
            assert got[k].tobytes() == EMPTY and recs[k]["n_frames"] == 1 and math.isnan(got[k]["time"])
            # a reserve on a store that holds aircraft is refused, with a good site or a new one; a bad site comes first
            for t in (table, twin):
                if t is twin:
                    twin.update(frames[:10])
                with pytest.raises(A.AdsbError) as e:
                    t.fixes_reserve((10.0, 20.0, 100.0))
                assert e.value.code == A.ADSB_E_STATE
                assert L.adsb_track_table_fixes_reserve(t._h, C.byref(_lib.AdsbSite(95.0, 0.0, 10.0))) == A.ADSB_E_ARG
            _check(table, state)
            # reset: the fixes are gone (the side array itself is empty again), and the site may change
            table.reset()
            assert len(table.fixes()) == 0
            raw = np.zeros(64 * 4, dtype=np.uint8)
            hip = _hip_runtime()
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            hip.hipMemcpy.restype = C.c_int
            assert hip.hipMemcpy(raw.ctypes.data, table.fixes_device(), raw.nbytes, 2) == 0     # device to host
            assert raw.tobytes() == EMPTY * 4
            other = (SITE[0] + 0.5, SITE[1] - 0.5, 100.0)
            table.fixes_reserve(other)
            twin.reset()
            twin.fixes_reserve(other)
            for t in (table, twin):
                t.update(frames[half:])
                _check(t, M.apply({}, other, frames[half:], 0, SPS))
            assert table.fixes().tobytes() == twin.fixes().tobytes()


def _hip_runtime():
    """The HIP runtime this process already holds (the one libadsb_hip.so is bound to), for a plain hipMemcpy."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path:
            return C.CDLL(path)
    raise RuntimeError("no HIP runtime mapped")


# ---- (e) a bank's receiver equals a table of its own with that receiver's site -----------------------------------------
@pytest.mark.parametrize("n_receivers", [1, 3, 64])
def test_bank_equals_separate_tables(gpu, oracle, n_receivers):
    R = n_receivers
    per = 3900 // R if R > 1 else 1500
    sites = [(40.0 + 0.3 * r, -100.0 + 0.4 * r, 180.0 - r) for r in range(R)]
    shared = M.mixed_traffic(oracle, seed=31, site=sites[0], n_aircraft=12, n_frames=per).astype(A.FRAME_DTYPE)
    rng = np.random.default_rng(32)
    lists = [shared[rng.random(per) < 0.8] for _ in range(R)]             # the same ICAOs on every receiver
    bases = [1000 * r + 7 for r in range(R)]
    L = _lib.load()
    with A.AdsbDemod(max_samples=1024, max_out=16) as d, \
            A.TrackBank(d, R, max_aircraft=64, max_frames=1 << 12, seconds_per_sample=SPS) as bank, \
            contextlib.ExitStack() as stack:
        # a bank's sites are checked one by one
        arr = (_lib.AdsbSite * R)(*[_lib.AdsbSite(*s) for s in sites])
        arr[R - 1].longitude = 181.0
        assert L.adsb_track_bank_fixes_reserve(bank._h, arr) == A.ADSB_E_ARG
        with pytest.raises(ValueError):
            bank.fixes_reserve(sites + [sites[0]])
        bank.fixes_reserve(sites)
        tables = [stack.enter_context(A.TrackTable(d, max_aircraft=64, max_frames=1 << 12, seconds_per_sample=SPS))
                  for _ in range(R)]
        for r, t in enumerate(tables):
            t.fixes_reserve(sites[r])
        for part in (0, 1):
            cut = [(slice(0, len(x) // 2) if part == 0 else slice(len(x) // 2, None)) for x in lists]
            fr = np.concatenate([x[c] for x, c in zip(lists, cut)])
            counts = [len(x[c]) for x, c in zip(lists, cut)]
            bank.update(fr, counts, bases)
            ff, pos = bank.frame_fixes(), 0
            assert len(ff) == len(fr)
            for r in range(R):
                tables[r].update(lists[r][cut[r]], bases[r])
                assert ff[pos:pos + counts[r]].tobytes() == tables[r].frame_fixes().tobytes(), r
                pos += counts[r]
        recs, got = bank.aircraft()[0], bank.fixes()
        assert len(got) == R
        for r in range(R):
            assert recs[r].tobytes() == tables[r].aircraft()[0].tobytes()
            _same(got[r], tables[r].fixes(), r)
            M.assert_fixes_equal(got[r], M.records(M.apply({}, sites[r], lists[r], bases[r], SPS), recs[r]["icao"]), r)
            assert len(got[r]) == len(recs[r]) > 0
        if R > 1:
            assert got[0].tobytes() != got[1].tobytes()
        with pytest.raises(A.AdsbError) as e:
            bank.fixes_reserve(sites)                                      # it holds aircraft
        assert e.value.code == A.ADSB_E_STATE


# ---- (f) from a launch ---------------------------------------------------------------------------------------------------
def test_update_launch_equals_a_host_fed_bank(gpu, oracle):
    import torch
    from tests.golden.make_golden import modulate, place
    nch, n = 3, 60_000
    stride = n + 8
    sites = [(47.45, 8.56, 180.0), (46.2, 6.1, 100.0), (48.35, 11.8, 180.0)]
    rng = np.random.default_rng(41)
    chans = []
    for c in range(nch):
        items = []
        for k in range(45):
            tc = int(rng.choice([5, 7, 11, 13, 20]))
            fr = M.frame_at(oracle, 0x4B0000 + (k % 9) + 4 * c, sites[c], float(rng.uniform(0, 44)), float(rng.uniform(0, 360)),
                            tc, k & 1, movement=int(rng.integers(0, 128)), track_valid=1, track=int(rng.integers(0, 128)))
            items.append((500 + 1300 * k + int(rng.integers(0, 50)), modulate(fr, (100, 30), None)))
        chans.append(place(n, items, np.int8, floor=3, seed=42 + c))
    buf = np.zeros((nch * stride, 2), dtype=np.int8)
    for c in range(nch):
        buf[c * stride:c * stride + n] = chans[c]
    bases = [0, 5_000_000, 11]
    with A.AdsbDemod(max_samples=n, max_out=1 << 12, max_channels=nch, host_staging=False) as d, \
            A.TrackBank(d, nch, max_aircraft=256, max_frames=1 << 12, seconds_per_sample=SPS) as bank, \
            A.TrackBank(d, nch, max_aircraft=256, max_frames=1 << 12, seconds_per_sample=SPS) as fed:
        bank.fixes_reserve(sites)
        fed.fixes_reserve(sites)
        dev = torch.from_numpy(buf).cuda()
        d.demod_device_async(dev.data_ptr(), n, n_channels=nch, channel_stride=stride)
        bank.update_launch(bases)
        frames, counts, total, flags = d.fetch()
        assert flags == 0 and sum(counts) == len(frames) == total and min(counts) >= 45
        fed.update(frames, counts, bases)
        assert bank.frame_fixes().tobytes() == fed.frame_fixes().tobytes()
        recs, got, want = bank.aircraft()[0], bank.fixes(), fed.fixes()
        pos = 0
        for c in range(nch):
            assert recs[c].tobytes() == fed.aircraft()[0][c].tobytes()
            _same(got[c], want[c], c)
            part = frames[pos:pos + counts[c]]
            pos += counts[c]
            M.assert_fixes_equal(got[c], M.records(M.apply({}, sites[c], part, bases[c], SPS), recs[c]["icao"]), c)
            assert int(got[c]["n_fixes"].sum()) >= 45 and (got[c]["flags"] & M.SURFACE).any()
        del dev


# ---- (g) one aircraft holds nearly the whole list ---------------------------------------------------------------------------
def test_one_aircraft_with_most_of_the_list(gpu, oracle, mixed):
    rng = np.random.default_rng(51)
    icao = int(np.median(M.frame_icaos(mixed)))                          # in the middle of the sorted list
    items = []
    for k in range(3900):
        tc = int(rng.choice([6, 11, 19, 21]))
        fr = M.frame_at(oracle, icao, SITE, float(rng.uniform(0, 48 if tc == 6 else 160)), float(rng.uniform(0, 360)), tc,
                        int(rng.integers(0, 2)), movement=int(rng.integers(0, 128)))
        items.append((10 + 20 * k, fr))
    big = _frames(items)
    others = mixed[:100].copy()
    others["offset"] = np.sort(rng.integers(0, 20 * 3900, size=100))
    frames = np.concatenate([big, others])
    frames = frames[np.argsort(frames["offset"], kind="stable")]
    state = M.apply({}, SITE, frames, 3, SPS)
    assert state[icao]["n_fixes"] > 2500 and state[icao]["n_rejected"] > 20
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        with _tables(d) as (table, twin):
            table.update(frames, 3)
            _, whole = _check(table, state, "one update")
            M.assert_frame_fixes_equal(table.frame_fixes(), M.frame_records(SITE, frames), "frame fixes")
            table.reset()
            for a, b in ((0, 1), (1, 2000), (2000, 3999), (3999, 4000)):
                table.update(frames[a:b], 3)
            _, cut = _check(table, state, "four updates")
            assert cut.tobytes() == whole.tobytes()


# ---- (h) tools/replay.py --aircraft --site ---------------------------------------------------------------------------------
def test_replay_aircraft_site(gpu, oracle, tmp_path):
    import importlib.util
    import os
    import subprocess
    import sys

    from tests.golden.make_golden import modulate, place
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    site = (-33.9, 151.2, 180.0)
    chunk = 20_000
    msgs = [M.frame_at(oracle, 0x7C0001, site, 30.0, 45.0, 11, 0), M.frame_at(oracle, 0x7C0001, site, 30.2, 45.0, 11, 1),
            M.frame_at(oracle, 0x7C0002, site, 2.0, 300.0, 7, 0, movement=40, track_valid=1, track=32),
            M.frame_at(oracle, 0x7C0003, site, 100.0, 180.0, 20, 1),
            M.frame_at(oracle, 0x7C0004, site, 10.0, 10.0, 6, 1, movement=0),
            M.raw_frame(oracle, 0x7C0005, 19 << 51 | 1 << 48 | 5 << 32 | 9 << 21),      # velocity only: no fix
            M.frame_at(oracle, 0x7C0006, site, 46.0, 90.0, 8, 1, movement=3)]           # surface beyond 45 NM: rejected
    items = [(chunk * (k // 2) + 300 + 4001 * (k % 2), modulate(fr, (900 + 50 * k, 30), None)) for k, fr in enumerate(msgs)]
    iq = place(chunk * 5, items, np.int16, floor=3, seed=6)           # (the fifth, frameless chunk is never sent)
    path = tmp_path / "capture.c16"
    iq.astype("<i2").tofile(path)
    frames = _frames([(o, fr) for (o, _), fr in zip(items, msgs)])
    state = M.apply({}, site, frames, 0, SPS)
    tool = os.path.join(root, "tools", "replay.py")
    spec = importlib.util.spec_from_file_location("replay_tool", tool)
    replay = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(replay)
    plain = subprocess.run([sys.executable, tool, str(path), "--aircraft"], capture_output=True, text=True, timeout=300,
                           check=True).stdout
    assert plain.startswith("ICAO\tCallsign\tAltitude\tLatitude\tLongitude\tVelocity\tAge\n")
    assert plain.count("\n") == 7 and all(line.count("\t") == 6 for line in plain.splitlines())
    with A.AdsbDemod(sample_type=A.ADSB_SAMPLE_I16, max_samples=1024, max_out=64, host_staging=False) as d:
        assert replay.aircraft_table(d, frames, 4 * chunk) == plain         # and the function's default is the same text
    want, n_fix = "", 0
    for k, line in enumerate(plain.splitlines()):
        if k == 0:
            want += line + "\tFixLat\tFixLon\tRange\tBearing\tGS\n"
            continue
        a = state[int(line.split("\t")[0], 16)]
        if not a["flags"] & M.VALID:
            want += line + "\tn/a\tn/a\tn/a\tn/a\tn/a\n"
            continue
        n_fix += 1
        gs = f"{float(a['ground_speed_kt']):.1f}" if a["flags"] & M.SPEED else "n/a"
        want += line + (f"\t{float(a['latitude']):.6f}\t{float(a['longitude']):.6f}\t{float(a['range_nm']):.1f}"
                        f"\t{float(a['bearing_deg']):.1f}\t{gs}\n")
    assert n_fix == 4 and "\t16.0\n" in want and want.count("n/a\tn/a\tn/a\tn/a\tn/a") == 2
    got = subprocess.run([sys.executable, tool, str(path), "--aircraft", f"--site={site[0]},{site[1]}"],
                         capture_output=True, text=True, timeout=300, check=True).stdout
    assert got == want
    assert replay.parse_site("1.5,-2") == (1.5, -2.0, 180.0) and replay.parse_site("1,2,60") == (1.0, 2.0, 60.0)
    assert replay.fix_columns(M.records({}, [1])[0]) == ["n/a"] * 5
