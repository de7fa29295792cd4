"""Comm-B registers per aircraft on the device (adsb_track_table_commb_reserve / update_commb / fetch_commb /
fetch_frame_commb) against tests/track_commb_model.py, a sequential model, and against the CPU mirror, byte for byte:
every field is an integer or the store's frame time, so nothing needs a tolerance.  Lists are
tests/track_commb_cases.py's, at most 4097 frames."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from tests import commb_model as CM
from tests import modes_model as MM
from tests import track_commb_cases as K
from tests import track_commb_mirror as MI
from tests import track_commb_model as T

pytestmark = pytest.mark.gpu
SPS = K.SPS
EMPTY = T.record(T.empty()).tobytes()


@contextlib.contextmanager
def _table(max_frames=1 << 13, reserve=True, cfg=None, **kw):
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        with A.TrackTable(d, seconds_per_sample=SPS, max_frames=max_frames, **kw) as table:
            if reserve:
                table.modes_reserve()
                table.commb_reserve(**(cfg or {}))
            yield table


def _frames(case):
    return np.ascontiguousarray(case["frames"]).view(A.FRAME_DTYPE)


def _update(table, case, lo=0, hi=None, base=0):
    hi = len(case["frames"]) if hi is None else hi
    table.update(_frames(case)[lo:hi], base, modes=case["recs"][lo:hi].view(A.MODES_DTYPE), commb=case["commb"][lo:hi].view(A.COMMB_DTYPE))
    return table.frame_commb()


def _run(table, model, case, cuts=(), what=""):
    """The case through the table and the model, cut alike; the per-frame outputs and the side records must agree."""
    edges = [0] + list(cuts) + [len(case["frames"])]
    got, want = [], []
    for lo, hi in zip(edges, edges[1:]):
        got.append(_update(table, case, lo, hi))
        want.append(model.update(case["frames"][lo:hi], case["recs"][lo:hi], case["commb"][lo:hi]))
        assert len(got[-1]) == hi - lo
    got, want = np.concatenate(got), np.concatenate(want)
    T.same_frames(got, want, (what, case["name"], cuts))
    assert table.aircraft()[0]["icao"].tolist() == sorted(model.state)
    recs = table.commb()
    assert recs.dtype == A.AIRCRAFT_COMMB_DTYPE
    T.same_records(recs, model.records(), (what, case["name"], cuts))
    return got, recs


@pytest.fixture(scope="module")
def big():
    """4097 frames of the realistic kind over 40 aircraft, with rejected frames, other squitters and 1,7 replies"""
    case = K.sized(4097)
    out, records, _ = K.run_model(case)
    settled = out[out["state"] == T.SETTLED]
    assert (settled["bds"] == 0x50).sum() > 50 and (settled["bds"] == 0x60).sum() > 10 and (out["state"] == T.AMBIGUOUS).any()
    return case, out, records


# ---- (a) the smallest shapes where the scans and the merge can go wrong ---------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4097])
def test_list_lengths(gpu, big, n):
    case = big[0] if n == 4097 else K.sized(n)
    assert len(case["frames"]) == n
    with _table() as table:
        out, recs = _run(table, T.Table(), case)
        mirror_out, mirror_recs = MI.run(case)
        T.same_frames(out, mirror_out)
        T.same_records(recs, mirror_recs)
    if n == 1:                                                   # and a single reply alone, and a single rejected one
        for kind in (T.KNOWN, T.UNKNOWN):
            with _table() as table:
                _run(table, T.Table(), K.build("one reply", [(K.reply(K.BOTH), K.A, kind)]))


@pytest.mark.parametrize("case", K.small_cases(), ids=lambda c: c["name"])
def test_constructed_lists(gpu, case):
    K.claims_hold(case)
    with _table() as table:
        out, recs = _run(table, T.Table(), case)
        mirror_out, mirror_recs = MI.run(case)
        T.same_frames(out, mirror_out)
        T.same_records(recs, mirror_recs)


def test_held_reference_and_the_lists_own(gpu):
    first, second = K.held()
    for cases, want in (((first, second), (T.SETTLED, 0x50)), ((first, K.list_wins()), (T.AMBIGUOUS, 0))):
        with _table() as table:
            model = T.Table()
            for c in cases:
                out, recs = _run(table, model, c)
            assert (int(out["state"][-1]), int(out["bds"][-1])) == want
            if want[0] == T.SETTLED:
                assert int(recs["bds50"]["settled"][0]) == 1 and int(recs["bds50"]["value"][0][2]) == 430
                assert int(recs["n_settled"][0]) == 1 and recs["bds50"]["time"][0] == 20 * K.STEP * SPS
    # too old by then: the same reply 10 s and one sample after the velocity message stays ambiguous; at 10 s it settles
    for offset, want in ((20_000_000, T.SETTLED), (20_000_001, T.AMBIGUOUS)):
        late = K.build("the reply alone, later", [(K.reply(K.BOTH), K.A, T.KNOWN)], offsets=[offset])
        with _table() as table:
            model = T.Table()
            _run(table, model, first)
            out, _ = _run(table, model, late)
            assert int(out["state"][0]) == want


# ---- (b) cuts -----------------------------------------------------------------------------------------------------------
def test_every_cut_of_the_twelve_frame_list(gpu):
    case = K.twelve()
    n = len(case["frames"])
    assert n == 12
    whole_out, whole_recs, _ = K.run_model(case)
    with _table(max_frames=64) as table:
        for a in range(1, n):
            for b in [None] + list(range(a + 1, n)):
                cuts = [a] if b is None else [a, b]
                table.reset()
                out, recs = _run(table, T.Table(), case, cuts)
                T.same_frames(out, whole_out, cuts)
                T.same_records(recs, whole_recs, cuts)


def test_random_cuts_of_4097_frames(gpu, big):
    case, whole_out, whole_recs = big
    rng = np.random.default_rng(3)
    with _table() as table:
        for k in range(3):
            cuts = sorted(set(rng.integers(1, 4097, size=(2, 9, 40)[k]).tolist()))
            table.reset()
            out, recs = _run(table, T.Table(), case, cuts)
            T.same_frames(out, whole_out, cuts)
            T.same_records(recs, whole_recs, cuts)


# ---- (c) a full table, expire, reset, held from before the reserve --------------------------------------------------------
def test_full_table_turns_away_and_counts_nothing(gpu, big):
    case = big[0]
    with _table(max_aircraft=8) as table:
        model = T.Table(max_aircraft=8)
        out, recs = _run(table, model, case, [1500])
        assert len(recs) == 8 and table.aircraft()[1] & 1                  # ADSB_TRACK_TABLE_FULL
        turned = (table.points()["flags"] & A.ADSB_TRACK_UNTRACKED) != 0
        assert turned.any()
        tail = out[1500:]
        assert not (tail["state"][turned] == T.SETTLED).any()
        assert tail[turned].tobytes() == case["commb"][1500:][turned].tobytes()


def test_expire_forgets_the_held_velocity_and_reset(gpu):
    first, second = K.held()
    other = K.build("another aircraft, later", [(K.other_frame(K.B), K.B, T.SELF)], offsets=[60_000_000])
    late = K.build("the reply alone, later", [(K.reply(K.BOTH), K.A, T.KNOWN)], offsets=[60_000_100])
    with _table(max_aircraft=4) as table:
        model = T.Table(max_aircraft=4)
        _run(table, model, first)
        _run(table, model, other)
        table.expire(10.0)                                                    # A was heard last at 0 s, B at 30 s
        model.expire([K.A])
        assert table.aircraft()[0]["icao"].tolist() == [K.B]
        T.same_records(table.commb(), model.records(), "after expire")
        fresh = K.build("velocity and reply of the re-admitted aircraft",
                        [(K.reply(K.BOTH), K.A, T.KNOWN), (K.ground_frame(K.A, **K.AGREES), K.A, T.SELF),
                         (K.reply(K.BOTH), K.A, T.KNOWN)], offsets=[60_000_100, 60_000_200, 60_000_300])
        out, recs = _run(table, model, fresh)
        assert out["state"].tolist() == [T.AMBIGUOUS, T.NOT_COMMB, T.SETTLED]   # the first one finds no velocity any more
        # a survivor's record moves with it
        more = K.build("replies of both", [(K.reply(CM.mb_17([7, 9])), K.B, T.KNOWN), (K.reply(K.BOTH), K.A, T.KNOWN)],
                       offsets=[60_000_400, 60_000_500])
        _run(table, model, more)
        before = {int(i): r.tobytes() for i, r in zip(table.aircraft()[0]["icao"], table.commb())}
        table.expire(30.0001)                                                 # evicts nothing of these
        table.expire(30.00022)                                                # B (heard last at 30.0002 s) goes, A moves to slot 0
        model.expire([K.B])
        assert table.aircraft()[0]["icao"].tolist() == [K.A] and table.commb()[0].tobytes() == before[K.A]
        T.same_records(table.commb(), model.records(), "after the second expire")
        # reset: every place empty, also the places no aircraft holds
        table.reset()
        assert len(table.commb()) == 0
        raw = np.zeros(4, dtype=A.AIRCRAFT_COMMB_DTYPE)
        hip = _hip_runtime()
        assert hip.hipMemcpy(raw.ctypes.data, table.commb_device(), raw.nbytes, 2) == 0     # device to host
        assert raw.tobytes() == EMPTY * 4
        with pytest.raises(A.AdsbError) as e:
            table.frame_commb()                                               # no update_commb since the reset
        assert e.value.code == A.ADSB_E_STATE
        model = T.Table(max_aircraft=4)
        _run(table, model, late)
        out, _ = _run(table, model, fresh)
        assert out["state"].tolist() == [T.AMBIGUOUS, T.NOT_COMMB, T.SETTLED]


def test_held_from_before_the_reserve(gpu):
    first, second = K.held()
    with _table(reserve=False) as table:
        table.update(_frames(first), 0)                                       # a plain update leaves the velocity behind
        table.modes_reserve()
        table.commb_reserve()
        got = table.commb()
        assert len(got) == 1 and got.tobytes() == EMPTY
        model = T.Table()
        model.update(first["frames"], first["recs"])
        out, recs = _run(table, model, second)
        assert int(out["state"][0]) == T.SETTLED and int(recs["n_settled"][0]) == 1


# ---- (d) what the reserve leaves alone -----------------------------------------------------------------------------------
def test_rejected_df20_frames_keep_their_stateless_record(gpu):
    items = [(K.ground_frame(K.A, **K.AGREES), K.A, T.SELF)]
    items += [(K.reply(K.BOTH), K.A, kind) for kind in (T.UNKNOWN, T.PARITY, T.UNSUPPORTED, T.KNOWN, T.UNKNOWN)]
    case = K.build("rejected replies", items)
    with _table() as table:
        out, recs = _run(table, T.Table(), case)
        assert out["state"].tolist() == [T.NOT_COMMB] + [T.AMBIGUOUS] * 3 + [T.SETTLED, T.AMBIGUOUS]
        assert out[[1, 2, 3, 5]].tobytes() == case["commb"][[1, 2, 3, 5]].tobytes()
        assert int(recs["n_commb"][0]) == 1 and int(recs["n_ambiguous"][0]) == 0
        assert (table.points()["flags"][[1, 2, 3, 5]] == A.ADSB_TRACK_UNADDRESSED).all()


def test_other_updates_leave_the_commb_records_alone_and_update_commb_is_update_modes(gpu, big):
    case = big[0]
    n = 1200
    frames, recs, commb = _frames(case)[:n], case["recs"][:n].view(A.MODES_DTYPE), case["commb"][:n].view(A.COMMB_DTYPE)
    sq = np.flatnonzero(np.isin(recs["df"], (17, 18)) & (recs["kind"] == T.SELF))
    kw = dict(seconds_per_sample=SPS, max_frames=1 << 12)
    with A.AdsbDemod(max_samples=1024, max_out=16) as d, A.TrackTable(d, **kw) as table, A.TrackTable(d, **kw) as bare:
        for t in (table, bare):
            t.summaries_reserve()
            t.mlat_reserve(1000.0)
            t.modes_reserve()
        table.commb_reserve()
        # update_commb gives everything update_modes gives
        table.update(frames[:600], 0, modes=recs[:600], commb=commb[:600])
        bare.update(frames[:600], 0, modes=recs[:600])
        for name in ("points", "summaries", "modes", "last_heard", "velocity"):
            assert getattr(table, name)().tobytes() == getattr(bare, name)().tobytes(), name
        assert table.aircraft()[0].tobytes() == bare.aircraft()[0].tobytes()
        held, held_frames = table.commb().tobytes(), table.frame_commb().tobytes()
        assert held != EMPTY * (len(held) // 128)
        # update, update_modes and update_mlat of the reserved table leave the commb records and the per-frame output alone
        fixes = np.zeros(600, dtype=A.MLAT_FIX_DTYPE)
        table.update(frames[sq[sq >= 600]], 0)
        table.update(frames[600:n], 0, modes=recs[600:n])
        table.update(frames[sq[sq >= 600]][:600], 0, mlat=fixes[:min(600, (sq >= 600).sum())])
        assert table.commb().tobytes() == held and table.frame_commb().tobytes() == held_frames
        # without either reserve: every commb entry point says so
        for call in (lambda: bare.commb(), lambda: bare.commb_device(), lambda: bare.frame_commb(),
                     lambda: bare.update(frames[:10], 0, modes=recs[:10], commb=commb[:10]),
                     lambda: bare.update(frames[:0], 0, modes=recs[:0], commb=commb[:0])):
            with pytest.raises(A.AdsbError) as e:
                call()
            assert e.value.code == A.ADSB_E_STATE
    with _table(max_frames=64, reserve=False) as table:                       # the commb reserve without the modes reserve
        table.commb_reserve()
        with pytest.raises(A.AdsbError) as e:
            table.update(frames[:10], 0, modes=recs[:10], commb=commb[:10])
        assert e.value.code == A.ADSB_E_STATE
        table.modes_reserve()
        with pytest.raises(A.AdsbError) as e:
            table.frame_commb()                                               # no update_commb yet
        assert e.value.code == A.ADSB_E_STATE
        L = _lib.load()
        assert L.adsb_track_table_update_commb(table._h, frames.ctypes.data, recs.ctypes.data, commb.ctypes.data, None, None,
                                               65, 0) == A.ADSB_E_CAPACITY
        with pytest.raises(A.AdsbError) as e:
            table.update(frames[:10], 0, modes=recs[:10], commb=commb[:10], mlat=fixes[:10])    # no mlat reserve
        assert e.value.code == A.ADSB_E_STATE
        table.update(frames[:0], 0, modes=recs[:0], commb=commb[:0])          # n = 0 is fine, and an empty list
        assert len(table.frame_commb()) == 0 and len(table.commb()) == 0
        table.commb_reserve(max_age_s=1.0)                                    # a second reserve changes nothing
        table.update(frames[:64], 0, modes=recs[:64], commb=commb[:64])
        model = T.Table()
        T.same_frames(table.frame_commb(), model.update(case["frames"][:64], case["recs"][:64], case["commb"][:64]))


def test_the_limits_of_the_reserve_are_used(gpu):
    first = K.build("a velocity message alone", [(K.ground_frame(K.A, -470, 0, vr=0), K.A, T.SELF)])      # 430 + 40 kt
    second = K.build("the reply alone", [(K.reply(K.BOTH), K.A, T.KNOWN)], offsets=[2000])
    age = 2000.0 * SPS
    for cfg, want in ((dict(), T.SETTLED), (dict(max_speed_diff_kt=39), T.AMBIGUOUS), (dict(max_age_s=age), T.SETTLED),
                      (dict(max_age_s=float(np.nextafter(age, 0.0))), T.AMBIGUOUS),
                      (dict(max_speed_diff_kt=39, max_vrate_diff_fpm=6000), T.AMBIGUOUS)):
        with _table(max_frames=64, cfg=cfg) as table:
            model = T.Table(cfg=cfg)
            _run(table, model, first)
            out, _ = _run(table, model, second)
            assert int(out["state"][0]) == want, cfg


# ---- (e) host or device memory, each list on its own ---------------------------------------------------------------------
def _hip_runtime():
    """The HIP runtime this process already holds (the one libadsb_hip.so is bound to), for a plain hipMemcpy."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path:
            hip = C.CDLL(path)
            hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            return hip
    raise RuntimeError("no HIP runtime mapped")


def test_memory_sides(gpu, big):
    case, whole_out, whole_recs = big
    n = 1500
    host = {"frames": _frames(case)[:n].copy(), "recs": case["recs"][:n].copy(), "commb": case["commb"][:n].copy()}
    want_out, want_recs, _ = K.run_model(dict(case, frames=case["frames"][:n], recs=case["recs"][:n], commb=case["commb"][:n]))
    with _table(max_frames=1 << 11) as table:
        hip, dev = _hip_runtime(), {}
        for k, v in host.items():
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), v.nbytes) == 0 and hip.hipMemcpy(p, v.ctypes.data, v.nbytes, 1) == 0
            dev[k] = p.value
        for combo in range(8):
            ptr = {k: (dev[k] if combo >> b & 1 else host[k].ctypes.data) for b, k in enumerate(host)}
            table.reset()
            table.update_device(ptr["frames"], n, 0, modes_ptr=ptr["recs"], commb_ptr=ptr["commb"])
            T.same_frames(table.frame_commb(), want_out, combo)
            T.same_records(table.commb(), want_recs, combo)
        table.reset()                                                    # waits: nothing reads the lists any more
        for p in dev.values():
            assert hip.hipFree(p) == 0


# ---- (f) wire input -> modes_of -> commb_of -> update_commb, all on one context --------------------------------------------
def test_the_chain_on_one_context(gpu, oracle):
    from tests import velocity_traffic as V
    from tests import wire_in_short_model as S
    adsb = 0x4B1234
    msgs = [V.velocity_frame(oracle, adsb, 1, dew=1, vew=414, dns=1, vns=121, vrsrc=1, svr=0, vr=1),   # 413 W, 120 S, level
            MM.reply(20, adsb, low3=0, b1=2, field=MM.field_of(Q=1) | 0x0A80, rest=K.BOTH),
            MM.reply(21, adsb, low3=0, b1=2, field=MM.field_of(A4=1, B2=1, C1=1), rest=CM.mb_17([7, 9, 16, 24])),
            MM.reply(20, 0x3C0001, low3=0, b1=2, field=MM.field_of(Q=1) | 0x0A80, rest=K.BOTH)]       # nobody's: UNKNOWN
    stream = b"".join(S.beast_frame(b"3", 6 * (1000 + 4000 * k), 40, m) for k, m in enumerate(msgs))
    with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d, \
            A.TrackTable(d, max_aircraft=16, max_frames=64, seconds_per_sample=SPS) as table:
        table.modes_reserve()
        table.commb_reserve()
        win = d.wire_in_of(stream, filter="short")
        n = len(win.frames)
        assert n == 4
        frames_dev = d.wire_in_device()[0]
        d.modes_of_async((frames_dev, n))
        d.commb_of_async((frames_dev, n))
        table.update_device(frames_dev, n, 0, modes_ptr=d.modes_device()[0], commb_ptr=d.commb_device()[0])
        stateless, _ = d.fetch_commb()
        mrec = d.fetch_modes()[0]
        assert mrec["kind"].tolist() == [T.SELF, T.KNOWN, T.KNOWN, T.UNKNOWN]
        assert stateless["state"].tolist() == [T.NOT_COMMB, T.AMBIGUOUS, T.ONE, T.AMBIGUOUS]
        assert not stateless["value"][1].any()                                # the stateless stage has nothing to say
        out = table.frame_commb()
        assert out["state"].tolist() == [T.NOT_COMMB, T.SETTLED, T.ONE, T.AMBIGUOUS] and int(out["bds"][1]) == 0x50
        assert out[[0, 2, 3]].tobytes() == stateless[[0, 2, 3]].tobytes()
        assert table.aircraft()[0]["icao"].tolist() == [adsb]
        rec = table.commb()[0]
        assert int(rec["bds50"]["settled"]) == 1 and int(rec["bds50"]["value"][2]) == 430 and int(rec["n_settled"]) == 1
        assert int(rec["n_commb"]) == 2 and int(rec["capability"]) == int(out["word"][2]) != 0
        phys = A.aircraft_commb_physical(table.commb())
        assert phys["ground_speed_kt"][0] == 430.0 and phys["bds50_settled"][0] == 1.0 and np.isnan(phys["mach"][0])
        assert abs(phys["true_track_deg"][0] - 1444 * 90 / 512) < 1e-9
        model = T.Table(max_aircraft=16)
        want = model.update(win.frames.view(CM.FRAME_DTYPE), mrec.view(MM.REC_DTYPE), stateless.view(CM.REC_DTYPE))
        T.same_frames(out, want)
        T.same_records(table.commb(), model.records())


# ---- (g) the tool ---------------------------------------------------------------------------------------------------------
def test_replay_prints_the_settled_ground_speed(gpu, oracle, tmp_path):
    """tools/replay.py --beast-in --modes --commb --aircraft on one recording: six more columns, the settled value marked;
    without --commb the table is the one it was"""
    import os
    import subprocess
    import sys
    from tests import velocity_traffic as V
    from tests import wire_in_short_model as S
    adsb = 0x4B1234
    msgs = [V.velocity_frame(oracle, adsb, 1, dew=1, vew=414, dns=1, vns=121, vrsrc=1, svr=0, vr=1),
            MM.reply(20, adsb, low3=0, b1=2, field=MM.field_of(Q=1) | 0x0A80, rest=K.BOTH),
            MM.reply(20, adsb, low3=0, b1=2, field=MM.field_of(Q=1) | 0x0A80, rest=CM.mb_40(mcp=0x555, baro=0x333))]
    path = tmp_path / "one.beast"
    path.write_bytes(b"".join(S.beast_frame(b"3", 6 * (1000 + 4000 * k), 40, m) for k, m in enumerate(msgs)))
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "replay.py")
    runs = [subprocess.run([sys.executable, tool, str(path), "--beast-in", "--modes", "--aircraft"] + more, capture_output=True,
                           text=True, timeout=120) for more in ([], ["--commb"])]
    assert runs[0].returncode == 0 and runs[1].returncode == 0, (runs[0].stderr, runs[1].stderr)
    plain, wide = ([line.split("\t") for line in r.stdout.splitlines()] for r in runs)
    assert len(plain) == len(wide) == 2 and len(plain[0]) == 12
    assert wide[0] == plain[0] + list(A.AIRCRAFT_COMMB_COLUMNS) and wide[1][:12] == plain[1]
    assert wide[1][12:] == [str(16 * 0x555), f"{(8000 + 0x333) / 10:.1f}", "430/254*", "n/a", "n/a", "n/a"]
