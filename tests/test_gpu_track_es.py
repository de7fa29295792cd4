"""Extended squitter status per aircraft on the device (adsb_track_table_es_reserve / update_es / fetch_es /
fetch_frame_es) against tests/track_es_model.py, a sequential model, and against the CPU mirror, byte for byte: every
field is an integer or the store's frame time, so nothing needs a tolerance.  Lists are tests/track_es_cases.py's, at
most 4097 frames."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from tests import commb_model as CM
from tests import es_model as M
from tests import modes_model as MM
from tests import track_es_cases as K
from tests import track_es_model as T

pytestmark = pytest.mark.gpu
SPS = K.SPS
EMPTY = T.record(T.empty()).tobytes()


@contextlib.contextmanager
def _table(max_frames=1 << 13, reserve=True, keyed=False, max_age_s=None, **kw):
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        with A.TrackTable(d, seconds_per_sample=SPS, max_frames=max_frames, **kw) as table:
            if keyed:
                table.modes_reserve()
            if reserve:
                table.es_reserve(**({} if max_age_s is None else dict(max_age_s=max_age_s)))
            yield table


def _frames(case):
    return np.ascontiguousarray(case["frames"]).view(A.FRAME_DTYPE)


def _update(table, case, lo=0, hi=None, base=0, keyed=False):
    hi = len(case["frames"]) if hi is None else hi
    more = dict(modes=case["recs"][lo:hi].view(A.MODES_DTYPE)) if keyed else {}
    table.update(_frames(case)[lo:hi], base, es=case["es"][lo:hi].view(A.ES_DTYPE), **more)
    return table.frame_es()


def _run(table, model, case, cuts=(), keyed=False, bases=None, what=""):
    """The case through the table and the model, cut alike; the per-frame outputs and the side records must agree."""
    edges = [0] + list(cuts) + [len(case["frames"])]
    got, want = [], []
    for k, (lo, hi) in enumerate(zip(edges, edges[1:])):
        base = 0 if bases is None else bases[k]
        got.append(_update(table, case, lo, hi, base, keyed))
        want.append(model.update(case["frames"][lo:hi], case["es"][lo:hi], case["recs"][lo:hi] if keyed else None, base))
        assert len(got[-1]) == hi - lo
    got, want = np.concatenate(got), np.concatenate(want)
    T.same_frames(got, want, (what, case["name"], cuts))
    assert table.aircraft()[0]["icao"].tolist() == sorted(model.state)
    recs = table.es()
    assert recs.dtype == A.AIRCRAFT_ES_DTYPE
    T.same_records(recs, model.records(), (what, case["name"], cuts))
    return got, recs


def _mirror(case, keyed=False, **kw):
    _, recs, out = A.host_track_es(_frames(case), case["es"].view(A.ES_DTYPE), case["recs"].view(A.MODES_DTYPE) if keyed else None,
                                   SPS, **kw)
    return out, recs


@pytest.fixture(scope="module")
def big():
    """4097 frames over 24 aircraft that reach every row of the integrity table and both STALE flags"""
    case = K.mix(4097)
    out, records, table = K.run_model(case)
    K.reaches_everything(table)
    return case, out, records


# ---- (a) the smallest shapes where the scans and the merge can go wrong ---------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4097])
def test_list_lengths(gpu, big, n):
    case = big[0] if n == 4097 else K.mix(n, seed=n)
    assert len(case["frames"]) == n
    with _table() as table:
        out, recs = _run(table, T.Table(), case)
        mirror_out, mirror_recs = _mirror(case)
        T.same_frames(out, mirror_out)
        T.same_records(recs, mirror_recs)
        assert len(out) == n and (n == 0) == (len(recs) == 0)
    if n == 1:                                                   # a single position alone, and a single frame that is not counted
        for msg in (K.position(K.A, 11, 1), K.position(K.A, 11, 1, df=18, low3=2), MM.reply(20, K.A, rest=bytes(7))):
            with _table() as table:
                _run(table, T.Table(), K.build("one frame", [msg]))


def test_one_aircraft_across_scan_tiles(gpu):
    case = K.one_aircraft_across_tiles(4097)
    K.claims_hold(case)
    with _table() as table:
        out, recs = _run(table, T.Table(), case)
        K.claims_hold(case, out=out)
        assert len(recs) == 1 and int(recs["n_es"][0]) == 4097 and int(recs["n_position"][0]) == 3
        assert (int(recs["nic"][0]), int(recs["rc_dm"][0])) == (3, 74080)
        mirror_out, mirror_recs = _mirror(case)
        T.same_frames(out, mirror_out)
        T.same_records(recs, mirror_recs)


def test_4097_aircraft_of_one_frame_each(gpu):
    case = K.many_aircraft(4097)
    with _table(max_aircraft=8192) as table:
        out, recs = _run(table, T.Table(), case)
        K.claims_hold(case, out=out)
        assert len(recs) == 4097 and (recs["n_es"] == 1).all() and not (out["flags"] & T.VERSIONED).any()


@pytest.mark.parametrize("keyed", [False, True], ids=["plain", "keyed"])
@pytest.mark.parametrize("case", K.small_cases() + [K.keyed_rejects()], ids=lambda c: c["name"])
def test_constructed_lists(gpu, case, keyed):
    if case["name"] == "keyed path rejects" and not keyed:
        case = dict(case, claim=None)                            # its claims are the keyed path's
    K.claims_hold(case, keyed=keyed)
    with _table(keyed=keyed) as table:
        out, recs = _run(table, T.Table(), case, keyed=keyed)
        K.claims_hold(case, out=out)
        mirror_out, mirror_recs = _mirror(case, keyed)
        T.same_frames(out, mirror_out)
        T.same_records(recs, mirror_recs)


def test_age_edges_and_the_reserves_limit(gpu):
    case, far = K.age_edges(), K.infinite_age()
    stale = T.COUNTED | T.POSITION | T.VERSIONED | T.STALE_A
    for max_age_s, want in ((K.AGE, (stale & ~T.STALE_A, stale)), (float(np.nextafter(K.AGE, 0.0)), (stale, stale)),
                            (None, (stale & ~T.STALE_A, stale))):                      # the default is 60 s = AGE
        with _table(max_frames=64, max_age_s=max_age_s) as table:
            out, _ = _run(table, T.Table(**({} if max_age_s is None else dict(max_age_s=max_age_s))), case)
            assert tuple(out["flags"][1:].tolist()) == want, max_age_s
    for max_age_s, want in ((math.inf, (9, 750)), (None, (8, 1852))):
        with _table(max_frames=64, max_age_s=max_age_s) as table:
            out, _ = _run(table, T.Table(**({} if max_age_s is None else dict(max_age_s=max_age_s))), far)
            assert (int(out["nic"][1]), int(out["rc_dm"][1])) == want
    L = _lib.load()
    with _table(max_frames=64, reserve=False) as table:
        for bad in (math.nan, -1.0):
            cfg = _lib.AdsbEsTrackCfg(bad)
            assert L.adsb_track_table_es_reserve(table._h, C.byref(cfg)) == A.ADSB_E_ARG
        assert L.adsb_track_table_es_reserve(table._h, None) == A.ADSB_OK            # NULL: 60 s
        table.es_reserve(max_age_s=1.0)                                                 # a second reserve changes nothing
        out, _ = _run(table, T.Table(), case)
        assert tuple(out["flags"][1:].tolist()) == (stale & ~T.STALE_A, stale)


def test_negative_age_is_stale(gpu):
    first, base1, second, base2 = K.negative_age()
    with _table(max_frames=64) as table:
        model = T.Table()
        _run(table, model, first, bases=[base1])
        out, recs = _run(table, model, second, bases=[base2])
        K.claims_hold(second, out=out)
        assert recs["position_time"][0] == 1.0 and recs["nic_a_time"][0] == 10.0


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


def test_held_state_and_the_lists_own(gpu):
    first = K.build("a status alone", [K.status(K.A, 2, nic_a=1)])
    held = K.build("the position alone", [K.position(K.A, 11, 1)], offsets=[20 * K.STEP])
    own = K.build("a newer status and the position", [K.status(K.A, 1, nic_a=0), K.position(K.A, 11, 1)],
                  offsets=[19 * K.STEP, 20 * K.STEP])
    for second, want in ((held, (9, 750, 2)), (own, (8, 1852, 1))):
        with _table(max_frames=64) as table:
            model = T.Table()
            _run(table, model, first)
            out, recs = _run(table, model, second)
            assert (int(out["nic"][-1]), int(out["rc_dm"][-1]), int(out["version"][-1])) == want
            assert (int(recs["nic"][0]), int(recs["rc_dm"][0]), int(recs["version"][0])) == want


# ---- (c) a full table, expire, reset, held from before the reserve --------------------------------------------------------
def test_full_table_turns_away_and_counts_nothing(gpu, big):
    case = big[0]
    with _table(max_aircraft=8) as table:
        model = T.Table(max_aircraft=8)
        out, recs = _run(table, model, case, [1500])
        assert len(recs) == 8 and table.aircraft()[1] & 1                  # ADSB_TRACK_TABLE_FULL
        turned = (table.points()["flags"] & A.ADSB_TRACK_UNTRACKED) != 0
        assert turned.any() and not out[1500:].view("<u8")[turned].any()


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


def test_expire_and_reset_forget_the_held_version_and_supplements(gpu):
    first = K.build("status and position of A", [K.status(K.A, 2, nic_a=1), K.position(K.A, 11, 1)])
    other = K.build("another aircraft, later", [K.status(K.B, 1, nic_a=1), K.position(K.B, 16)], offsets=[60_000_000, 60_000_100])
    late = K.build("a position of A alone, later", [K.position(K.A, 11, 1)], offsets=[60_000_200])
    with _table(max_aircraft=4, max_frames=64) as table:
        model = T.Table(max_aircraft=4)
        _run(table, model, first)
        _run(table, model, other)
        table.expire(10.0)                                                    # A was heard last at 1 ms, B at 30 s
        model.expire([K.A])
        assert table.aircraft()[0]["icao"].tolist() == [K.B]
        T.same_records(table.es(), model.records(), "after expire")           # B's record moved to slot 0 with it
        assert int(table.es()["nic"][0]) == 3
        out, recs = _run(table, model, late)                                  # re-admitted: nothing is known any more
        assert out["flags"][0] == T.COUNTED | T.POSITION and (int(out["nic"][0]), int(out["rc_dm"][0])) == (0, 1852)
        k = sorted((K.A, K.B)).index(K.A)
        assert int(recs["n_es"][k]) == 1 and math.isnan(recs["version_time"][k])
        table.reset()                                                         # every place empty, also those no aircraft holds
        assert len(table.es()) == 0
        raw = np.zeros(4, dtype=A.AIRCRAFT_ES_DTYPE)
        assert _hip_runtime().hipMemcpy(raw.ctypes.data, table.es_device(), raw.nbytes, 2) == 0     # device to host
        assert raw.tobytes() == EMPTY * 4
        with pytest.raises(A.AdsbError) as e:
            table.frame_es()                                                  # no update_es since the reset
        assert e.value.code == A.ADSB_E_STATE
        model = T.Table(max_aircraft=4)
        out, _ = _run(table, model, late)
        assert out["flags"][0] == T.COUNTED | T.POSITION
        out, _ = _run(table, model, first, bases=[70_000_000])
        assert (int(out["nic"][1]), int(out["rc_dm"][1])) == (9, 750)


def test_held_from_before_the_reserve(gpu):
    first = K.build("status and position of A", [K.status(K.A, 2, nic_a=1), K.position(K.A, 11, 1)])
    second = K.build("the position alone", [K.position(K.A, 11, 1)], offsets=[20 * K.STEP])
    with _table(max_frames=64, reserve=False) as table:
        table.update(_frames(first), 0)                                       # a plain update: the status is not kept
        table.es_reserve()
        got = table.es()
        assert len(got) == 1 and got.tobytes() == EMPTY
        model = T.Table()
        model.update(first["frames"])
        out, recs = _run(table, model, second)
        assert out["flags"][0] == T.COUNTED | T.POSITION and int(recs["n_es"][0]) == 1


# ---- (d) what the reserve leaves alone, and what update_es is --------------------------------------------------------------
def test_other_updates_leave_the_es_records_alone_and_update_es_is_the_update_it_extends(gpu, big):
    case = big[0]
    n = 1200
    frames, recs, es = _frames(case)[:n], case["recs"][:n].view(A.MODES_DTYPE), case["es"][:n].view(A.ES_DTYPE)
    commb = CM.commb(case["frames"][:n])["recs"].view(A.COMMB_DTYPE)
    levels = np.zeros(n, dtype=A.LEVEL_DTYPE)
    kw = dict(seconds_per_sample=SPS, max_frames=1 << 12)
    with A.AdsbDemod(max_samples=1024, max_out=16) as d, A.TrackTable(d, **kw) as table, A.TrackTable(d, **kw) as bare:
        for t in (table, bare):
            t.summaries_reserve()
            t.levels_reserve()
            t.modes_reserve()
            t.commb_reserve()
        table.es_reserve()
        same = ("points", "summaries", "modes", "commb", "levels", "last_heard", "velocity")
        for k, more in enumerate((dict(), dict(levels=levels[:600]), dict(modes=recs[:600]), dict(modes=recs[:600], commb=commb[:600]),
                                  dict(modes=recs[:600], levels=levels[:600]))):
            table.reset(), bare.reset()
            table.update(frames[:600], 0, es=es[:600], **more)
            bare.update(frames[:600], 0, **more)
            for name in same:
                assert getattr(table, name)().tobytes() == getattr(bare, name)().tobytes(), (k, name)
            assert table.aircraft()[0].tobytes() == bare.aircraft()[0].tobytes(), k
            if "commb" in more:
                assert table.frame_commb().tobytes() == bare.frame_commb().tobytes()
            model = T.Table()
            T.same_frames(table.frame_es(), model.update(case["frames"][:600], case["es"][:600], case["recs"][:600] if "modes" in more else None))
            T.same_records(table.es(), model.records(), k)
        held, held_frames = table.es().tobytes(), table.frame_es().tobytes()
        assert held != EMPTY * (len(held) // 256)
        # update, update_levels, update_modes and update_commb of the reserved table leave the es records and the per-frame
        # output alone (no aircraft is admitted: the same 600 frames again)
        table.update(frames[:600], 0)
        table.update(frames[:600], 0, levels=levels[:600])
        table.update(frames[:600], 0, modes=recs[:600])
        table.update(frames[:600], 0, modes=recs[:600], commb=commb[:600])
        assert table.es().tobytes() == held and table.frame_es().tobytes() == held_frames
        # without the reserve: every es entry point says so
        for call in (lambda: bare.es(), lambda: bare.es_device(), lambda: bare.frame_es(),
                     lambda: bare.update(frames[:10], 0, es=es[:10]), lambda: bare.update(frames[:0], 0, es=es[:0])):
            with pytest.raises(A.AdsbError) as e:
                call()
            assert e.value.code == A.ADSB_E_STATE
    L = _lib.load()
    with _table(max_frames=64) as table:                                      # the es reserve alone
        with pytest.raises(A.AdsbError) as e:
            table.frame_es()                                                  # no update_es yet
        assert e.value.code == A.ADSB_E_STATE
        for more in (dict(modes=recs[:10]), dict(levels=levels[:10]), dict(mlat=np.zeros(10, dtype=A.MLAT_FIX_DTYPE))):
            with pytest.raises(A.AdsbError) as e:
                table.update(frames[:10], 0, es=es[:10], **more)              # no modes / levels / mlat reserve
            assert e.value.code == A.ADSB_E_STATE, more
        table.modes_reserve()
        with pytest.raises(A.AdsbError) as e:
            table.update(frames[:10], 0, es=es[:10], modes=recs[:10], commb=commb[:10])     # no commb reserve
        assert e.value.code == A.ADSB_E_STATE
        args = (frames.ctypes.data, es.ctypes.data)
        assert L.adsb_track_table_update_es(table._h, *args, None, commb.ctypes.data, None, None, 10, 0) == A.ADSB_E_ARG
        assert L.adsb_track_table_update_es(table._h, None, es.ctypes.data, None, None, None, None, 10, 0) == A.ADSB_E_ARG
        assert L.adsb_track_table_update_es(table._h, frames.ctypes.data, None, None, None, None, None, 10, 0) == A.ADSB_E_ARG
        assert L.adsb_track_table_update_es(table._h, *args, None, None, None, None, 65, 0) == A.ADSB_E_CAPACITY
        assert L.adsb_track_table_update_es(table._h, None, None, None, None, None, None, 0, 0) == A.ADSB_OK
        assert len(table.frame_es()) == 0 and len(table.es()) == 0            # n = 0 is fine, and an empty list
        assert L.adsb_track_table_fetch_es(table._h, None, 4, None) == A.ADSB_E_ARG
        assert L.adsb_track_table_fetch_frame_es(table._h, None, 4, None) == A.ADSB_E_ARG
        table.update(frames[:64], 0, es=es[:64])
        T.same_frames(table.frame_es(), T.Table().update(case["frames"][:64], case["es"][:64]))


# ---- (e) host or device memory, each list on its own ---------------------------------------------------------------------
def test_memory_sides(gpu, big):
    case, whole_out, whole_recs = big
    n = 1500
    host = {"frames": _frames(case)[:n].copy(), "es": case["es"][:n].copy()}
    want_out, want_recs, _ = K.run_model(dict(case, frames=case["frames"][:n], es=case["es"][:n], recs=case["recs"][:n]))
    with A.AdsbDemod(max_samples=1024, max_out=16) as d, A.TrackTable(d, seconds_per_sample=SPS, max_frames=1 << 11) as table:
        table.es_reserve()
        hip, dev = _hip_runtime(), {}
        for k, v in host.items():
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), v.nbytes) == 0 and hip.hipMemcpy(p, v.ctypes.data, v.nbytes, 1) == 0
            dev[k] = p.value
        for combo in range(4):
            ptr = {k: (dev[k] if combo >> b & 1 else host[k].ctypes.data) for b, k in enumerate(host)}
            table.reset()
            table.update_device(ptr["frames"], n, 0, es_ptr=ptr["es"])
            T.same_frames(table.frame_es(), want_out, combo)
            T.same_records(table.es(), want_recs, combo)
        for frames_ptr in (dev["frames"], host["frames"].ctypes.data):        # adsb_es_device's pointer, the ctx's scratch
            table.reset()
            d.es_of_async((dev["frames"], n))
            table.update_device(frames_ptr, n, 0, es_ptr=d.es_device()[0])
            T.same_frames(table.frame_es(), want_out, "es_device")
            T.same_records(table.es(), want_recs, "es_device")
        table.reset()                                                    # waits: nothing reads the lists any more
        for p in dev.values():
            assert hip.hipFree(p) == 0


# ---- (f) wire input -> modes_of -> commb_of -> es_of -> update_es, all on one context --------------------------------------
def test_the_chain_on_one_context(gpu):
    from tests import wire_in_short_model as S
    other = 0x3C0001
    msgs = [K.status(K.A, 2, nic_a=1), K.position(K.A, 11, 1), MM.reply(20, K.A, low3=0, b1=2, field=MM.field_of(Q=1) | 0x0A80),
            K.position(K.B, 13, 1), K.target(K.A), MM.reply(20, other, low3=0, b1=2, field=MM.field_of(Q=1) | 0x0A80)]
    stream = b"".join(S.beast_frame(b"3", 6 * (1000 + 4000 * k), 40, m) for k, m in enumerate(msgs))
    with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d, \
            A.TrackTable(d, max_aircraft=16, max_frames=64, seconds_per_sample=SPS) as table:
        table.modes_reserve()
        table.commb_reserve()
        table.es_reserve()
        win = d.wire_in_of(stream, filter="short")
        n = len(win.frames)
        assert n == 6
        frames_dev = d.wire_in_device()[0]
        d.modes_of_async((frames_dev, n))
        d.commb_of_async((frames_dev, n))
        d.es_of_async((frames_dev, n))
        table.update_device(frames_dev, n, 0, modes_ptr=d.modes_device()[0], commb_ptr=d.commb_device()[0], es_ptr=d.es_device()[0])
        stateless, _ = d.fetch_es()                                           # nothing was fetched before this line
        mrec = d.fetch_modes()[0]
        assert mrec["kind"].tolist() == [MM.SELF, MM.SELF, MM.KNOWN, MM.SELF, MM.SELF, MM.UNKNOWN]
        assert stateless.tobytes() == M.es(win.frames.view(M.FRAME_DTYPE))["recs"].tobytes()
        out = table.frame_es()
        assert out["flags"].tolist() == [T.COUNTED, T.COUNTED | T.POSITION | T.VERSIONED, 0, T.COUNTED | T.POSITION, T.COUNTED, 0]
        assert (int(out["nic"][1]), int(out["rc_dm"][1])) == (9, 750) and (int(out["nic"][3]), int(out["rc_dm"][3])) == (0, 9260)
        assert table.aircraft()[0]["icao"].tolist() == sorted((K.A, K.B))
        model = T.Table(max_aircraft=16)
        want = model.update(win.frames.view(M.FRAME_DTYPE), stateless.view(M.REC_DTYPE), mrec.view(MM.REC_DTYPE))
        T.same_frames(out, want)
        T.same_records(table.es(), model.records())
        assert int(table.commb()["n_commb"][sorted((K.A, K.B)).index(K.A)]) == 1          # update_commb ran too
        phys = A.aircraft_es_physical(table.es())
        k = sorted((K.A, K.B)).index(K.A)
        assert abs(phys["rc_m"][k] - 75.0) < 1e-9 and phys["selected_altitude_ft"][k] == 32.0 * 531


def test_two_runs_give_the_same_bytes(gpu, big):
    case = big[0]
    got = []
    for _ in range(2):
        with _table() as table:
            out = _update(table, case, 0, 2000)
            out2 = _update(table, case, 2000, 4097)
            got.append((out.tobytes(), out2.tobytes(), table.es().tobytes()))
    assert got[0] == got[1]


# ---- (g) the tool ---------------------------------------------------------------------------------------------------------
def test_replay_prints_the_resolved_integrity(gpu, tmp_path):
    """tools/replay.py --beast-in --es --aircraft on one recording: eight more columns; an aircraft whose operational status
    was heard gets the resolved NIC and Rc, one whose status was not heard the type code's radius, marked; without --es the
    table is the one it was"""
    import os
    import subprocess
    import sys
    from tests import wire_in_short_model as S
    msgs = [K.status(K.A, 2, nic_a=1), K.position(K.A, 11, 1), K.position(K.B, 11, 1), K.emergency(K.A, 1, 7700), K.target(K.A)]
    path = tmp_path / "one.beast"
    path.write_bytes(b"".join(S.beast_frame(b"3", 6 * (1000 + 4000 * k), 40, m) for k, m in enumerate(msgs)))
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "replay.py")
    for mode in ([], ["--modes"]):
        runs = [subprocess.run([sys.executable, tool, str(path), "--beast-in", "--aircraft"] + mode + more, capture_output=True,
                               text=True, timeout=120) for more in ([], ["--es"])]
        assert runs[0].returncode == 0 and runs[1].returncode == 0, (runs[0].stderr, runs[1].stderr)
        plain, wide = ([line.split("\t") for line in r.stdout.splitlines()] for r in runs)
        assert len(plain) == len(wide) == 3
        width = len(plain[0])
        assert wide[0] == plain[0] + list(A.AIRCRAFT_ES_COLUMNS) and [w[:width] for w in wide[1:]] == plain[1:]
        rows = {w[0]: w[width:] for w in wide[1:]}
        assert rows[f"{K.A:x}"] == ["2", "9", "75.0", "10", "2", "1", "7700", "16992"]
        assert rows[f"{K.B:x}"] == ["n/a", "0?", "185.2?", "n/a", "n/a", "n/a", "n/a", "n/a"]


def test_replay_from_samples_and_from_avr(gpu, tmp_path):
    """--es --aircraft on a capture of samples (the synthetic stream as raw rtl_sdr bytes) and on AVR text: eight more
    columns, the rest of the table as it was, and the columns are what the mirror makes of the same frames"""
    import os
    import subprocess
    import sys
    from tests import wire_in_short_model as W
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "replay.py")
    iq = A.synth_fill_host(A.synth_default(seed=4242), A.ADSB_SAMPLE_I8, 0, 0, 200_000)
    samples = tmp_path / "synth.u8"
    samples.write_bytes((iq.view(np.uint8) ^ 0x80).tobytes())
    msgs = [K.status(K.A, 2, nic_a=1), K.position(K.A, 11, 1), K.position(K.B, 13, 1)]
    avr = tmp_path / "three.avr"
    avr.write_bytes(b"".join(W.avr_line(m, t=12_000 * (i + 1)) for i, m in enumerate(msgs)))
    for path, more in ((samples, []), (avr, ["--avr-in"])):
        runs = [subprocess.run([sys.executable, tool, str(path), "--aircraft"] + more + es, capture_output=True, text=True, timeout=120)
                for es in ([], ["--es"])]
        assert runs[0].returncode == 0 and runs[1].returncode == 0, (runs[0].stderr, runs[1].stderr)
        plain, wide = ([line.split("\t") for line in r.stdout.splitlines()] for r in runs)
        width = len(plain[0])
        assert len(plain) == len(wide) > 1 and wide[0] == plain[0] + list(A.AIRCRAFT_ES_COLUMNS)
        assert [w[:width] for w in wide] == plain and all(len(w) == width + 8 for w in wide)
    rows = {w[0]: w[width:] for w in wide[1:]}
    assert rows[f"{K.A:x}"][:3] == ["2", "9", "75.0"] and rows[f"{K.B:x}"][:3] == ["n/a", "0?", "926.0?"]
    with A.AdsbDemod(max_samples=20_240, max_out=20_240, host_staging=False) as d:      # the tool's own read of the file
        frames = d.replay_file(str(samples), _lib.ADSB_FILE_U8, chunk_len=20_000, carry=False, send_tail=False, max_frames=1 << 16)[0]
    icaos, side, _ = A.host_track_es(frames, A.host_es(frames)[0])
    want = dict(zip((f"{int(a):x}" for a in icaos), A.aircraft_es_columns(side)))
    text = subprocess.run([sys.executable, tool, str(samples), "--aircraft", "--es"], capture_output=True, text=True, timeout=120).stdout
    got = {line.split("\t")[0]: line.split("\t")[-8:] for line in text.splitlines()[1:]}
    assert got == want and len(got) > 5


def test_mlat_tool_on_the_device_prints_what_its_host_path_prints(gpu, oracle, tmp_path):
    """tools/mlat.py --modes --es --aircraft: update_es on the keyed path behind correlate, where the frames lie"""
    import os
    import subprocess
    import sys
    from tests import track_modes_cases as N
    args = N.recordings(N.network(oracle), tmp_path)
    tool = [sys.executable, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "mlat.py"),
            "--modes", "--es", "--commb", "--aircraft", "--max-iterations", "200"]
    dev = subprocess.run(tool + args, capture_output=True, text=True, timeout=120)
    host = subprocess.run(tool + ["--host"] + args, capture_output=True, text=True, timeout=120)
    assert dev.returncode == 0 and host.returncode == 0, (dev.stderr, host.stderr)
    cols = lambda text: [line.split("\t")[:1] + line.split("\t")[16:] for line in text.splitlines()]
    assert cols(dev.stdout) == cols(host.stdout) and len(cols(dev.stdout)) == 3 and len(cols(dev.stdout)[0]) == 1 + 6 + 8
