"""Mode S replies per aircraft on the device (adsb_track_table_modes_reserve / update_modes / fetch_modes) against
tests/track_modes_model.py, a sequential model, byte for byte: every field is an integer, a copied byte or the store's
frame time, so nothing needs a tolerance.  The main 128-byte record is checked against adsb_track_table_update on a
transformed list (every accepted reply as a DF17 frame of type code 0 with the reply's address, rejected frames
dropped), which is how the header defines it.  Lists are tests/modes_cases.py's, at most 4097 frames, with the records of
adsb_host_modes or records written by hand."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from tests import modes_cases as K
from tests import modes_model as MM
from tests import track_modes_cases as N
from tests import track_modes_model as M

pytestmark = pytest.mark.gpu
SPS = 0.5e-6
BASE = 1_000_000
EMPTY = M.record(M.empty()).tobytes()


class Traffic:
    """A frame list with its Mode S records (the CPU mirror's, with half of the address pool known)."""

    def __init__(self, frames, known=(), recs=None, base=BASE):
        self.frames = np.ascontiguousarray(frames).view(A.FRAME_DTYPE).copy()
        self.known = np.array(sorted(set(int(a) for a in known)), dtype=np.uint32)
        self.recs = A.host_modes(self.frames, known=self.known)[0] if recs is None else np.ascontiguousarray(recs, dtype=A.MODES_DTYPE)
        self.base = base
        assert len(self.recs) == len(self.frames)

    def __len__(self):
        return len(self.frames)

    def cut(self, lo, hi):
        return Traffic(self.frames[lo:hi], recs=self.recs[lo:hi], base=self.base)


def _random(n, seed, n_addresses=24):
    frames, pool = K.random_list(n, seed, n_addresses)
    return Traffic(frames, known=pool[::2].tolist())


@contextlib.contextmanager
def _table(max_frames=1 << 13, reserve=True, **kw):
    with A.AdsbDemod(max_samples=1024, max_out=16) as d:
        with A.TrackTable(d, seconds_per_sample=SPS, max_frames=max_frames, **kw) as table:
            if reserve:
                table.modes_reserve()
            yield table


def _check(table, model, tr, want, what=""):
    """The last update's points and the table's side records against the model's (want = model.update's result)."""
    flags, icao = want
    pts = table.points()
    assert len(pts) == len(tr)
    assert (pts["flags"] & ~np.uint32(M.NEW_POSITION) == flags).all(), (what, "point flags")
    assert (pts["icao"] == icao).all(), (what, "point icao")
    off = flags != 0
    assert (pts["flags"][off] == flags[off]).all() and not pts["latitude"][off].any() and not pts["longitude"][off].any()
    recs, tflags = table.aircraft()
    assert recs["icao"].tolist() == sorted(model.state), what
    assert tflags == model.flags, what
    got = table.modes()
    assert got.dtype == A.AIRCRAFT_MODES_DTYPE
    M.same_records(got, model.records(), what)
    return recs, got


def _run(table, model, tr, what="", **kw):
    table.update(tr.frames, tr.base, modes=tr.recs, **kw)
    return _check(table, model, tr, model.update(tr.frames, tr.recs, tr.base), what)


@pytest.fixture(scope="module")
def mixed():
    """4097 frames of every DF and kind over 24 addresses: the list most tests cut pieces from."""
    tr = _random(4097, 7)
    kinds = np.bincount(tr.recs["kind"], minlength=5)
    assert (kinds > 100).all() and len(set(tr.recs["df"].tolist())) > 20
    return tr


# ---- (a) the smallest shapes where the sort, the scan and the merge can go wrong ----------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4097])
def test_list_lengths(gpu, mixed, n):
    starts = (0,)
    if n < 3:                                                            # 1 and 2: an accepted and a rejected first frame
        starts = (int(np.flatnonzero(mixed.recs["kind"] <= 1)[0]), int(np.flatnonzero(mixed.recs["kind"] >= 2)[0]))
    for lo in starts:
        tr = mixed.cut(lo, lo + n)
        with _table() as table:
            _, got = _run(table, M.Table(), tr, (n, lo))
            if n == 4097:
                assert (got["flags"] & M.SQUITTER != 0).any() and (got["flags"] & M.SQUITTER == 0).any()
                assert (got["n_replies"] > 50).sum() >= 20 and (got["flags"] & M.CALLSIGN != 0).any()
                assert (got["flags"] & M.ALT != 0).any() and (got["flags"] & M.SQUAWK != 0).any()


def test_no_accepted_frame_at_all(gpu, mixed):
    bad = np.flatnonzero(mixed.recs["kind"] >= 2)[:600]
    tr = Traffic(mixed.frames[bad], recs=mixed.recs[bad])
    with _table() as table:
        table.summaries_reserve()
        _run(table, M.Table(), tr)
        pts = table.points()
        assert (pts["flags"] == A.ADSB_TRACK_UNADDRESSED).all() and (pts["icao"] == tr.recs["address"]).all()
        assert len(table.aircraft()[0]) == 0 and len(table.modes()) == 0 and len(table.changed()[0]) == 0
        sums = table.summaries()
        assert (sums["icao"] == tr.recs["address"]).all() and not sums["n_frames"].any()
        # and beside held aircraft: nothing moves
        ok = mixed.cut(0, 300)
        model = M.Table()
        _run(table, model, ok)
        before = (table.aircraft()[0].tobytes(), table.modes().tobytes(), table.last_heard().tobytes())
        _run(table, model, tr, "rejected after accepted")
        assert before == (table.aircraft()[0].tobytes(), table.modes().tobytes(), table.last_heard().tobytes())
        assert len(table.changed()[0]) == 0


def test_none_rejected(gpu, mixed):
    ok = np.flatnonzero(mixed.recs["kind"] <= 1)[:1000]
    tr = Traffic(mixed.frames[ok], recs=mixed.recs[ok])
    with _table() as table:
        _run(table, M.Table(), tr)
        assert not (table.points()["flags"] & (A.ADSB_TRACK_UNADDRESSED | A.ADSB_TRACK_UNTRACKED)).any()


def test_one_aircraft_longer_than_a_scan_block_and_300_at_one_offset(gpu):
    big, rng = 0x500000, np.random.default_rng(5)
    f25 = lambda k: MM.field_of(Q=1) | (0x80 * (k % 16)) | (k % 16)
    msgs, offsets = [], []
    for k in range(600):
        sort = k % 5
        msgs.append([MM.reply(4, big, low3=k % 8, field=f25(k)), MM.reply(5, big, low3=k % 6, field=0x0AAA ^ (k & 0xFF)),
                     MM.reply(20, big, low3=k % 4, field=f25(k + 3), rest=MM.callsign_mb("BIG%04d_" % k)), MM.all_call(big),
                     MM.reply(0, big, low3=4 * (k % 2), field=f25(k + 1))][sort])
        offsets.append(5 * k if k < 150 else 1000 if k < 450 else 1000 + 10 * (k - 449))   # 300 frames at one offset
    others = sorted(int(x) for x in rng.choice(np.arange(0x400000, 0x600000), size=100, replace=False))
    at = sorted(rng.choice(600, size=100, replace=False).tolist(), reverse=True)
    for icao, k in zip(others, at):                                      # one frame each, scattered through the big list
        msgs.insert(k, MM.reply(4, icao, field=f25(icao)))
        offsets.insert(k, offsets[k])
    tr = Traffic(MM.frame_list(msgs, offsets=np.array(offsets)), known=[big] + others)
    assert (tr.recs["kind"] <= 1).all() and (tr.recs["address"] == big).sum() == 600
    with _table() as table:
        model = M.Table()
        _, got = _run(table, model, tr)
        g = got[sorted(model.state).index(big)]
        assert g["n_replies"] == 600 and g["n_allcall"] == 120 and g["n_surveillance"] == 360 and g["n_airair"] == 120
        whole = got.tobytes()
        table.reset()
        model = M.Table()
        for lo, hi in ((0, 200), (200, 201), (201, 520), (520, len(tr))):  # cuts inside the run of equal offsets
            _run(table, model, tr.cut(lo, hi), (lo, hi))
        assert table.modes().tobytes() == whole


@pytest.mark.parametrize("field", ["alt", "squawk", "callsign", "status"])
@pytest.mark.parametrize("side", ["before", "after"])
def test_segment_straddles_the_256_thread_boundary(gpu, field, side):
    """One aircraft's segment lies across sorted positions 250..261; its newest frame of one sort sits on either side of
    256, and later frames of the other sorts must not disturb it."""
    low, mid = 0x100000, 0x200000
    winner = {"alt": MM.reply(4, mid, low3=1, field=MM.field_of(Q=1) | 0x0B85),
              "squawk": MM.reply(5, mid, low3=2, field=0x0AAA),
              "callsign": MM.reply(21, mid, low3=5, field=0x1555, rest=MM.callsign_mb("WINNER__")),
              "status": MM.reply(20, mid, low3=3, field=0)}[field]
    filler = MM.all_call(mid)                                            # DF11: writes none of the four
    msgs = [MM.reply(4, low + k, field=MM.field_of(Q=1) | 0x0A80) for k in range(250)]
    seg = [MM.reply(20, mid, low3=4, field=MM.field_of(Q=1) | 0x0C81, rest=MM.callsign_mb("FIRST___")),
           MM.reply(5, mid, field=0x1555)] + [filler] * 10
    seg[4 if side == "before" else 8] = winner                           # sorted position 254 or 258
    rng = np.random.default_rng(3)
    order = rng.permutation(250).tolist()
    mixed_in = []
    for k, m in enumerate(seg):                                          # the segment's frames spread through the list
        mixed_in += [msgs[i] for i in order[20 * k:20 * k + 20]] + [m]
    mixed_in += [msgs[i] for i in order[240:]]
    tr = Traffic(MM.frame_list(mixed_in), known=[mid] + [low + k for k in range(250)])
    assert (tr.recs["kind"] <= 1).all()
    with _table() as table:
        model = M.Table()
        _, got = _run(table, model, tr)
        g = got[250]
        assert g["n_replies"] == 12
        if field == "callsign":
            assert g["callsign"] == b"WINNER__"
        if field == "status":
            assert g["fs"] == 3 and g["flags"] & M.GROUND and g["flags"] & M.ALERT
        if field == "alt":
            assert g["altitude_ft"] == 25 * ((0x0B85 & 0x1F80) >> 2 | (0x0B85 & 0x20) >> 1 | (0x0B85 & 0xF)) - 1000
        if field == "squawk":
            assert g["squawk"] == MM.squawk(0x0AAA)


def test_addresses_zero_and_ffffff_and_a_parity_record_of_address_zero(gpu):
    _, frames, _ = K.edge_addresses()
    tr = Traffic(frames, known=[0])                                      # 0 from known_in: KNOWN from the first frame on
    assert tr.recs["kind"][0] == MM.KNOWN and tr.recs["address"][0] == 0
    bad = MM.squitter(0x123456)
    bad = bad[:13] + bytes([bad[13] ^ 1])
    more = Traffic(MM.frame_list([bad, MM.reply(4, 0, field=MM.field_of(Q=1) | 0x0A81), bytes([1 << 3]) + bytes(6)],
                                 offsets=np.array([5000, 5001, 5002])), known=[0])
    assert more.recs["kind"].tolist() == [MM.PARITY, MM.KNOWN, MM.UNSUPPORTED] and more.recs["address"][0] == 0
    with _table() as table:
        model = M.Table()
        recs, got = _run(table, model, tr)
        assert recs["icao"].tolist() == [0, 0xFFFFFF] and (got["n_replies"] > 0).all() and (got["flags"] & M.SQUITTER).all()
        zero_frames = int(recs["n_frames"][0])
        recs, got = _run(table, model, more, "a PARITY record of address 0 beside aircraft 0")
        assert int(recs["n_frames"][0]) == zero_frames + 1 and recs["icao"].tolist() == [0, 0xFFFFFF]
        pts = table.points()
        assert pts["flags"].tolist() == [A.ADSB_TRACK_UNADDRESSED, 0, A.ADSB_TRACK_UNADDRESSED] and pts["icao"].tolist() == [0, 0, 0]


# ---- (b) the main record: update_modes against update on the transformed list -------------------------------------------
def _levels(n, seed):
    rng = np.random.default_rng(seed)
    levels = np.zeros(n, dtype=A.LEVEL_DTYPE)
    levels["signal_sum"] = rng.integers(0, 1 << 38, size=n, dtype=np.uint64)
    levels["noise_sum"] = rng.integers(0, 1 << 38, size=n, dtype=np.uint64)
    levels["flags"] = (rng.random(n) >= 0.2).astype(np.uint16)
    return levels


def _fixes(n, seed):
    rng = np.random.default_rng(seed)
    fixes = np.zeros(n, dtype=A.MLAT_FIX_DTYPE)
    fixes["latitude"], fixes["longitude"] = 47.0 + rng.random(n), 8.0 + rng.random(n)
    fixes["height_m"], fixes["pdop"], fixes["n_used"] = 9000.0 + rng.random(n), 2.0, 4
    fixes["flags"] = np.where(rng.random(n) < 0.7, A.ADSB_MLAT_ATTEMPTED | A.ADSB_MLAT_CONVERGED | A.ADSB_MLAT_VALID,
                              A.ADSB_MLAT_ATTEMPTED | A.ADSB_MLAT_TOO_FEW)
    return fixes


SILENT = 0x000123                                                        # (a low address: admitted while there is room)
CRAFTED_TCS = [1, 2, 3, 4] + list(range(9, 19)) + [19]


def _differential_traffic(mixed, n=2000):
    """The first n frames of `mixed` with crafted frames among them: a velocity squitter, eight replies of an aircraft
    that only answers interrogations, and for each of six frequent aircraft DF20 and DF4 replies whose byte 4 would read
    as type codes 1-4 (identification), 9-18 (position) and 19 (velocity).  -> (Traffic, is_crafted_reply)"""
    addr = mixed.known.tolist()[:6]
    craft = [MM.squitter(addr[0], me=bytes([19 << 3 | 1, 0x44, 0x5A, 0x18, 0x88, 0x04, 0x10]))]     # a velocity message
    at = [3]
    for k in range(8):
        craft.append(MM.reply(4, SILENT, field=MM.field_of(Q=1) | 0x0A80) if k % 2 else
                     MM.reply(20, SILENT, field=0x0AAA, rest=bytes([9 << 3 | k, 1, 2, 3, 4, 5, 6])))
        at.append(50 + 230 * k)
    for k, tc in enumerate(CRAFTED_TCS):
        a = addr[k % len(addr)]
        mb = bytes([tc << 3 | (1 if tc == 19 else k & 7)]) + bytes([0x5A ^ k, 0xC3, 0x71 + k, 0xC3, 0x2C, 0xE0])
        for low in range(1 << 16):                                       # a DF4 whose parity byte (byte 4) reads as tc
            short = MM.overlay(bytes([4 << 3, low >> 8, 0x0A, low & 0xFF]), a)
            if short[4] >> 3 == tc:
                break
        craft += [MM.reply(20, a, low3=k % 6, field=MM.field_of(Q=1) | 0x0A80, rest=mb), short]
        at += [100 * k + 7, 100 * k + 9]
    frames = np.insert(mixed.frames[:n].copy(), at, MM.frame_list(craft).view(A.FRAME_DTYPE))
    frames["offset"] = np.arange(len(frames)) * 240
    tr = Traffic(frames, known=addr + [SILENT] + mixed.known.tolist())
    order = np.argsort(at, kind="stable")                                # np.insert: the k-th smallest index lands k places on
    where = np.empty(len(at), dtype=np.int64)
    where[order] = np.sort(at, kind="stable") + np.arange(len(at))
    crafted = np.zeros(len(tr), dtype=bool)
    crafted[where[9:]] = True
    b = tr.frames["bytes"][crafted]
    assert (tr.recs["kind"][crafted] == MM.KNOWN).all() and (b[0::2, 0] >> 3 == 20).all() and (b[1::2, 0] >> 3 == 4).all()
    assert (b[0::2, 4] >> 3).tolist() == CRAFTED_TCS == (b[1::2, 4] >> 3).tolist()
    return tr, crafted


def test_differential_against_update_on_the_transformed_list(gpu, mixed):
    """update_modes against update on the transformed list, with every reserve, over cuts and a full table.  Among the
    frames are replies whose byte 4 would read as an identification, position or velocity message: the field override
    is what is tested."""
    tr, crafted = _differential_traffic(mixed)
    silent_aircraft = SILENT
    other, keep = M.to_squitters(tr.frames, tr.recs)
    n_all = len(tr)
    levels, fixes = _levels(n_all, 1), _fixes(n_all, 2)
    fixes["flags"][tr.recs["address"] == silent_aircraft] = A.ADSB_MLAT_ATTEMPTED | A.ADSB_MLAT_CONVERGED | A.ADSB_MLAT_VALID
    site = (47.0, 8.0, 180.0)
    kw = dict(seconds_per_sample=SPS, max_frames=1 << 12, max_aircraft=20)   # some aircraft are turned away
    with A.AdsbDemod(max_samples=1024, max_out=16) as d, A.TrackTable(d, **kw) as table, A.TrackTable(d, **kw) as twin:
        for t in (table, twin):
            t.summaries_reserve()
            t.levels_reserve()
            t.fixes_reserve(site)
            t.mlat_reserve(1000.0)
        table.modes_reserve()
        table.modes_reserve()                                            # a second reserve changes nothing
        model = M.Table(max_aircraft=20)
        cuts = [0, 700, 700, 1500, n_all]
        for lo, hi in zip(cuts, cuts[1:]):
            part = tr.cut(lo, hi)
            sel = keep[(keep >= lo) & (keep < hi)]
            table.update(part.frames, part.base, modes=part.recs, levels=levels[lo:hi], mlat=fixes[lo:hi])
            want = model.update(part.frames, part.recs, part.base)
            assert not want[0][crafted[lo:hi]].any()                    # the crafted replies are counted, not turned away
            _check(table, model, part, want, (lo, hi))
            twin.update(other[(keep >= lo) & (keep < hi)], tr.base, levels=levels[sel], mlat=fixes[sel])
            (x, fx), (y, fy) = table.aircraft(), twin.aircraft()
            assert x.tobytes() == y.tobytes() and fx == fy, (lo, hi)
            assert table.last_heard().tobytes() == twin.last_heard().tobytes()
            assert table.velocity().tobytes() == twin.velocity().tobytes()
            assert table.levels().tobytes() == twin.levels().tobytes()
            assert table.fixes().tobytes() == twin.fixes().tobytes()
            assert table.mlat().tobytes() == twin.mlat().tobytes()
            assert all(p.tobytes() == q.tobytes() for p, q in zip(table.changed(), twin.changed()))
            rel = sel - lo
            assert table.points()[rel].tobytes() == twin.points().tobytes()
            assert table.summaries()[rel].tobytes() == twin.summaries().tobytes()
            assert table.frame_fixes()[rel].tobytes() == twin.frame_fixes().tobytes()
            assert table.frame_mlat()[rel].tobytes() == twin.frame_mlat().tobytes()
            # a frame that is not accepted: what an UNTRACKED frame gets, with the record's address as icao
            rej = np.setdiff1d(np.arange(hi - lo), rel)
            if len(rej):
                s, ff, fm = table.summaries()[rej], table.frame_fixes()[rej], table.frame_mlat()[rej]
                want_icao = part.recs["address"][rej]
                assert (s["icao"] == want_icao).all() and not s["n_frames"].any() and np.isnan(s["last_contact"]).all()
                assert (ff["icao"] == want_icao).all() and not ff["flags"].any() and not ff["latitude"].any()
                assert (fm["icao"] == want_icao).all() and not fm["flags"].any() and not fm["disagreement_m"].any()
        assert fx == A.ADSB_TRACK_TABLE_FULL and (table.velocity()["subtype"] != 0).any()
        k = x["icao"].tolist().index(silent_aircraft)                    # the point of the feature: a record and a fix
        side, fix = table.modes()[k], table.mlat()[k]
        assert not side["flags"] & M.SQUITTER and side["n_replies"] == 8 == x["n_frames"][k] == fix["n_valid"]
        assert fix["flags"] & A.ADSB_TRACK_MLAT_VALID and x["has_position"][k] == 0 and not x["callsign"][k]


def test_squitter_only_list_is_update_mlat(gpu, mixed):
    sq = np.flatnonzero((mixed.recs["kind"] == MM.SELF) & np.isin(mixed.recs["df"], (17, 18)))
    tr = Traffic(mixed.frames[sq], recs=mixed.recs[sq])
    n = len(tr)
    assert n > 500
    levels, fixes = _levels(n, 3), _fixes(n, 4)
    kw = dict(seconds_per_sample=SPS, max_frames=1 << 12, max_aircraft=12)
    with A.AdsbDemod(max_samples=1024, max_out=16) as d, A.TrackTable(d, **kw) as table, A.TrackTable(d, **kw) as twin:
        for t in (table, twin):
            t.summaries_reserve()
            t.levels_reserve()
            t.fixes_reserve((47.0, 8.0, 180.0))
            t.mlat_reserve(1000.0)
        table.modes_reserve()
        for lo, hi, with_fixes in ((0, 300, True), (300, n, False)):
            kwargs = dict(levels=levels[lo:hi], **({"mlat": fixes[lo:hi]} if with_fixes else {}))
            table.update(tr.frames[lo:hi], tr.base, modes=tr.recs[lo:hi], **kwargs)
            twin.update(tr.frames[lo:hi], tr.base, **kwargs)
            for name in ("points", "summaries", "frame_fixes", "frame_mlat", "levels", "fixes", "mlat", "last_heard", "velocity"):
                assert getattr(table, name)().tobytes() == getattr(twin, name)().tobytes(), (name, lo)
            assert table.aircraft()[0].tobytes() == twin.aircraft()[0].tobytes() and table.aircraft()[1] == twin.aircraft()[1]
            assert all(p.tobytes() == q.tobytes() for p, q in zip(table.changed(), twin.changed()))
        got = table.modes()
        assert (got["flags"] == M.SQUITTER).all() and not got["n_replies"].any() and set(got["last_df"].tolist()) <= {17, 18}


# ---- (c) cuts ------------------------------------------------------------------------------------------------------------
def _everything(table):
    return tuple(getattr(table, name)().tobytes() for name in ("modes", "levels", "mlat", "last_heard", "velocity")) + \
        (table.aircraft()[0].tobytes(),)


def test_cuts_give_identical_bytes(gpu, mixed):
    n = len(mixed)
    levels, fixes = _levels(n, 5), _fixes(n, 6)
    with _table() as table:
        table.levels_reserve()
        table.mlat_reserve(1000.0)

        def run(tr, lv, fx, edges):
            table.reset()
            for lo, hi in zip(edges, edges[1:]):
                table.update(tr.frames[lo:hi], tr.base, modes=tr.recs[lo:hi], levels=lv[lo:hi], mlat=fx[lo:hi])
            return _everything(table)

        short = mixed.cut(40, 80)
        whole = run(short, levels[40:80], fixes[40:80], [0, 40])
        for cut in range(41):
            assert run(short, levels[40:80], fixes[40:80], [0, cut, 40]) == whole, cut
        whole = run(mixed, levels, fixes, [0, n])
        rng = np.random.default_rng(17)
        for trial in range(3):
            edges = [0] + sorted(rng.choice(np.arange(1, n), size=5, replace=False).tolist()) + [n]
            assert run(mixed, levels, fixes, edges) == whole, edges
        assert run(mixed, levels, fixes, [0, n]) == whole                 # two runs give the same bytes


# ---- (d) host or device memory, each list on its own ---------------------------------------------------------------------
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


def test_memory_sides(gpu, mixed):
    n = 1500
    host = {"frames": mixed.frames[:n].copy(), "recs": mixed.recs[:n].copy(), "fixes": _fixes(n, 8), "levels": _levels(n, 9)}
    first = None
    with A.AdsbDemod(max_samples=1024, max_out=16) as d, A.TrackTable(d, seconds_per_sample=SPS, max_frames=1 << 11) as table:
        table.modes_reserve()
        table.levels_reserve()
        table.mlat_reserve(1000.0)
        hip, dev = _hip_runtime(), {}
        for k, v in host.items():
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), v.nbytes) == 0 and hip.hipMemcpy(p, v.ctypes.data, v.nbytes, 1) == 0
            dev[k] = p.value
        for combo in range(16):                                          # every pair of sides occurs
            ptr = {k: (dev[k] if combo >> b & 1 else host[k].ctypes.data) for b, k in enumerate(host)}
            for fx, lv in ((True, True), (False, False)):
                table.reset()
                table.update_device(ptr["frames"], n, BASE, levels_ptr=ptr["levels"] if lv else None,
                                    mlat_ptr=ptr["fixes"] if fx else None, modes_ptr=ptr["recs"])
                now = (table.modes().tobytes(), table.aircraft()[0].tobytes(), table.points().tobytes())
                first = now if first is None else first
                assert now == first, (combo, fx, lv)
        # recs straight from modes_device(): the ctx's scratch, ordered on the same stream
        d.modes_of_async(host["frames"], known=mixed.known)
        table.reset()
        table.update_device(dev["frames"], n, BASE, modes_ptr=d.modes_device()[0])
        assert d.fetch_modes()[0].tobytes() == host["recs"].tobytes()
        assert (table.modes().tobytes(), table.aircraft()[0].tobytes(), table.points().tobytes()) == first
        model = M.Table()
        model.update(host["frames"], host["recs"], BASE)
        M.same_records(table.modes(), model.records())
        table.reset()                                                    # waits: nothing reads the lists any more
        assert len(table.modes()) == 0
        for p in dev.values():
            assert hip.hipFree(p) == 0


# ---- (e) a full table, expire, reset, held from before the reserve --------------------------------------------------------
def test_full_table_expire_reset_and_held_from_before_the_reserve(gpu, mixed):
    tr = mixed.cut(0, 3000)
    with _table(max_aircraft=16) as table:
        model = M.Table(max_aircraft=16)
        _run(table, model, tr.cut(0, 1500), "first")
        pts = table.points()["flags"]
        assert (pts & A.ADSB_TRACK_UNTRACKED).any() and (pts & A.ADSB_TRACK_UNADDRESSED).any()
        assert model.flags == M.TABLE_FULL and len(model.state) == 16
        turned = tr.recs[:1500][(pts & A.ADSB_TRACK_UNTRACKED) != 0]
        assert (turned["kind"] <= 1).all() and (turned["kind"] == MM.KNOWN).any()
        # expire: the survivors' records move with them, byte for byte; re-admission starts from the empty record
        late = Traffic(tr.frames[1500:1600], recs=tr.recs[1500:1600], base=BASE + 40_000_000)     # 20 s later
        _run(table, model, late, "late")
        recs = table.aircraft()[0]
        heard = dict(zip(recs["icao"].tolist(), table.last_heard().tolist()))
        cut = float(BASE + 20_000_000) * SPS
        assert 0 < sum(t < cut for t in heard.values()) < 16
        table.expire(cut)
        model.expire(heard, cut)
        assert table.aircraft()[0]["icao"].tolist() == sorted(model.state)
        M.same_records(table.modes(), model.records(), "after expire")
        again = Traffic(tr.frames[1600:3000], recs=tr.recs[1600:3000], base=BASE + 40_000_000)
        _run(table, model, again, "re-admission")
        # reset: every place empty, also the places no aircraft holds
        table.reset()
        assert len(table.modes()) == 0
        raw = np.zeros(16, dtype=A.AIRCRAFT_MODES_DTYPE)
        hip = _hip_runtime()
        assert hip.hipMemcpy(raw.ctypes.data, table.modes_device(), raw.nbytes, 2) == 0     # device to host
        assert raw.tobytes() == EMPTY * 16
        _run(table, M.Table(max_aircraft=16), tr.cut(0, 1500), "after reset")
    # held from before the reserve: empty until the next counted frame
    sq = np.flatnonzero((tr.recs["kind"] == MM.SELF) & np.isin(tr.recs["df"], (17, 18)))[:200]
    with _table(reserve=False) as table:
        table.update(tr.frames[sq], tr.base)
        held = table.aircraft()[0]["icao"].tolist()
        table.modes_reserve()
        got = table.modes()
        assert len(got) == len(held) > 3 and got.tobytes() == EMPTY * len(held)
        model = M.Table()
        for a in held:
            model.state[a] = M.empty()
        _run(table, model, tr.cut(1000, 1400), "held from before the reserve")


# ---- (f) the reserve changes nothing else --------------------------------------------------------------------------------
def test_plain_updates_of_a_table_with_the_reserve_and_update_modes_without_it(gpu, mixed):
    sq = np.flatnonzero((mixed.recs["kind"] == MM.SELF) & np.isin(mixed.recs["df"], (17, 18)))[:900]
    frames, recs = mixed.frames[sq], mixed.recs[sq]
    n = len(frames)
    levels, fixes = _levels(n, 12), _fixes(n, 13)
    kw = dict(seconds_per_sample=SPS, max_frames=1 << 12, max_aircraft=12)
    with A.AdsbDemod(max_samples=1024, max_out=16) as d, A.TrackTable(d, **kw) as table, A.TrackTable(d, **kw) as bare:
        for t in (table, bare):
            t.summaries_reserve()
            t.levels_reserve()
            t.fixes_reserve((47.0, 8.0, 180.0))
            t.mlat_reserve(1000.0)
        table.modes_reserve()
        for lo, hi, kwargs in ((0, 300, {}), (300, 600, dict(levels=levels[300:600])),
                               (600, n, dict(levels=levels[600:n], mlat=fixes[600:n]))):
            table.update(frames[lo:hi], BASE, **kwargs)
            bare.update(frames[lo:hi], BASE, **kwargs)
            for name in ("points", "summaries", "frame_fixes", "levels", "fixes", "mlat", "last_heard", "velocity"):
                assert getattr(table, name)().tobytes() == getattr(bare, name)().tobytes(), (name, lo)
            assert table.aircraft()[0].tobytes() == bare.aircraft()[0].tobytes()
            got = table.modes()
            assert got.tobytes() == EMPTY * len(got) and len(got) == len(table.aircraft()[0])
        # without the reserve: every modes entry point says so
        L = _lib.load()
        for call in (lambda: bare.modes(), lambda: bare.modes_device(), lambda: bare.update(frames[:10], BASE, modes=recs[:10]),
                     lambda: bare.update(frames[:0], BASE, modes=recs[:0])):
            with pytest.raises(A.AdsbError) as e:
                call()
            assert e.value.code == A.ADSB_E_STATE
    with _table(max_frames=64) as table:
        with pytest.raises(A.AdsbError) as e:
            table.update(frames[:10], BASE, modes=recs[:10], mlat=fixes[:10])      # fixes without an mlat reserve
        assert e.value.code == A.ADSB_E_STATE
        with pytest.raises(A.AdsbError) as e:
            table.update(frames[:10], BASE, modes=recs[:10], levels=levels[:10])   # levels without a levels reserve
        assert e.value.code == A.ADSB_E_STATE
        assert L.adsb_track_table_update_modes(table._h, frames.ctypes.data, recs.ctypes.data, None, None, 65, 0) == A.ADSB_E_CAPACITY
        table.update(frames[:0], BASE, modes=recs[:0])                   # n = 0 is fine, and an empty list
        assert len(table.points()) == 0 and len(table.modes()) == 0


# ---- (g) wire input -> correlate -> modes_of -> multilaterate -> update_modes, all on the device ---------------------------
def test_network_end_to_end_on_the_device(gpu, oracle):
    from tests import mlat_model as ML
    net = N.network(oracle)
    who = net["who"]
    assert {int(MM.first_pass(f.ljust(14, b"\0"))["df"]) for f, w in zip(net["frames"], who) if w == "s"} == {4, 5, 11, 20}
    with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d, \
            A.TrackTable(d, max_aircraft=64, max_frames=256, seconds_per_sample=SPS) as table:
        table.mlat_reserve(1000.0)
        table.modes_reserve()
        win = d.wire_in_of(b"".join(net["streams"]), net["ends"], filter="short")
        frames_dev, rx_dev = d.wire_in_device()[:2]
        d.correlate_of_async((frames_dev, len(win.frames)), win.counts, 5000)
        n_msgs = len(d.fetch_correlated()[0])
        assert n_msgs == 24
        d.modes_of_async((d.correlated_device()[1], n_msgs))
        # (no altitude equation for these formats: see tests/test_gpu_modes_chain.py)
        fixes, _ = d.multilaterate(net["rcv"], rx=rx_dev, time_source="ticks", max_iterations=200)
        table.update_device(d.correlated_device()[1], n_msgs, 0, mlat_ptr=d.mlat_device()[0], modes_ptr=d.modes_device()[0])
        recs, flags = table.aircraft()
        assert recs["icao"].tolist() == [N.MODE_S, N.ADSB] and flags == 0                            # the noise admits nothing
        pts = table.points()
        garbage = np.array([w == "g" for w in who])
        assert (pts["flags"][garbage] == A.ADSB_TRACK_UNADDRESSED).all() and not (pts["flags"][~garbage] & 6).any()
        silent, adsb = table.modes()
        mode_s = np.array([w == "s" for w in who])
        assert int(recs["n_frames"][0]) == mode_s.sum() == silent["n_replies"] and not silent["flags"] & M.SQUITTER
        assert silent["n_allcall"] == 1 and silent["flags"] & M.ALT and silent["flags"] & M.SQUAWK and silent["flags"] & M.CALLSIGN
        assert silent["squawk"] == 4210 and silent["callsign"] == b"SILENT1_" and recs["has_position"][0] == 0
        assert adsb["flags"] == M.SQUITTER and adsb["n_replies"] == 0
        # against the model, on the lists fetched
        frames_out, mrec = d.fetch_correlated()[1], d.fetch_modes()[0]
        model = M.Table(max_aircraft=64)
        model.update(frames_out, mrec, 0)
        M.same_records(table.modes(), model.records(), "end to end")
        last = np.flatnonzero(mode_s & (mrec["flags"] & MM.ALT != 0))[-1]
        assert silent["altitude_ft"] == mrec["altitude_ft"][last]
        # the kept fix of the Mode S aircraft is its newest valid one, near where that reply was sent from
        kept = table.mlat()[0]
        newest = np.flatnonzero(mode_s & (fixes["flags"] & ML.VALID != 0))[-1]
        assert kept["flags"] & A.ADSB_TRACK_MLAT_VALID and kept["n_valid"] == mode_s.sum()
        assert kept["latitude"] == fixes["latitude"][newest] and kept["longitude"] == fixes["longitude"][newest]
        err = float(np.sqrt(((ML.ecef_of(kept["latitude"], kept["longitude"], float(kept["height_m"])) - net["pos"][newest]) ** 2).sum()))
        print(f"Mode S aircraft: kept fix {err:.0f} m from its emitter, pdop {float(kept['pdop']):.2f}")
        assert err < 150.0 * 3 * float(fixes["pdop"][mode_s].max())          # tests/test_gpu_modes_chain.py's bound


# ---- (h) the tool ---------------------------------------------------------------------------------------------------------
def test_the_tool_prints_the_same_table_on_the_device_and_through_the_mirrors(gpu, oracle, tmp_path):
    import os
    import subprocess
    import sys
    args = N.recordings(N.network(oracle), tmp_path)
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "mlat.py")
    runs = [subprocess.run([sys.executable, tool] + extra + ["--modes", "--aircraft", "--max-iterations", "200"] + args,
                           capture_output=True, text=True, timeout=120) for extra in ([], ["--host"])]
    assert runs[0].returncode == 0 == runs[1].returncode, (runs[0].stderr, runs[1].stderr)
    assert runs[0].stdout == runs[1].stdout
    N.check_table(runs[0].stdout)
    # --modes alone: one line per fix of a message with an aircraft's address, solved where the messages lie
    runs = [subprocess.run([sys.executable, tool] + extra + ["--modes", "--max-iterations", "200"] + args,
                           capture_output=True, text=True, timeout=120) for extra in ([], ["--host"])]
    assert runs[0].returncode == 0 == runs[1].returncode, (runs[0].stderr, runs[1].stderr)
    assert runs[0].stdout == runs[1].stdout and len(runs[0].stdout.splitlines()) == 22


def test_replay_prints_the_table_of_one_recording(gpu, oracle, tmp_path):
    """tools/replay.py --beast-in --modes --aircraft on one receiver's recording: the table through update(modes=)"""
    import os
    import subprocess
    import sys
    args = N.recordings(N.network(oracle), tmp_path)
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "replay.py")
    out = subprocess.run([sys.executable, tool, args[1], "--beast-in", "--modes", "--aircraft"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [line.split("\t") for line in out.stdout.splitlines()]
    assert rows[0] == ["ICAO", "Callsign", "Altitude", "Latitude", "Longitude", "Velocity", "Age", "Alt(S)", "Squawk", "Call(S)",
                       "Replies", "S"]
    by_icao = {int(row[0], 16): row for row in rows[1:]}
    assert set(by_icao) == {N.MODE_S, N.ADSB}                           # the garbage this receiver heard admits nothing
    silent, adsb = by_icao[N.MODE_S], by_icao[N.ADSB]
    assert silent[8:] == ["4210", "SILENT1", "15", "S"] and silent[7] != "n/a" and silent[3] == silent[4] == "n/a"
    assert adsb[7:] == ["n/a", "n/a", "n/a", "0", ""]
