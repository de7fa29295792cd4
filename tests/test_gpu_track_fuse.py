"""The fused view of a track bank on the device (adsb_track_bank_fuse_*, TrackBank.fuse): one record per distinct ICAO
over all receivers, ascending ICAO.  Every fused field is a copy of one receiver's record or an integer sum, so every
comparison here is byte for byte (tobytes() of the structured arrays, NaNs included) against tests/fuse_model.py fed the
bank's own fetches (aircraft(), last_heard(), velocity()); the model is pinned by hand in test_track_fuse_args.py."""
import ctypes as C
import math

import numpy as np
import pytest

import air_rs_amd as A
from tests import fuse_model
from tests.traffic import ident_frame, position_frame
from tests.velocity_traffic import velocity_frame, velocity_traffic

RECEIVER_FIELDS = ("heard_receiver", "contact_receiver", "position_receiver", "callsign_receiver", "velocity_receiver")
SPS = 1e-3


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


def _icao(b):
    return (int(b[1]) << 16) | (int(b[2]) << 8) | int(b[3])


def _reicao(oracle, frame, icao):
    data = bytes([frame[0], (icao >> 16) & 0xFF, (icao >> 8) & 0xFF, icao & 0xFF]) + bytes(frame[4:11])
    crc = oracle.get_adsb_crc(data)
    return data + bytes([(crc >> 16) & 0xFF, (crc >> 8) & 0xFF, crc & 0xFF])


def _even_odd(oracle, icao, odd):
    # the CPR halves of the reference pair (aircraft.rs:201-212), under another ICAO: every such pair decodes
    return position_frame(oracle, icao, odd, 74158 if odd else 93000, 50194 if odd else 51372)


def _fleet(oracle, n_receivers, seed, n_aircraft=45, n_frames=4000, span_s=60.0):
    """Positions, identifications and TC 19 frames of one fleet (velocity_traffic), heard by n_receivers receivers with
    overlapping coverage: a third of the aircraft on every receiver, a third on two or three, a third on one; a
    receiver misses 40 % of what it could hear, so who heard an aircraft last differs from aircraft to aircraft.  The
    fleet's lowest and highest ICAO become 000000 and FFFFFF, the highest one heard by the last receiver too.
    Returns (per-receiver FRAME_DTYPE lists with offsets in samples, per-receiver sample_base): receiver r's clock is
    ahead by base[r] samples, so times of different receivers differ also for the same message."""
    R = n_receivers
    rng = np.random.default_rng(1000 + seed)
    traffic = velocity_traffic(oracle, seed=seed, n_aircraft=n_aircraft, n_frames=n_frames, span_s=span_s)
    icaos = sorted({_icao(fr) for _, fr in traffic})
    remap = {icaos[0]: 0x000000, icaos[-1]: 0xFFFFFF}
    hears = {}
    for k, icao in enumerate(icaos):
        kind = k % 3
        if kind == 0 or R == 1:
            who = set(range(R))
        elif kind == 1:
            who = {int(x) for x in rng.choice(R, size=min(R, int(rng.integers(2, 4))), replace=False)}
        else:
            who = {int(rng.integers(0, R))}
        hears[icao] = who
    hears[icaos[-1]] = hears[icaos[-1]] | {R - 1}
    base = [int(x) for x in rng.integers(0, 2000, size=R)]
    lists = [[] for _ in range(R)]
    for t, fr in traffic:
        icao = _icao(fr)
        out = _reicao(oracle, fr, remap[icao]) if icao in remap else fr
        for r in hears[icao]:
            if rng.random() < 0.6:
                lists[r].append((round(t / SPS), out))
    return [_frames(x) for x in lists], base


def _model(bank, since=-math.inf):
    recs, _ = bank.aircraft()
    return fuse_model.fuse(recs, bank.last_heard(), bank.velocity(), since)


def _bank(d, n_receivers, lists=None, base=None, **kw):
    kw.setdefault("max_frames", 1 << 17)
    bank = A.TrackBank(d, n_receivers, seconds_per_sample=SPS, **kw)
    if lists is not None:
        bank.update(_concat(lists), [len(x) for x in lists], base)
    return bank


def _same(got, want):
    assert got.dtype == want.dtype == A.FUSED_DTYPE
    assert len(got) == len(want), (len(got), len(want))
    if got.tobytes() != want.tobytes():                      # say where, then fail
        for k in range(len(got)):
            assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])
    assert list(got["icao"]) == sorted(set(int(x) for x in got["icao"]))


def _state(bank):
    recs, flags = bank.aircraft()
    return (b"".join(x.tobytes() for x in recs), tuple(flags), b"".join(x.tobytes() for x in bank.last_heard()),
            b"".join(x.tobytes() for x in bank.velocity()), bank.points().tobytes())


def _hip_runtime():
    """The HIP runtime this process already holds (the one libadsb_hip.so is bound to), for a plain hipMemcpy."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path:
            return C.CDLL(path)
    raise RuntimeError("no HIP runtime mapped")


def _read_device(ptr, nbytes):
    buf = C.create_string_buffer(nbytes)
    hip = _hip_runtime()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(buf, ptr, nbytes, 2) == 0           # hipMemcpyDeviceToHost
    return buf.raw


@pytest.mark.gpu
@pytest.mark.parametrize("n_receivers,seed", [(1, 1), (3, 2), (8, 3), (64, 4)])
def test_fused_equals_model(gpu, oracle, n_receivers, seed):
    """Random multi-receiver traffic with overlapping coverage: the fused view equals the model, for every record and
    for a `since` in the middle; fuse(since=t) equals fuse(-inf) of a second bank after expire(t)."""
    R = n_receivers
    lists, base = _fleet(oracle, R, seed, n_aircraft=45 if R < 64 else 150, n_frames=4000 if R < 64 else 5000)
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, _bank(d, R, lists, base) as bank, \
            _bank(d, R, lists, base) as twin:
        want = _model(bank)
        got, total, flags = bank.fuse()
        _same(got, want)
        assert total == len(want) and flags == 0
        assert int(got["n_receivers"].max()) == R and int(got["n_receivers"].min()) == 1
        assert {0x000000, 0xFFFFFF} <= {int(x) for x in got["icao"]}
        assert int(got[got["icao"] == 0xFFFFFF]["n_receivers"][0]) >= 1
        assert (got["has_position"] != 0).sum() > 10 and (got["velocity"]["subtype"] != 0).sum() > 10
        assert (got["callsign"] != b"").sum() > 10
        if R >= 3:
            for name in RECEIVER_FIELDS:                     # not "receiver 0 always wins"
                seen = {int(x) for x in got[name]} - {A.ADSB_FUSED_NONE}
                assert len(seen) >= 3, (name, seen)
        # since: -inf is everything, +inf nothing, a cut in the middle equals the model and an expired twin
        again, total, flags = bank.fuse(since=-math.inf)
        assert again.tobytes() == got.tobytes()
        none, total, flags = bank.fuse(since=math.inf)
        assert len(none) == 0 and total == 0 and flags == 0
        heard = np.sort(np.concatenate(bank.last_heard()))
        for cut in (float(heard[len(heard) // 2]), float(heard[len(heard) // 4]) + 1e-9, float(heard[-1])):
            want = _model(bank, cut)
            got, total, flags = bank.fuse(since=cut)
            _same(got, want)
            assert total == len(want) > 0 and flags == 0
        cut = float(heard[len(heard) // 2])                  # a record with last_heard == cut stays in both
        got, _, _ = bank.fuse(since=cut)
        twin.expire([cut] * R)
        expired, total, flags = twin.fuse()
        assert expired.tobytes() == got.tobytes() and total == len(got) and flags == 0
        _same(expired, _model(twin))


@pytest.mark.gpu
def test_any_cut_gives_the_same_fused_bytes(gpu, oracle):
    R = 5
    lists, base = _fleet(oracle, R, 11, n_frames=3000)
    rng = np.random.default_rng(5)
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, _bank(d, R, lists, base) as whole, _bank(d, R) as cutup:
        want, total, _ = whole.fuse()
        cursor, n_upd = [0] * R, 0
        while any(cursor[r] < len(lists[r]) for r in range(R)):
            take = [min(int(rng.integers(0, 300)), len(lists[r]) - cursor[r]) for r in range(R)]
            parts, bases = [], []
            for r in range(R):
                part = lists[r][cursor[r]:cursor[r] + take[r]].copy()
                first = int(part["offset"][0]) if take[r] else 0
                part["offset"] -= first                      # offsets relative to the part's first frame
                parts.append(part)
                bases.append(base[r] + first)
                cursor[r] += take[r]
            cutup.update(_concat(parts), take, bases)
            n_upd += 1
        assert n_upd > 5
        got, gtotal, _ = cutup.fuse()
        assert got.tobytes() == want.tobytes() and gtotal == total
        _same(got, _model(cutup))


@pytest.mark.gpu
def test_exact_ties_go_to_receiver_0(gpu, oracle):
    """The same frames with the same sample_base on every receiver: every time ties, receiver 0 wins everything."""
    R = 8
    lists, _ = _fleet(oracle, 1, 21, n_frames=1500)
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, _bank(d, R, [lists[0]] * R, 77) as bank, \
            _bank(d, 1, lists, 77) as one:
        got, total, flags = bank.fuse()
        single, _, _ = one.fuse()
        _same(got, _model(bank))
        assert len(got) == len(single) == total > 30
        for name in RECEIVER_FIELDS:
            assert set(int(x) for x in got[name]) <= {0, A.ADSB_FUSED_NONE}, name
            assert (got[name] == single[name]).all(), name
        assert (got["n_receivers"] == R).all() and (got["n_frames"] == R * single["n_frames"]).all()
        for name in ("latitude", "longitude", "position_time", "last_contact", "last_heard", "altitude", "callsign",
                     "velocity", "has_position", "icao"):
            assert got[name].tobytes() == single[name].tobytes(), name


@pytest.mark.gpu
def test_fuse_only_reads_the_bank(gpu, oracle):
    R = 4
    lists, base = _fleet(oracle, R, 31, n_frames=2400)
    thirds = [[x[k * len(x) // 3:(k + 1) * len(x) // 3] for x in lists] for k in range(3)]
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, _bank(d, R) as fused, _bank(d, R) as plain:
        for part in thirds:
            for bank in (fused, plain):
                bank.update(_concat(part), [len(x) for x in part], base)
            before = _state(fused)
            got, _, _ = fused.fuse()                         # between every two updates
            fused.fuse(since=float(np.median(got["last_heard"])))
            assert _state(fused) == before
            assert _state(fused) == _state(plain)
        _same(fused.fuse()[0], _model(plain))


@pytest.mark.gpu
def test_after_expire_and_after_reset(gpu, oracle):
    R = 6
    lists, base = _fleet(oracle, R, 41, n_frames=3000)
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, _bank(d, R, lists, base) as bank:
        n_before = sum(len(x) for x in bank.aircraft()[0])
        heard = np.sort(np.concatenate(bank.last_heard()))
        cuts = [float(heard[len(heard) // 3]) if r % 2 else -math.inf for r in range(R)]   # survivors move in place
        bank.expire(cuts)
        n_after = sum(len(x) for x in bank.aircraft()[0])
        assert 0 < n_after < n_before
        got, total, flags = bank.fuse()
        _same(got, _model(bank))
        assert total == len(got) and flags == 0
        bank.update(_concat(lists), [len(x) for x in lists], [b + 100_000 for b in base])  # heard again, re-admitted
        _same(bank.fuse()[0], _model(bank))
        bank.reset()
        got, total, flags = bank.fuse()
        assert len(got) == 0 and total == 0 and flags == 0
        bank.update(_concat(lists[:1] + [x[:0] for x in lists[1:]]), [len(lists[0])] + [0] * (R - 1), base)
        got, total, flags = bank.fuse()
        _same(got, _model(bank))
        assert total > 0 and (got["n_receivers"] == 1).all() and (got["heard_receiver"] == 0).all()


@pytest.mark.gpu
def test_truncation_keeps_the_lowest_icaos(gpu, oracle):
    R = 3
    lists, base = _fleet(oracle, R, 51, n_frames=2000)
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, _bank(d, R, lists, base) as bank:
        want = _model(bank)
        assert len(want) > 20
        got, total, flags = bank.fuse(max_fused=7)
        assert len(got) == 7 and total == len(want) and flags == A.ADSB_TRACK_FUSED_TRUNCATED
        assert got.tobytes() == want[:7].tobytes()
        got, total, flags = bank.fuse()                      # max_fused stays as reserved
        assert len(got) == 7 and flags == A.ADSB_TRACK_FUSED_TRUNCATED
        got, total, flags = bank.fuse(max_fused=len(want))   # exactly enough is not truncated
        assert flags == 0 and total == len(want)
        _same(got, want)
        got, total, flags = bank.fuse(max_fused=len(want) - 1)
        assert flags == A.ADSB_TRACK_FUSED_TRUNCATED and got.tobytes() == want[:-1].tobytes()
        got, total, flags = bank.fuse(max_fused=0)           # the worst case: everything
        assert flags == 0
        _same(got, want)


@pytest.mark.gpu
def test_a_full_receiver(gpu, oracle):
    """max_aircraft = 16: receiver 1 is offered 24 ICAOs and holds its lowest 16 (FULL), so it lacks aircraft the others
    hold; receiver 0 holds exactly 16 without turning any away."""
    rng = np.random.default_rng(61)
    icaos = sorted(int(x) for x in rng.choice(np.arange(1, 1 << 24), size=24, replace=False))
    per = [icaos[:16], icaos, icaos[10:20]]
    lists = []
    for r, mine in enumerate(per):
        items = []
        for k, icao in enumerate(mine):
            items += [(40 * k + r, _even_odd(oracle, icao, False)), (40 * k + 10 + r, _even_odd(oracle, icao, True)),
                      (40 * k + 20 + r, ident_frame(oracle, icao, [r + 1] * 8))]
        lists.append(_frames(items))
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            _bank(d, 3, lists, [0, 5000, 200], max_aircraft=16, max_frames=256) as bank:
        recs, flags = bank.aircraft()
        assert [len(x) for x in recs] == [16, 16, 10] and flags == [0, A.ADSB_TRACK_TABLE_FULL, 0]
        got, total, flags = bank.fuse()
        _same(got, _model(bank))
        assert [int(x) for x in got["icao"]] == icaos[:20] and total == 20 and flags == 0
        assert [int(x) for x in got["n_receivers"]] == [2] * 10 + [3] * 6 + [1] * 4
        assert (got["heard_receiver"][:16] == 1).all() and (got["heard_receiver"][16:] == 2).all()
        assert (got["has_position"] == 1).all()


@pytest.mark.gpu
def test_argument_and_state_errors(gpu, oracle):
    from air_rs_amd import _lib
    L = _lib.load()
    lists, base = _fleet(oracle, 2, 71, n_frames=300)
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, _bank(d, 2, lists, base) as bank:
        h = bank._h
        n, total, flags = C.c_size_t(), C.c_size_t(), C.c_uint32()
        out = (_lib.AdsbFusedAircraft * 4)()
        rec, counts = C.c_void_p(), C.c_void_p()
        assert L.adsb_track_bank_fuse(h, -math.inf) == A.ADSB_E_STATE                    # no reserve yet
        assert L.adsb_track_bank_fetch_fused(h, out, 4, C.byref(n), C.byref(total), C.byref(flags)) == A.ADSB_E_STATE
        assert L.adsb_track_bank_fused_device(h, C.byref(rec), C.byref(counts)) == A.ADSB_E_STATE
        assert L.adsb_track_bank_fuse(h, math.nan) == A.ADSB_E_ARG
        assert L.adsb_track_bank_fuse_reserve(h, 1000) == A.ADSB_OK
        assert L.adsb_track_bank_fetch_fused(h, out, 4, C.byref(n), C.byref(total), C.byref(flags)) == A.ADSB_E_STATE
        assert L.adsb_track_bank_fused_device(h, C.byref(rec), C.byref(counts)) == A.ADSB_E_STATE
        assert L.adsb_track_bank_fuse(h, math.nan) == A.ADSB_E_ARG
        assert L.adsb_track_bank_fuse(h, -math.inf) == A.ADSB_OK
        assert L.adsb_track_bank_fetch_fused(h, None, 4, C.byref(n), C.byref(total), C.byref(flags)) == A.ADSB_E_ARG
        assert L.adsb_track_bank_fetch_fused(h, out, 4, C.byref(n), C.byref(total), C.byref(flags)) == A.ADSB_OK
        want = _model(bank)
        assert n.value == 4 and total.value == len(want) > 4 and flags.value == 0
        assert bytes(out) == want[:4].tobytes()
        assert L.adsb_track_bank_fetch_fused(h, None, 0, None, None, None) == A.ADSB_OK
        assert L.adsb_track_bank_fuse_reserve(h, 1000) == A.ADSB_OK                      # a new reserve: no fuse yet
        assert L.adsb_track_bank_fused_device(h, C.byref(rec), C.byref(counts)) == A.ADSB_E_STATE


@pytest.mark.gpu
def test_two_fuses_are_identical_and_device_counts(gpu, oracle):
    R = 8
    lists, base = _fleet(oracle, R, 81, n_frames=3000)
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, _bank(d, R, lists, base) as bank:
        a, total, flags = bank.fuse(max_fused=4096)
        b, total_b, flags_b = bank.fuse()
        assert a.tobytes() == b.tobytes() and (total, flags) == (total_b, flags_b) and total == len(a)
        rec_ptr, counts_ptr = bank.fused_device()
        counts = np.frombuffer(_read_device(counts_ptr, 16), dtype=np.uint64)
        assert [int(x) for x in counts] == [len(a), total]
        raw = _read_device(rec_ptr, 128 * len(a))
        assert raw == a.tobytes()
        c, total_c, flags_c = bank.fuse(max_fused=5)
        counts = np.frombuffer(_read_device(bank.fused_device()[1], 16), dtype=np.uint64)
        assert [int(x) for x in counts] == [5, total] and flags_c == A.ADSB_TRACK_FUSED_TRUNCATED
        assert c.tobytes() == a[:5].tobytes()


@pytest.mark.gpu
def test_update_launch_then_fuse(gpu, oracle):
    """Modulated traffic in a 4-channel device buffer, the same fleet on every channel with different gaps, applied by
    update_launch over several launches: the fused view equals the model on that bank's fetches."""
    import torch

    from tests.golden.make_golden import modulate, place
    C_, n, stride, R, max_out = 4, 20_000, 20_480, 5, 256
    sps = 1.0 / n
    fleet = [fr for _, fr in velocity_traffic(oracle, seed=91, n_aircraft=25, n_frames=1200)]
    with A.AdsbDemod(max_samples=n, max_out=max_out, max_channels=C_, host_staging=False) as d, \
            A.TrackBank(d, R, max_frames=max_out, seconds_per_sample=sps) as bank:
        k = [0, 300, 600, 900]                               # every channel walks the fleet's list from its own start
        for launch in range(8):
            host = np.full((C_, stride, 2), 77, dtype=np.int8)
            for c in range(C_):
                gap = 500 + 60 * c
                items = []
                for j in range((n - 600) // gap):
                    items.append((300 + gap * j, modulate(fleet[k[c] % len(fleet)], (80, 30), None)))
                    k[c] += 1
                host[c, :n] = place(n, items, np.int8, floor=3, seed=2000 * launch + c)
            buf = torch.from_numpy(host).cuda()
            d.demod_device_async(buf.data_ptr(), n, C_, stride)
            bank.update_launch([launch * n + 11 * r for r in range(R)])
            got, total, flags = bank.fuse()
            torch.cuda.synchronize()
        want = _model(bank)
        _same(got, want)
        assert total == len(want) > 15 and flags == 0
        assert int(got["n_receivers"].max()) == C_ and len({int(x) for x in got["heard_receiver"]}) >= 3
        assert (got["has_position"] != 0).sum() > 3 and (got["velocity"]["subtype"] != 0).sum() > 3


@pytest.mark.gpu
def test_many_workgroups(gpu, oracle):
    """64 receivers, more than 20 000 records: 700 ICAOs (000000 and FFFFFF among them), each receiver holds a random
    330 or so of them in an order of its own, with an identification, sometimes a velocity and sometimes a position pair."""
    R = 64
    rng = np.random.default_rng(101)
    pool = sorted({0x000000, 0xFFFFFF} | {int(x) for x in rng.choice(np.arange(1, 0xFFFFFF), size=698, replace=False)})
    lists, n_records = [], 0
    for r in range(R):
        mine = [icao for icao in pool if rng.random() < 0.47 or (icao == 0xFFFFFF and r == R - 1)]
        n_records += len(mine)
        rng.shuffle(mine)                                    # who heard an aircraft last: a different receiver each
        items, t = [], 0
        for icao in mine:
            items.append((t, ident_frame(oracle, icao, list(rng.integers(1, 27, size=8)))))
            if rng.random() < 0.4:
                items.append((t + 1, velocity_frame(oracle, icao, 1, dew=int(rng.integers(0, 2)),
                                                    vew=int(rng.integers(1, 1024)), dns=0,
                                                    vns=int(rng.integers(1, 1024)), vr=int(rng.integers(0, 512)))))
            if rng.random() < 0.2:
                items += [(t + 2, _even_odd(oracle, icao, False)), (t + 3, _even_odd(oracle, icao, True))]
            t += int(rng.integers(4, 9))
        lists.append(_frames(items))
    base = [int(x) for x in rng.integers(0, 300, size=R)]
    assert n_records >= 20_000
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            _bank(d, R, lists, base, max_aircraft=1024, max_frames=1 << 17) as bank:
        assert sum(len(x) for x in bank.aircraft()[0]) == n_records
        want = _model(bank)
        got, total, flags = bank.fuse(max_fused=1024)
        _same(got, want)
        assert total == len(pool) and flags == 0
        assert int(got["n_receivers"].max()) > 32 and int(got["n_frames"].sum()) == sum(len(x) for x in lists)
        for name in RECEIVER_FIELDS:
            assert len({int(x) for x in got[name]} - {A.ADSB_FUSED_NONE}) >= 32, name
        heard = np.sort(np.concatenate(bank.last_heard()))
        cut = float(heard[len(heard) // 2])
        _same(bank.fuse(since=cut)[0], _model(bank, cut))
        wide, total, flags = bank.fuse(max_fused=0)          # a reduce grid sized for 64 x 1024 places
        assert wide.tobytes() == got.tobytes() and total == len(pool) and flags == 0


@pytest.mark.gpu
def test_more_than_128_receivers(gpu, oracle):
    """256 receivers (the sort key no longer fits 32 bits next to the 'no record' bit), FFFFFF on receiver 255."""
    R = 256
    rng = np.random.default_rng(111)
    pool = sorted({0x000000, 0xFFFFFF} | {int(x) for x in rng.choice(np.arange(1, 0xFFFFFF), size=30, replace=False)})
    lists = []
    for r in range(R):
        mine = [icao for icao in pool if rng.random() < 0.3 or (icao == 0xFFFFFF and r in (0, R - 1))]
        lists.append(_frames([(3 * k, ident_frame(oracle, icao, [1 + (r + k) % 26] * 8)) for k, icao in enumerate(mine)]))
    base = [int(x) for x in rng.integers(0, 500, size=R)]
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, _bank(d, R, lists, base, max_aircraft=16) as bank:
        got, total, flags = bank.fuse()
        _same(got, _model(bank))
        assert total == len(pool) and flags == 0 and int(got["heard_receiver"].max()) > 128
        last = got[got["icao"] == 0xFFFFFF][0]
        assert last["n_receivers"] >= 2
