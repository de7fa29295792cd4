"""Airborne velocity (DF17 TC 19) in the device track table and bank (adsb_track_*_fetch_velocity, TrackTable /
TrackBank.velocity): every record keeps the decode of its aircraft's last velocity message of subtype 1-4, checked
field by field against the NumPy model in tests/velocity_traffic.py (integers and speed exact, direction within
1e-4 degrees), while every other record field still equals the oracle's, which treats TC 19 as `Uknown`."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import air_rs_amd as A
from tests.traffic import position_frame
from tests.velocity_traffic import (DIRECTION, SPEED, VRATE, decode, empty, last_velocity, random_velocity_frame,
                                    velocity_frame, velocity_traffic)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN_ST1, KNOWN_ST3 = "8D485020994409940838175B284F", "8DA05F219B06B6AF189400CBC33F"
SHARED = [0x3ABCDE, 0xA00011, 0xC0FFEE]  # outside random_traffic's range: active on several receivers


def _frames(items):
    """[(offset, 14 frame bytes)] -> FRAME_DTYPE array."""
    out = np.zeros(len(items), dtype=A.FRAME_DTYPE)
    for k, (off, b) in enumerate(items):
        out[k]["offset"] = off
        out[k]["bytes"] = np.frombuffer(bytes(b), dtype=np.uint8)
        out[k]["fixed_bit"] = 0xFF
    return out


def _icao(b):
    return (int(b[1]) << 16) | (int(b[2]) << 8) | int(b[3])


def _timed(frames, base, sps):
    """FRAME_DTYPE array -> [(time_s, bytes)] with the table's frame time"""
    return [(float(base + int(f["offset"])) * sps, bytes(f["bytes"])) for f in frames]


def _same_velocity(got, recs, want):
    """got: VELOCITY_DTYPE aligned with recs; want: {icao: model velocity}, absent = none yet"""
    assert len(got) == len(recs)
    for v, rec in zip(got, recs):
        w = want.get(int(rec["icao"]), empty())
        for name in ("subtype", "flags", "vertical_rate_fpm", "v_ew_kt", "v_ns_kt", "vrate_baro", "airspeed_tas",
                     "reserved", "speed_kt"):
            assert v[name] == w[name], (hex(int(rec["icao"])), name, v, w)
        assert (math.isnan(v["time"]) and math.isnan(w["time"])) or v["time"] == w["time"], (v, w)
        assert abs(float(v["direction_deg"]) - float(w["direction_deg"])) <= 1e-4, (v, w)
        assert 0.0 <= float(v["direction_deg"]) < 360.0


def _same_table(recs, want, counts):
    assert [int(r["icao"]) for r in recs] == [s.icao for s in want]
    for rec, s in zip(recs, want):
        assert rec["n_frames"] == counts[s.icao]
        assert rec["callsign"].decode() == s.callsign.decode() and rec["altitude"] == s.altitude
        assert bool(rec["has_position"]) == bool(s.has_position)
        if s.has_position:
            assert (rec["latitude"], rec["longitude"]) == pytest.approx((s.latitude, s.longitude), abs=1e-9)
        assert (math.isnan(rec["last_contact"]) and math.isnan(s.last_contact)) or \
            rec["last_contact"] == pytest.approx(s.last_contact, abs=1e-9)


def _host_list(oracle, seed, n_aircraft=40, n_frames=3000, span_s=60.0):
    """velocity_traffic as (FRAME_DTYPE at 2 MSPS offsets, sps)"""
    sps = 0.5e-6
    traffic = velocity_traffic(oracle, seed=seed, n_aircraft=n_aircraft, n_frames=n_frames, span_s=span_s)
    return _frames([(int(round(t / sps)), fr) for t, fr in traffic]), sps


@pytest.mark.gpu
def test_known_answers_through_a_table(gpu):
    sps = 0.5e-6
    frames = _frames([(1000, bytes.fromhex(KNOWN_ST1)), (3000, bytes.fromhex(KNOWN_ST3))])
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, A.TrackTable(d, max_frames=16, seconds_per_sample=sps) as t:
        t.update(frames, sample_base=10)
        recs, _ = t.aircraft()
        vel = t.velocity()
    assert [int(r["icao"]) for r in recs] == [0x485020, 0xA05F21] and all(r["n_frames"] == 1 for r in recs)
    a, b = vel
    assert a["time"] == 1010 * sps and a["subtype"] == 1 and a["flags"] == SPEED | DIRECTION | VRATE
    assert (int(a["v_ew_kt"]), int(a["v_ns_kt"]), int(a["vertical_rate_fpm"]), int(a["vrate_baro"])) == (-8, -159,
                                                                                                        -832, 0)
    assert a["speed_kt"] == np.float32(math.sqrt(8 * 8 + 159 * 159))
    assert float(a["direction_deg"]) == pytest.approx(182.8804, abs=1e-4)
    assert b["time"] == 3010 * sps and b["subtype"] == 3 and b["flags"] == SPEED | DIRECTION | VRATE
    assert b["direction_deg"] == np.float32(243.984375) and b["speed_kt"] == np.float32(375.0)
    assert (int(b["airspeed_tas"]), int(b["vertical_rate_fpm"]), int(b["vrate_baro"])) == (1, -2304, 1)
    _same_velocity(vel, recs, last_velocity(_timed(frames, 10, sps)))


@pytest.mark.gpu
def test_random_messages_match_the_model(gpu, oracle):
    """4000 aircraft with one random TC 19 message each (subtypes 0-7, raw fields zero, one, maximum or random) in one
    update: every field of every record equals the model; subtypes 0 and 5-7 leave the record without velocity."""
    rng = np.random.default_rng(5)
    icaos = rng.choice(np.arange(1, 1 << 24), size=4000, replace=False)
    items = [(64 * k, random_velocity_frame(oracle, rng, int(icao))) for k, icao in enumerate(icaos)]
    frames, sps = _frames(items), 0.5e-6
    want = last_velocity(_timed(frames, 0, sps))
    subtypes = {int(fr[4]) & 7 for _, fr in items}
    assert subtypes == set(range(8))
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_frames=len(frames), seconds_per_sample=sps) as t:
        t.update(frames)
        recs, flags = t.aircraft()
        vel = t.velocity()
    assert flags == 0 and len(recs) == 4000 and all(r["n_frames"] == 1 for r in recs)
    _same_velocity(vel, recs, want)
    got = {(int(v["subtype"]), int(v["flags"])) for v in vel}
    assert len(want) < 4000 and (0, 0) in got                     # ST 0, 5-7: none
    for st in (1, 2, 3, 4):                                       # every subtype with and without every field
        assert any(s == st and f == SPEED | DIRECTION | VRATE for s, f in got), st
        assert any(s == st and not f & SPEED for s, f in got), st
        assert any(s == st and not f & VRATE for s, f in got), st
    assert {int(v["v_ew_kt"]) < 0 for v in vel if v["flags"] & SPEED and v["subtype"] <= 2} == {False, True}
    assert {int(v["vertical_rate_fpm"]) < 0 for v in vel if v["flags"] & VRATE} == {False, True}
    assert max(abs(int(v["v_ns_kt"])) for v in vel) == 1022 * 4  # maximum raw field, supersonic


@pytest.mark.gpu
def test_streaming_velocity_and_records(gpu, oracle):
    """Modulated traffic with a third of its frames TC 19 through the per-buffer feed in 20 000-sample buffers, one
    update per popped buffer: velocity is the last ST 1-4 message's, every other record field still the oracle's."""
    from tests.golden.make_golden import modulate, place
    traffic = velocity_traffic(oracle, seed=31, n_aircraft=35, n_frames=3000)
    chunk, gap = 20_000, 400
    sps = 1.0 / chunk
    n = 300 + gap * len(traffic) + 600
    items = [(300 + gap * k, modulate(fr, (80, 30), None)) for k, (_, fr) in enumerate(traffic)]
    iq = place(n, items, np.int8, floor=3, seed=31)
    ot = oracle.tracker()
    counts, seen = {}, []
    n_buf = 0
    with A.AdsbDemod(max_samples=chunk, max_out=1 << 12) as d, \
            A.TrackTable(d, max_frames=1 << 12, seconds_per_sample=sps) as table, \
            A.Feed(d, max_chunk=chunk, carry=False) as f:

        def consume():
            nonlocal n_buf
            frames, flags, first = f.pop()
            assert flags == 0
            table.update(frames, first)
            for t, b in _timed(frames, first, sps):
                ot.update(b, t)
                counts[_icao(b)] = counts.get(_icao(b), 0) + 1
            seen.extend(_timed(frames, first, sps))
            if n_buf % 7 == 0 or f.in_flight == 0:
                recs, _ = table.aircraft()
                _same_table(recs, sorted(ot.aircraft(), key=lambda s: s.icao), counts)
                _same_velocity(table.velocity(), recs, last_velocity(seen))
            n_buf += 1

        for a in range(0, n, chunk):
            b = min(a + chunk, n)
            if b - a < A.WINDOW:
                break
            f.push(iq[a:b])
            if f.in_flight == 2:
                consume()
        while f.in_flight:
            consume()
        recs, _ = table.aircraft()
        _same_table(recs, sorted(ot.aircraft(), key=lambda s: s.icao), counts)
        vel = table.velocity()
        _same_velocity(vel, recs, last_velocity(seen))
    n_vel = sum(decode(b, t) is not None for t, b in seen)
    assert n_buf >= 50 and len(recs) >= 30 and n_vel > 300, (n_buf, len(recs), n_vel)
    assert sum(int(v["subtype"]) != 0 for v in vel) >= 30


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [41, 42])
def test_any_cut_gives_the_same_velocity(gpu, oracle, seed):
    frames, sps = _host_list(oracle, seed, n_aircraft=50, n_frames=2500)
    rng = np.random.default_rng(seed)
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_frames=len(frames), seconds_per_sample=sps) as one, \
            A.TrackTable(d, max_frames=len(frames), seconds_per_sample=sps) as cut:
        one.update(frames)
        edges = np.sort(rng.choice(np.arange(1, len(frames)), size=12, replace=False))
        for a, b in zip(np.concatenate([[0], edges]), np.concatenate([edges, [len(frames)]])):
            cut.update(frames[a:b])
            cut.update(frames[:0])                                   # an empty update changes nothing
        assert one.aircraft()[0].tobytes() == cut.aircraft()[0].tobytes()
        assert one.velocity().tobytes() == cut.velocity().tobytes()
        recs, _ = one.aircraft()
        _same_velocity(one.velocity(), recs, last_velocity(_timed(frames, 0, sps)))


@pytest.mark.gpu
def test_reset_clears_velocity(gpu, oracle):
    sps = 0.5e-6
    frames = _frames([(100, bytes.fromhex(KNOWN_ST1)), (300, bytes.fromhex(KNOWN_ST3))])
    pos = _frames([(500, position_frame(oracle, 0x485020, False, 1000, 2000))])
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, A.TrackTable(d, max_frames=16, seconds_per_sample=sps) as t:
        t.update(frames)
        assert [int(v["subtype"]) for v in t.velocity()] == [1, 3]
        t.reset()
        assert len(t.velocity()) == 0
        t.update(pos)                                                # the same aircraft again, no velocity message
        vel = t.velocity()
    assert len(vel) == 1 and vel[0]["subtype"] == 0 and vel[0]["flags"] == 0 and math.isnan(vel[0]["time"])
    assert vel.tobytes()[8:] == bytes(24)


@pytest.mark.gpu
def test_expire_moves_and_drops_velocity(gpu, oracle):
    """200 aircraft with velocity, every third one silent since t = 1 s: expire evicts those (the lowest ICAO first,
    so the compaction moves survivors into low slots); survivors keep their velocity bit for bit, and an evicted
    aircraft heard again starts without one."""
    sps, rng = 0.5e-6, np.random.default_rng(8)
    icaos = sorted(int(x) for x in rng.choice(np.arange(0x100000, 0x200000), size=200, replace=False))
    old = [a for k, a in enumerate(icaos) if k % 3 == 0]
    first = _frames([(100 * k, random_velocity_frame(oracle, rng, a) if k % 5 else
                      velocity_frame(oracle, a, 1, vew=5, vns=9, vr=3)) for k, a in enumerate(icaos)])
    later = _frames([(4_000_000 + 100 * k, velocity_frame(oracle, a, 3, status=1, heading=k, airspeed=k + 2) if k % 2
                      else position_frame(oracle, a, False, 100 + k, 200 + k))   # half the survivors: a new velocity
                     for k, a in enumerate(icaos) if a not in old])
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackTable(d, max_aircraft=256, max_frames=256, seconds_per_sample=sps) as t:
        t.update(first)
        t.update(later)
        recs, _ = t.aircraft()
        before = dict(zip((int(r["icao"]) for r in recs), t.velocity()))
        _same_velocity(t.velocity(), recs, last_velocity(_timed(first, 0, sps) + _timed(later, 0, sps)))
        t.expire(1.0)
        recs, _ = t.aircraft()
        vel = t.velocity()
        assert [int(r["icao"]) for r in recs] == [a for a in icaos if a not in old]
        for r, v in zip(recs, vel):
            assert v.tobytes() == before[int(r["icao"])].tobytes()
        t.update(_frames([(6_000_000, position_frame(oracle, old[0], True, 10, 20))]))
        recs, _ = t.aircraft()
        vel = t.velocity()
    k = [int(r["icao"]) for r in recs].index(old[0])
    assert recs[k]["n_frames"] == 1 and vel[k]["subtype"] == 0 and vel[k]["flags"] == 0 and math.isnan(vel[k]["time"])
    assert before[old[0]]["subtype"] != 0


def _receiver_lists(oracle, n_receivers, seed):
    """Per receiver, three successive host lists of velocity traffic; the lowest aircraft fly under SHARED ICAOs."""
    out = []
    for r in range(n_receivers):
        traffic = velocity_traffic(oracle, seed=seed * 1000 + r, n_aircraft=8, n_frames=240, span_s=30.0)
        remap = dict(zip(sorted({_icao(fr) for _, fr in traffic}), SHARED))
        lst = []
        for t, fr in traffic:
            if _icao(fr) in remap:
                data = bytes(fr[:1]) + remap[_icao(fr)].to_bytes(3, "big") + bytes(fr[4:11])
                crc = oracle.get_adsb_crc(data)
                fr = data + crc.to_bytes(3, "big")
            lst.append((int(round(t / 0.5e-6)), fr))
        f = _frames(lst)
        out.append([f[:80], f[80:170], f[170:]])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n_receivers,seed", [(1, 1), (3, 2), (8, 3), (64, 4)])
def test_bank_equals_separate_tables(gpu, oracle, n_receivers, seed):
    """Receiver r's velocities equal a table of its own fed receiver r's lists, also for ICAOs active on several
    receivers; one table, reset between receivers, stands in for n_receivers of them."""
    sps = 0.5e-6
    lists = _receiver_lists(oracle, n_receivers, seed)
    bases = [7 * r for r in range(n_receivers)]
    with A.AdsbDemod(max_samples=4096, max_out=64) as d, \
            A.TrackBank(d, n_receivers, max_aircraft=64, max_frames=512 * n_receivers, seconds_per_sample=sps) as bank, \
            A.TrackTable(d, max_aircraft=64, max_frames=512, seconds_per_sample=sps) as table:
        for u in range(3):
            parts = [lists[r][u] for r in range(n_receivers)]
            bank.update(np.concatenate(parts), [len(p) for p in parts], bases)
        recs, _ = bank.aircraft()
        vel = bank.velocity()
        n_shared = 0
        for r in range(n_receivers):
            table.reset()
            for u in range(3):
                table.update(lists[r][u], bases[r])
            trecs, _ = table.aircraft()
            assert recs[r].tobytes() == trecs.tobytes(), r
            assert vel[r].tobytes() == table.velocity().tobytes(), r
            _same_velocity(vel[r], recs[r], last_velocity(sum((_timed(lists[r][u], bases[r], sps) for u in range(3)),
                                                              [])))
            n_shared += sum(int(a["icao"]) in SHARED and v["subtype"] != 0 for a, v in zip(recs[r], vel[r]))
    assert n_shared >= n_receivers


@pytest.mark.gpu
def test_bank_update_launch_velocity(gpu, oracle):
    """A 3-channel device launch of modulated velocity traffic through update_launch gives the velocities of a bank
    fed the fetched host lists, and the model's."""
    import torch

    from tests.golden.make_golden import modulate, place
    C_, n, stride, gap = 3, 20_000, 20_480, 500
    sps = 1.0 / n
    streams = [iter(velocity_traffic(oracle, seed=70 + c, n_aircraft=20, n_frames=400)) for c in range(C_)]
    seen = [[] for _ in range(C_)]
    with A.AdsbDemod(max_samples=n, max_out=1024, max_channels=C_, host_staging=False) as d, \
            A.TrackBank(d, C_, max_frames=1024, seconds_per_sample=sps) as bank, \
            A.TrackBank(d, C_, max_frames=1024, seconds_per_sample=sps) as host_bank:
        for launch in range(5):
            host = np.full((C_, stride, 2), 77, dtype=np.int8)
            for c in range(C_):
                items = [(300 + gap * k, modulate(next(streams[c])[1], (80, 30), None)) for k in range((n - 600) // gap)]
                host[c, :n] = place(n, items, np.int8, floor=3, seed=100 * launch + c)
            buf = torch.from_numpy(host).cuda()
            d.demod_device_async(buf.data_ptr(), n, C_, stride)
            bases = [launch * n + r for r in range(C_)]
            bank.update_launch(bases)
            frames, counts, _, flags = d.fetch(n_channels=C_)
            assert flags == 0
            host_bank.update(frames, [int(x) for x in counts], bases)
            a = 0
            for c in range(C_):
                seen[c].extend(_timed(frames[a:a + int(counts[c])], bases[c], sps))
                a += int(counts[c])
        recs, _ = bank.aircraft()
        vel = bank.velocity()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(recs, host_bank.aircraft()[0]))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(vel, host_bank.velocity()))
    for c in range(C_):
        _same_velocity(vel[c], recs[c], last_velocity(seen[c]))
        assert sum(int(v["subtype"]) != 0 for v in vel[c]) >= 10


@pytest.mark.gpu
def test_replay_aircraft_table(gpu, oracle, tmp_path):
    """tools/replay.py --aircraft on a .c16 capture prints the table the oracle and the model predict, Velocity filled;
    without the flag it prints the stream text as before (TC 19 frames as of unknown type)."""
    from tests.golden.make_golden import modulate, place
    traffic = velocity_traffic(oracle, seed=77, n_aircraft=15, n_frames=400, span_s=10.0)
    chunk, per_chunk, gap = 20_000, 40, 400
    offsets = [chunk * (k // per_chunk) + 300 + gap * (k % per_chunk) for k in range(len(traffic))]
    n = chunk * (len(traffic) // per_chunk + 2)                  # the last, frameless chunk is never sent
    iq = place(n, [(o, modulate(fr, (80, 30), None)) for o, (_, fr) in zip(offsets, traffic)], np.int16, floor=3,
               seed=77)
    path = tmp_path / "capture.c16"
    iq.astype("<i2").tofile(path)
    sps = 0.5e-6
    timed = [(o * sps, fr) for o, (_, fr) in zip(offsets, traffic)]
    ot = oracle.tracker()
    heard = {}
    for t, fr in timed:
        ot.update(fr, t)
        heard[_icao(fr)] = t
    vel = last_velocity(timed)
    rows = []
    for s in ot.aircraft():
        v = vel.get(s.icao)
        age = int(n * sps - heard[s.icao])
        rows.append((age, s.icao, "\t".join([
            f"{s.icao:x}", s.callsign.decode().rstrip("\0"), str(s.altitude),
            f"{s.latitude:.6f}" if s.has_position else "n/a", f"{s.longitude:.6f}" if s.has_position else "n/a",
            f"{float(v['speed_kt']):.0f}" if v is not None and v["flags"] & SPEED else "n/a", str(age)])))
    want = "ICAO\tCallsign\tAltitude\tLatitude\tLongitude\tVelocity\tAge\n" + \
        "".join(r[2] + "\n" for r in sorted(rows, key=lambda r: (r[0], r[1])))
    assert sum(r[2].split("\t")[5] != "n/a" for r in rows) >= 5 and len(rows) >= 10  # some rows carry a velocity
    tool = os.path.join(ROOT, "tools", "replay.py")
    got = subprocess.run([sys.executable, tool, str(path), "--aircraft"], capture_output=True, text=True, timeout=300,
                         check=True).stdout
    assert got == want
    stream = subprocess.run([sys.executable, tool, str(path)], capture_output=True, text=True, timeout=300,
                            check=True).stdout
    assert stream == "".join("\n" + oracle.packet_display(fr, "") + "\n" for _, fr in timed)
    assert "Message Type    : 19" in stream                       # TC 19 frames print as before
