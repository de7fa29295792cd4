"""Mode S replies end to end on the device: five receivers hear an aircraft that sends no ADS-B -- a DF11 all-call reply,
then DF4 and DF5 surveillance replies -- beside one ADS-B aircraft and garbage.  Their Beast streams go through
wire_in_of(SHORT) -> correlate_of -> modes_of on correlate's frames_out -> multilaterate, all where the lists lie on the
device: the replies get the aircraft's address and are placed, the garbage gets none, and the squitters are the ADS-B
aircraft's frames, which a track table accepts.  Geometry and tolerance are tests/test_gpu_mlat.py's end-to-end test's."""
import numpy as np
import pytest

import air_rs_amd as A
from tests import mlat_cases as K
from tests import mlat_model as MM
from tests import modes_model as M
from tests import traffic
from tests import wire_in_short_model as S

pytestmark = pytest.mark.gpu
MODE_S, ADSB = 0x3C4A5B, 0x400123


def test_a_mode_s_only_aircraft_is_placed(gpu, oracle):
    rcv = K.receivers(5, seed=946)
    pos, _ = K.emitters(oracle, 24, seed=947)
    rng = np.random.default_rng(948)
    f25 = lambda k: M.field_of(Q=1) | (0x0A80 + 0x80 * (k % 4))
    frames, heard, who = [], [], []
    for i in range(24):
        if i == 0:
            frames.append(M.all_call(MODE_S)), who.append("s")                                  # iid 0: SELF
        elif i % 3 == 0:
            frames.append(traffic.position_frame(oracle, ADSB, i & 1, 1000 + i, 2000 + i, alt_code=0xC38, tc=11)), who.append("a")
        elif i % 8 == 5:
            junk = bytes([(4 if i % 16 == 5 else 17) << 3]) + bytes(rng.integers(0, 256, size=13).astype(np.uint8))
            frames.append(junk[:7] if junk[0] >> 3 == 4 else junk), who.append("g")
        elif i % 2:
            frames.append(M.reply(4, MODE_S, low3=0, b1=i, field=f25(i))), who.append("s")
        else:
            frames.append(M.reply(5, MODE_S, low3=0, b1=i, field=M.field_of(A4=1, B2=1, C1=1))), who.append("s")
        heard.append([i % 5] if who[-1] == "g" else list(range(5)))                                     # garbage: one receiver
    assert who.count("s") >= 10 and who.count("a") >= 6 and who.count("g") >= 2
    padded = [f.ljust(14, b"\0") for f in frames]
    lst = K.build(rcv, pos, padded, spt=0.5e-6, heard=heard)                                     # offsets in 2 MHz samples
    streams, ends, at = [], [], 0
    for r in range(5):
        mine = lst["frames"][at:at + int(lst["counts"][r])]
        at += len(mine)
        parts = []
        for f in mine:
            msg = f["bytes"].tobytes()
            short = msg[0] >> 3 < 16
            parts.append(S.beast_frame(b"2" if short else b"3", 6 * int(f["offset"]), 40 + r, msg[:7] if short else msg))
        streams.append(b"".join(parts))
        ends.append(sum(len(s) for s in streams))
    with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
        old = d.wire_in_of(b"".join(streams), ends)                                              # without the bit: long frames only
        assert len(old.frames) == sum(len(f) == 14 for f, h in zip(frames, heard) for _ in h)
        win = d.wire_in_of(b"".join(streams), ends, filter="short")
        assert win.counts.tolist() == lst["counts"].tolist() and win.frames["bytes"].tobytes() == lst["frames"]["bytes"].tobytes()
        assert (win.rx["ticks"] == 6 * lst["frames"]["offset"]).all()
        frames_dev, rx_dev = d.wire_in_device()[:2]
        d.correlate_of_async((frames_dev, len(win.frames)), win.counts, 5000)
        msgs, frames_out, recs = d.fetch_correlated()
        assert len(msgs) == 24
        mrec, known_out, squitters, _, hdr = d.modes_of((d.correlated_device()[1], len(msgs)))
        M.same((mrec, known_out, squitters, None, hdr), M.modes(frames_out), "model")
        # (no altitude equation for these formats: a free solve over ground receivers, which are nearly coplanar, creeps
        # along the height and needs more than the default 24 steps to come to rest)
        fixes, mh = d.multilaterate(rcv, rx=rx_dev, time_source="ticks", max_iterations=200)
        # messages are in time order, which is the order they were sent in
        assert [m["bytes"].tobytes() for m in msgs] == padded
        mode_s = np.array([w == "s" for w in who])
        assert mrec["kind"][0] == M.SELF and (mrec["kind"][mode_s][1:] == M.KNOWN).all()
        assert (mrec["address"][mode_s] == MODE_S).all() and (msgs["n_receivers"][mode_s] == 5).all()
        replies = mrec[mode_s][1:]
        assert {4, 5} == set(replies["df"].tolist())
        assert ((replies["df"] == 4) == (replies["flags"] & M.ALT != 0)).all() and set(replies["squawk"][replies["df"] == 5].tolist()) == {4210}
        assert set(replies["altitude_ft"][replies["df"] == 4].tolist()) <= {25 * n - 1000 for n in range(2048)}
        garbage = np.array([w == "g" for w in who])
        assert np.isin(mrec["kind"][garbage], (M.UNKNOWN, M.PARITY)).all()
        # the fixes of the Mode S aircraft: valid and near their emitters, by the rule of the ADS-B end-to-end test
        valid = fixes["flags"] & MM.VALID != 0
        assert valid[mode_s].all() and not valid[garbage].any()
        err = np.array([float(np.sqrt(((MM.ecef_of(f["latitude"], f["longitude"], f["height_m"]) - p) ** 2).sum()))
                        for f, p in zip(fixes, pos)])
        print(f"Mode S fixes: largest error {err[mode_s].max():.0f} m, median {np.median(err[mode_s]):.0f} m, "
              f"largest pdop {float(fixes['pdop'][mode_s].max()):.2f}")
        assert err[mode_s].max() < 150.0 * 3 * float(fixes["pdop"][mode_s].max()) and np.median(err[mode_s]) < 5000.0
        # the squitters are the ADS-B aircraft's frames, and a track table takes them
        adsb = np.array([w == "a" for w in who])
        assert squitters.tobytes() == frames_out[adsb].tobytes() and int(hdr["n_squitters"]) == adsb.sum()
        assert known_out.tolist() == sorted([MODE_S, ADSB])
        with A.TrackTable(d, max_aircraft=64, max_frames=256) as table:
            table.update_device(d.modes_device()[2], len(squitters))
            craft, flags = table.aircraft()
            assert craft["icao"].tolist() == [ADSB] and int(craft["n_frames"][0]) == adsb.sum() and flags == 0
            assert d.modes_of(frames_out, known=table)[0]["kind"][garbage].tolist() == mrec["kind"][garbage].tolist()
