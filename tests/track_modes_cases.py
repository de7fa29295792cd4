"""The network the Mode S side of the track table is checked on end to end (tests/test_gpu_track_modes.py on the device,
tests/test_track_modes_tool.py through tools/mlat.py --host): tests/test_gpu_modes_chain.py's geometry with DF20 replies
that carry a BDS 2,0 callsign added."""
import numpy as np

from tests import modes_model as M

MODE_S, ADSB = 0x3C4A5B, 0x400123


def network(oracle):
    """Five receivers' Beast streams: one ADS-B aircraft, one that only answers interrogations (DF11, DF4, DF5, DF20 with
    BDS 2,0), and garbage heard by one receiver each.  tests/test_gpu_modes_chain.py's geometry."""
    from tests import mlat_cases as MK
    from tests import traffic
    from tests import wire_in_short_model as S
    rcv = MK.receivers(5, seed=946)
    pos, _ = MK.emitters(oracle, 24, seed=947)
    rng = np.random.default_rng(948)
    f25 = lambda k: M.field_of(Q=1) | (0x0A80 + 0x80 * (k % 4))
    frames, heard, who = [], [], []
    for i in range(24):
        if i == 0:
            frames.append(M.all_call(MODE_S)), who.append("s")
        elif i % 3 == 0:
            frames.append(traffic.position_frame(oracle, ADSB, i & 1, 1000 + i, 2000 + i, alt_code=0xC38, tc=11)), who.append("a")
        elif i % 8 == 5:
            junk = bytes([(4 if i % 16 == 5 else 17) << 3]) + bytes(rng.integers(0, 256, size=13).astype(np.uint8))
            frames.append(junk[:7] if junk[0] >> 3 == 4 else junk), who.append("g")
        elif i % 4 == 2:
            frames.append(M.reply(20, MODE_S, low3=0, b1=i, field=f25(i), rest=M.callsign_mb("SILENT1_"))), who.append("s")
        elif i % 2:
            frames.append(M.reply(4, MODE_S, low3=0, b1=i, field=f25(i))), who.append("s")
        else:
            frames.append(M.reply(5, MODE_S, low3=0, b1=i, field=M.field_of(A4=1, B2=1, C1=1))), who.append("s")
        heard.append([i % 5] if who[-1] == "g" else list(range(5)))
    padded = [f.ljust(14, b"\0") for f in frames]
    lst = MK.build(rcv, pos, padded, spt=0.5e-6, heard=heard)
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
    return dict(rcv=rcv, pos=pos, who=who, frames=frames, streams=streams, ends=ends)




def recordings(net, directory):
    """The streams as files beside a sites file -> the tool's positional arguments"""
    sites = directory / "sites.csv"
    sites.write_text("".join(f"{float(r['latitude'])!r},{float(r['longitude'])!r},{float(r['height_m'])!r}\n" for r in net["rcv"]))
    paths = []
    for r, stream in enumerate(net["streams"]):
        paths.append(directory / f"r{r}.beast")
        paths[-1].write_bytes(stream)
    return [str(sites)] + [str(p) for p in paths]


def check_table(text):
    """tools/mlat.py --modes --aircraft on the recordings: two rows, the Mode S aircraft placed and marked"""
    rows = [line.split("\t") for line in text.splitlines() if not line.startswith("#")]
    assert rows[0] == ["ICAO", "Callsign", "Latitude", "Longitude", "MlatLat", "MlatLon", "Age", "Pdop", "Valid/Attempted",
                       "Checked/Disagree", "MaxDisagreement", "Alt(S)", "Squawk", "Call(S)", "Replies", "S"]
    assert [row[0] for row in rows[1:]] == [f"{MODE_S:06X}", f"{ADSB:06X}"] and all(len(row) == 16 for row in rows)
    silent, adsb = rows[1], rows[2]
    n_replies = 24 - 7 - 2                                                # 24 messages, 7 squitters, 2 of garbage
    assert silent[15] == "S" and silent[14] == str(n_replies) and silent[12] == "4210" and silent[13] == "SILENT1"
    assert silent[1] == silent[2] == silent[3] == "n/a" and silent[4] != "n/a" and silent[8] == f"{n_replies}/{n_replies}"
    assert int(silent[11]) in {25 * n - 1000 for n in range(2048)}
    assert adsb[15] == "" and adsb[14] == "0" and adsb[11:14] == ["n/a"] * 3 and adsb[8].split("/")[1] == "7"
