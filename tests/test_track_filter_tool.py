"""tools/mlat.py --aircraft --filter through the CPU mirrors (--host): without the flag the output is byte for byte what
it was, with it six columns are appended last, and an aircraft that sends no ADS-B gets a speed and a track.  No device."""
import os
import subprocess
import sys

from tests import track_filter_cases as K
from tests import track_modes_cases as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = [sys.executable, os.path.join(ROOT, "tools", "mlat.py"), "--host"]
COLUMNS = ["Lat(f)", "Lon(f)", "GS(f)", "Trk(f)", "VR(f)", "Outl"]


def test_six_more_columns_and_the_rest_unchanged(lib, oracle, tmp_path):
    args = N.recordings(N.network(oracle), tmp_path)
    for more in (["--modes", "--aircraft", "--max-iterations", "200"], ["--aircraft"]):
        plain = subprocess.run(TOOL + more + args, capture_output=True, text=True, check=True).stdout
        wide = subprocess.run(TOOL + more + ["--filter"] + args, capture_output=True, text=True, check=True).stdout
        rows, cols = [l.split("\t") for l in plain.splitlines()], [l.split("\t") for l in wide.splitlines()]
        assert len(rows) == len(cols) >= 2 and cols[0][-6:] == COLUMNS
        for a, b in zip(rows, cols):
            assert b[:-6] == a and len(b) == len(a) + 6
    N.check_table(subprocess.run(TOOL + ["--modes", "--aircraft", "--max-iterations", "200"] + args, capture_output=True,
                                 text=True, check=True).stdout)
    bad = subprocess.run(TOOL + ["--filter"] + args, capture_output=True, text=True)
    assert bad.returncode != 0 and "--filter needs --aircraft" in bad.stderr


def test_an_aircraft_without_ads_b_gets_a_speed_and_a_track(lib, tmp_path):
    net = K.flying_network()
    args = N.recordings(net, tmp_path)
    out = subprocess.run(TOOL + ["--modes", "--aircraft", "--filter", "--max-iterations", "200"] + args,
                         capture_output=True, text=True, check=True).stdout
    rows = [l.split("\t") for l in out.splitlines()]
    assert len(rows) == 2 and rows[0][-6:] == COLUMNS and rows[1][0] == f"{K.MODE_S:06X}" and rows[1][15] == "S"
    assert rows[1][2:4] == ["n/a", "n/a"]                                 # it reports no position of its own
    lat, lon, gs, trk, vr, outl = rows[1][-6:]
    print("\n" + out)
    assert abs(float(lat) - net["truth"][-1, 0]) < 0.02 and abs(float(lon) - net["truth"][-1, 1]) < 0.03
    want_kt = net["speed"] * 3600.0 / 1852.0
    assert abs(float(gs) - want_kt) < 0.25 * want_kt and abs(float(trk) - net["heading"]) < 20.0 and int(outl) <= 3
