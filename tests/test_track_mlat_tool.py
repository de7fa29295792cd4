"""tools/mlat.py --aircraft through the CPU mirrors (--host): Beast recordings of eight receivers -> wire input ->
correlate -> clock sync -> the solver -> the per-aircraft mlat records.  The tool is what the test is about, so it is
started as a command, once."""
import os
import subprocess
import sys

import pytest

import air_rs_amd as A
from tests import track_mlat_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lines(oracle, tmp_path_factory):
    """2 MHz frame offsets (what the Beast encoder multiplies by 6), clock offsets inside the default correlate window;
    the aircraft that lies is 0.1 degrees (11 km) off."""
    sc = K.network(oracle, spt=0.5e-6, displaced_deg=0.1, offset_s=2e-4, drift=5e-6, tick_base=1000)
    d = tmp_path_factory.mktemp("mlat_aircraft")
    sites = d / "sites.csv"
    sites.write_text("".join(f"{float(r['latitude'])!r},{float(r['longitude'])!r},{float(r['height_m'])!r}\n" for r in sc["rcv"]))
    paths, at = [], 0
    for r in range(8):
        mine = sc["lst"]["frames"][at:at + int(sc["lst"]["counts"][r])]
        at += len(mine)
        paths.append(d / f"r{r}.beast")
        paths[-1].write_bytes(A.host_wire_encode(mine)[0])
    # a 2 MHz sample is 150 m of range and the solver's dilution makes about 1.5 km of it at worst here; the lie is
    # 11 km: the limit sits between the two
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mlat.py"), "--host", "--aircraft", "--sync",
                          "--max-residual-us", "5", "--max-disagreement", "4000", str(sites)] + [str(p) for p in paths],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return [line.split("\t") for line in out.stdout.splitlines() if not line.startswith("#")]


def test_one_line_per_aircraft(lib, lines):
    assert lines[0] == ["ICAO", "Callsign", "Latitude", "Longitude", "MlatLat", "MlatLon", "Age", "Pdop",
                        "Valid/Attempted", "Checked/Disagree", "MaxDisagreement"]
    assert [row[0] for row in lines[1:]] == [f"{0x400000 + k:06X}" for k in range(16)]
    assert all(len(row) == 11 for row in lines)


def test_the_liar_disagrees_and_the_silent_are_placed(lib, lines):
    for row in lines[1:]:
        icao = int(row[0], 16)
        valid, attempted = (int(x) for x in row[8].split("/"))
        checked, disagree = (int(x) for x in row[9].split("/"))
        assert attempted == 10 and valid >= 7 and row[4] != "n/a" and float(row[6]) >= 0.0, row
        if icao == K.LIAR:
            assert checked == disagree == valid and 9000 < float(row[10]) < 13000, row
        elif icao in (K.VELOCITY_ONLY, K.IDENT_ONLY):
            assert checked == 0 and row[2] == row[3] == row[10] == "n/a", row          # placed, though it says nothing
        else:
            assert checked == valid and disagree == 0 and float(row[10]) < 4000, row
