"""tools/mlat.py --sync through the CPU mirrors (--host): Beast recordings of five receivers with clock offsets and
drifts -> wire input -> correlate -> clock sync -> corrected receptions -> the solver.  The tool is what the test is
about, so it is started as a command."""
import os
import subprocess
import sys

import numpy as np
import pytest

import air_rs_amd as A
from tests import clock_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recordings(oracle, tmp_path_factory):
    """2 MHz frame offsets (what the Beast encoder multiplies by 6), offsets inside the default correlate window."""
    sc = CC.scenario(oracle, 5, 80, seed=3, spt=0.5e-6, offset_s=2e-4, drift=5e-6, p_heard=1.0, tick_base=1000)
    d = tmp_path_factory.mktemp("mlat_tool")
    sites = d / "sites.csv"
    sites.write_text("# latitude,longitude,height_m\n" +
                     "".join(f"{float(r['latitude'])!r},{float(r['longitude'])!r},{float(r['height_m'])!r}\n" for r in sc["rcv"]))
    paths, at = [], 0
    for r in range(5):
        mine = sc["lst"]["frames"][at:at + int(sc["lst"]["counts"][r])]
        at += len(mine)
        paths.append(d / f"r{r}.beast")
        paths[-1].write_bytes(A.host_wire_encode(mine)[0])
    return sc, [str(sites)] + [str(p) for p in paths]


def _run(args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mlat.py"), "--host"] + args, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    clocks = [line.split() for line in out.stdout.splitlines() if line.startswith("# clock")]
    fixes = [line.split() for line in out.stdout.splitlines() if line and not line.startswith("#")]
    return clocks, fixes, out.stderr


def _residuals(fixes):
    return np.array([float(f[5]) for f in fixes])


def test_sync_prints_the_clocks_and_better_fixes(lib, recordings):
    sc, args = recordings
    none, raw, _ = _run(args)
    assert none == [] and len(raw) > 0
    clocks, fixed, err = _run(["--sync", "--max-residual-us", "5"] + args)
    assert len(clocks) == 5 and "80 messages" in err
    assert clocks[0][3] == "reference" and all(c[3] == "reached" for c in clocks[1:])
    # the clocks against the scenario's: 2 MHz samples are 0.5 us, the estimates are good to a fraction of one
    ta, tb = CC.truth(sc)
    assert np.abs(np.array([float(c[5]) for c in clocks]) - ta).max() < 2e-7
    assert np.abs(np.array([float(c[8]) for c in clocks]) * 1e-6 - tb).max() < 2e-8
    # uncorrected offsets of 0.2 ms are 60 km of range: the residuals say so, the corrected ones are those of a tick
    assert len(fixed) >= 70 and np.median(_residuals(fixed)) < 150.0 < 1000.0 < np.median(_residuals(raw))


def test_reference(lib, recordings):
    sc, args = recordings
    clocks, fixed, _ = _run(["--sync", "--reference", "2"] + args)
    assert [c[3] for c in clocks] == ["reached", "reached", "reference", "reached", "reached"]
    ta, _ = CC.truth(sc, reference=2)
    assert np.abs(np.array([float(c[5]) for c in clocks]) - ta).max() < 2e-7 and len(fixed) >= 70
