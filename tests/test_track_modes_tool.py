"""tools/mlat.py --modes --aircraft through the CPU mirrors (--host): Beast recordings of five receivers with an aircraft
that only answers interrogations -> wire input with short frames -> correlate -> the Mode S stage -> the solver -> the
table keyed by the resolved addresses.  The tool is what the test is about, so it is started as a command, once.  The
device path is compared with this one in tests/test_gpu_track_modes.py."""
import os
import subprocess
import sys

from tests import track_modes_cases as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_mode_s_only_aircraft_has_a_row(lib, oracle, tmp_path):
    args = N.recordings(N.network(oracle), tmp_path)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mlat.py"), "--host", "--modes", "--aircraft",
                          "--max-iterations", "200"] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    N.check_table(out.stdout)
    # without --aircraft: one line per fix of a message with an aircraft's address, none for the garbage
    fixes = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mlat.py"), "--host", "--modes", "--max-iterations", "200"]
                           + args, capture_output=True, text=True, timeout=120)
    assert fixes.returncode == 0, fixes.stderr
    who = [line.split()[1] for line in fixes.stdout.splitlines()]
    assert set(who) == {f"{N.MODE_S:06X}", f"{N.ADSB:06X}"} and who.count(f"{N.MODE_S:06X}") == 15
