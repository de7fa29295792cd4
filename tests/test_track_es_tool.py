"""The aircraft table's extended squitter columns: tools/mlat.py --modes --es --aircraft through the CPU mirrors (--host),
on tests/track_modes_cases.py's network, and the column text itself from the mirror's records.  tools/replay.py --es
--aircraft needs the device and is in tests/test_gpu_track_es.py.  No device."""
import os
import subprocess
import sys

import numpy as np

from tests import track_es_cases as K
from tests import track_modes_cases as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = ["Ver", "NIC", "Rc", "NACp", "SIL", "Emerg", "Squawk(ES)", "SelAlt"]


def test_eight_more_columns_and_the_rest_unchanged(lib, oracle, tmp_path):
    args = N.recordings(N.network(oracle), tmp_path)
    tool = [sys.executable, os.path.join(ROOT, "tools", "mlat.py"), "--host", "--modes", "--aircraft", "--max-iterations", "200"]
    plain = subprocess.run(tool + args, capture_output=True, text=True, check=True).stdout
    N.check_table(plain)
    more = subprocess.run(tool + ["--es"] + args, capture_output=True, text=True, check=True).stdout
    rows, wide = [l.split("\t") for l in plain.splitlines()], [l.split("\t") for l in more.splitlines()]
    assert len(rows) == len(wide) == 3
    assert wide[0][16:] == list(lib.AIRCRAFT_ES_COLUMNS) == COLUMNS
    for a, b in zip(rows, wide):
        assert b[:16] == a and len(b) == 24
    assert wide[1][16:] == ["n/a"] * 8                                       # the aircraft that only answers interrogations
    adsb = wide[2][16:]                                                      # squitters, but no operational status among them
    assert adsb == ["n/a", "0?", "185.2?", "n/a", "n/a", "n/a", "n/a", "n/a"]   # its newest position is a TC 11: 185.2 m, unversioned
    both = subprocess.run(tool + ["--commb", "--es"] + args, capture_output=True, text=True, check=True).stdout
    assert [l.split("\t")[22:] for l in both.splitlines()] == [w[16:] for w in wide]
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mlat.py"), "--host", "--modes", "--es"] + args,
                         capture_output=True, text=True)
    assert bad.returncode != 0 and "--es needs --modes and --aircraft" in bad.stderr


def _columns(lib, case, keyed=False):
    frames, es, recs = case["frames"].view(lib.FRAME_DTYPE), case["es"].view(lib.ES_DTYPE), case["recs"].view(lib.MODES_DTYPE)
    icaos, side, _ = lib.host_track_es(frames, es, recs if keyed else None)
    return dict(zip(icaos.tolist(), lib.aircraft_es_columns(side)))


def test_the_columns_of_a_resolved_and_of_an_unversioned_position(lib):
    msgs = [K.status(K.A, 2, nic_a=1), K.position(K.A, 11, 1), K.position(K.B, 11, 1), K.emergency(K.A, 1, 7700), K.target(K.A)]
    exact = _columns(lib, K.build("heard and not heard", msgs))
    assert exact[K.A] == ["2", "9", "75.0", "10", "2", "1", "7700", "16992"]
    assert exact[K.B] == ["n/a", "0?", "185.2?", "n/a", "n/a", "n/a", "n/a", "n/a"]
    # the status heard only after the position: the newest position was resolved without it, and is marked; a target state
    # message after the position (the first list) does not unmark a position that was resolved with a version
    exact = _columns(lib, K.build("status after", [K.position(K.A, 11, 1), K.status(K.A, 1, nic_a=1, nac_p=8, sil=1)]))
    assert exact[K.A] == ["1", "0?", "185.2?", "8", "1", "n/a", "n/a", "n/a"]
    # an unknown radius is n/a, and the mark stays with NIC
    exact = _columns(lib, K.build("TC 8 of version 1", [K.status(K.A, 1, nic_a=1, surface=True), K.position(K.A, 8)]))
    assert exact[K.A][:3] == ["1", "0", "n/a"]
    exact = _columns(lib, K.every_block())
    assert exact[K.A] == ["2", "8", "185.2", "10", "2", "1", "7700", "16992"]


def test_physical_units(lib):
    case = K.every_block()
    side = lib.host_track_es(case["frames"].view(lib.FRAME_DTYPE), case["es"].view(lib.ES_DTYPE))[1]
    stateless = lib.es_physical(case["es"].view(lib.ES_DTYPE)[3:4])           # the target state message itself
    phys = lib.aircraft_es_physical(side)
    for key in ("selected_altitude_ft", "baro_setting_mb", "selected_heading_deg"):
        assert phys[key][0] == stateless[key][0] and not np.isnan(phys[key][0]), key
    assert abs(phys["rc_m"][0] - 185.2) < 1e-9
    assert set(phys) == {"rc_m", "selected_altitude_ft", "baro_setting_mb", "selected_heading_deg"}
