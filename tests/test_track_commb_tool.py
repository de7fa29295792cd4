"""tools/mlat.py --modes --commb --aircraft through the CPU mirrors (--host), on tests/track_modes_cases.py's network:
the table without --commb stays what it was, and six columns are appended.  No device."""
import os
import subprocess
import sys

from tests import track_modes_cases as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_six_more_columns_and_the_rest_unchanged(lib, oracle, tmp_path):
    args = N.recordings(N.network(oracle), tmp_path)
    tool = [sys.executable, os.path.join(ROOT, "tools", "mlat.py"), "--host", "--modes", "--aircraft", "--max-iterations", "200"]
    plain = subprocess.run(tool + args, capture_output=True, text=True, check=True).stdout
    N.check_table(plain)
    more = subprocess.run(tool + ["--commb"] + args, capture_output=True, text=True, check=True).stdout
    rows, wide = [l.split("\t") for l in plain.splitlines()], [l.split("\t") for l in more.splitlines()]
    assert len(rows) == len(wide) == 3
    assert wide[0][16:] == list(lib.AIRCRAFT_COMMB_COLUMNS) == ["SelAlt", "QNH", "GS/Trk(B)", "Hdg", "IAS", "Mach"]
    for a, b in zip(rows, wide):
        assert b[:16] == a and len(b) == 22
    assert wide[1][16:] == ["n/a"] * 6 and wide[2][16:] == ["n/a"] * 6       # BDS 2,0 replies only: nothing to show
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mlat.py"), "--host", "--modes", "--commb"] + args,
                         capture_output=True, text=True)
    assert bad.returncode != 0 and "--commb needs --modes and --aircraft" in bad.stderr


def test_the_columns_of_a_settled_reply(lib):
    from tests import track_commb_cases as K
    case = K.twelve()
    addresses, recs, out = lib.host_track_commb(case["frames"].view(lib.FRAME_DTYPE), case["recs"].view(lib.MODES_DTYPE),
                                                case["commb"].view(lib.COMMB_DTYPE))
    assert addresses.tolist() == [K.B, K.A]
    cols = lib.aircraft_commb_columns(recs)
    assert cols[0] == ["n/a"] * 6 and cols[1] == ["n/a", "n/a", "430/254*", "n/a", "n/a", "n/a"]
    want_out, want_recs, _ = K.run_model(case)
    assert out.tobytes() == want_out.tobytes() and recs.tobytes() == want_recs.tobytes()
    reg = K.registers()
    cols = lib.aircraft_commb_columns(lib.host_track_commb(reg["frames"].view(lib.FRAME_DTYPE), reg["recs"].view(lib.MODES_DTYPE),
                                                           reg["commb"].view(lib.COMMB_DTYPE))[1])
    assert cols[2] == ["21840", "881.9", "438/114", "290", "280", "0.800"]   # unambiguous replies carry no mark
