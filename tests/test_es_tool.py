"""tools/replay.py --es, CPU tier: the text one ES_DTYPE record gives (es_text) and the lines of a frame list (es_lines),
on the mirror's records of the known answers and of a few constructed frames.  The command itself needs a device
(tests/test_gpu_es.py starts it, through --avr-in)."""
import importlib.util
import os

from tests import es_cases as K
from tests import es_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN_TEXT = ["EMERGENCY state=0 squawk=6513",
              "TARGET_STATE alt=16992ft(mcp) baro=1012.8mb hdg=66.8 nac_p=9 nic_baro=1 sil=3 modes=autopilot,vnav,lnav tcas",
              "CATEGORY A0",
              "VELOCITY st=1 nac_v=0 ifr",
              "POSITION tc=11 nic_b=0 rc=185.2m",
              "POSITION tc=7 rc=185.2m",
              "OPERATIONAL st=0 v2 cc=2300 om=0300 nic_a=0 nac_p=9 sil=3 nic_baro=1 sil_supp=0 sda=3 gva=2"]
KNOWN_ADDRESSES = ["A2C1B6", "A05629", "4840D6", "485020", "40621D", "484175", "4840D6"]


def _tool():
    spec = importlib.util.spec_from_file_location("replay_tool", os.path.join(ROOT, "tools", "replay.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_es_text(lib):
    tool = _tool()
    recs, _ = lib.host_es(M.frame_list(K.KNOWN_FRAMES))
    assert [tool.es_text(r) for r in recs] == KNOWN_TEXT
    more = [M.frame(M.me_tc(23, 5)), M.frame(M.me_tc(29, 1)), M.frame(K.TARGET_FULL, df=18, low3=2), M.frame(M.me_tc(18, 3)),
            M.frame(M.me_emergency(state=1, code=7700, x=1)), M.frame(M.me_tc(28, 2, rest=0x2A85 << 34 | 9 << 30 | 1 << 29 | 2 << 26 | 0x2ABCDEF)),
            M.frame(M.me_target(alt=2047, fms=1, heading=None, heading_raw=5, mode_status=1, sil_supp=1)),
            M.frame(M.me_tc(31, 1, rest=3 << 13)), M.frame(M.me_tc(19, 3, rest=1 << 47 | 5 << 43))]
    recs, _ = lib.host_es(M.frame_list(more))
    assert [tool.es_text(r) for r in recs] == [
        "RESERVED tc=23 st=5", "RESERVED tc=29 st=0", "FOREIGN", "POSITION tc=18 nic_b=1",
        "EMERGENCY state=1 squawk=7700", "ACAS_RA ara=2A85 rac=9 rat=1 mte=0 tti=2 tid=2ABCDEF",
        "TARGET_STATE alt=65472ft(fms) nac_p=0 nic_baro=0 sil=0 sil_supp=1 modes=none",
        "OPERATIONAL st=1 v3", "VELOCITY st=3 nac_v=5 intent"]


def test_es_lines(lib):
    """one line per DF17/18 frame, none for the others"""
    tool = _tool()
    msgs = [K.KNOWN_FRAMES[0], M.frame(K.TARGET_FULL, df=20), K.KNOWN_FRAMES[5], M.frame(K.TARGET_FULL, df=11)]
    fr = M.frame_list(msgs)
    fr["offset"] = [2, 4000, 2_000_000, 2_000_240]
    rows = tool.es_lines(fr, lib.host_es(fr)[0]).splitlines()
    assert rows == ["0.000001 DF17 A2C1B6 " + KNOWN_TEXT[0], "1.000000 DF17 484175 " + KNOWN_TEXT[5]]
