"""tools/replay.py --commb, CPU tier: the text one COMMB_DTYPE record adds to a DF20/21 line (commb_text), on the
mirror's records of the known answers and of the ambiguous cases.  The command itself needs a device
(tests/test_gpu_commb.py starts it)."""
import importlib.util
import os

from tests import commb_cases as K
from tests import commb_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOWN_TEXT = ["BDS4,0 mcp=3008ft fms=3008ft baro=1020.0mb",
              "BDS5,0 roll=2.11 track=114.26 gs=438kt rate=0.125 tas=424kt",
              "BDS6,0 hdg=42.71 ias=252kt mach=0.420 baro=-1920ft/min inertial=-1920ft/min",
              "BDS1,7 0,5 0,6 0,7 0,8 0,9 2,0 4,0 5,0 5,1 5,2 6,0",
              "BDS1,0 version=0 ovc=0",
              "BDS2,0"]


def _tool():
    spec = importlib.util.spec_from_file_location("replay_tool", os.path.join(ROOT, "tools", "replay.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_commb_text(lib):
    tool = _tool()
    recs, _ = lib.host_commb(M.frame_list(K.KNOWN_FRAMES))
    assert [tool.commb_text(r) for r in recs] == KNOWN_TEXT
    name, fr, claim = K.ambiguous()
    recs, _ = lib.host_commb(fr)
    texts = [tool.commb_text(r) for r in recs]
    assert texts[0] == "?4,0|5,0|6,0" and texts[2] == "?5,0|6,0" and texts[-1] == "?1,7|4,0"
    assert all(t[0] == "?" and t.count("|") == int(r["n_candidates"]) - 1 for t, r in zip(texts, recs))
    recs, _ = lib.host_commb(M.frame_list([M.frame(bytes(7)), M.frame(b"\xff" * 7), M.frame(M.mb_40(modes=5, source=2)),
                                           M.frame(M.mb_30(ara=0x2A85, rac=9, rat_mte=1, tti=1, tid=0x2ABCDEF))]))
    assert [tool.commb_text(r) for r in recs] == ["-", "-", "BDS4,0 mode=5 source=2",
                                                  "BDS3,0 ara=2A85 rac=9 rat_mte=1 tti=1 tid=2ABCDEF"]
