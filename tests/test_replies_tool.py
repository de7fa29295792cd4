"""tools/replay.py --replies, CPU tier: the lines of a merged list (replies_lines) and, behind them, --modes' lines on the
mirror's records of the same list.  The command itself needs a device (tests/test_gpu_replies.py starts it)."""
import importlib.util
import os

import numpy as np

from tests import modes_model as MM
from tests import replies_cases as K
from tests import replies_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("replay_tool", os.path.join(ROOT, "tools", "replay.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def capture():
    """an i8 capture with a DF11, a DF4 and a DF20 of one aircraft and a DF17 of another -> (iq, the four messages)"""
    iq = M.noise(6000, np.int8, 1, K.LOW)
    msgs = [MM.all_call(0x4B1A2C), MM.reply(4, 0x4B1A2C, field=0x1838), MM.squitter(0xA05629, me=bytes([0x58, 1, 2, 3, 4, 5, 6])),
            MM.reply(20, 0x4B1A2C, field=0x1838, rest=MM.callsign_mb("SWR123__"))]
    for k, m in enumerate(msgs):
        M.render(iq, m, 100 + 1000 * k)
    return iq, msgs


def test_replies_lines(lib):
    tool = _tool()
    iq, msgs = capture()
    replies, counts, _ = lib.host_replies(iq)
    squitters = MM.frame_list([msgs[2]], offsets=[2100])
    frames, src, _ = lib.host_merge_lists(squitters, [1], replies, counts)
    rows = tool.replies_lines(frames, src).splitlines()
    want = [f"0.000050 100 replies DF11 {msgs[0].hex().upper()}", f"0.000550 1100 replies DF4 {msgs[1].hex().upper()}",
            f"0.001050 2100 demod DF17 {msgs[2].hex().upper()}", f"0.001550 3100 replies DF20 {msgs[3].hex().upper()}"]
    assert [r for r in rows if r.split()[1] in ("100", "1100", "2100", "3100")] == want
    assert all(len(r.split()[4]) == (14 if int(r.split()[3][2:]) < 16 else 28) for r in rows)
    assert tool.replies_lines(frames[:0], src[:0]) == ""


def test_modes_lines_of_the_merged_list(lib):
    """the DF11 teaches the address, the replies behind it are KNOWN, the squitter is another aircraft's"""
    tool = _tool()
    iq, msgs = capture()
    replies, counts, _ = lib.host_replies(iq)
    frames, src, _ = lib.host_merge_lists(MM.frame_list([msgs[2]], offsets=[2100]), [1], replies, counts)
    keep = np.isin(frames["offset"], [100, 1100, 2100, 3100])
    rows = tool.modes_lines(frames[keep], lib.host_modes(frames[keep])[0]).splitlines()
    assert rows == ["0.000050 DF11 SELF 4B1A2C - - -", "0.000550 DF4 KNOWN 4B1A2C 38000 - -", "0.001050 DF17 SELF A05629 - - -",
                    "0.001550 DF20 KNOWN 4B1A2C 38000 - SWR123"]
