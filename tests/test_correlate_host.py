"""adsb_host_correlate, the CPU mirror of the device's correlate, against the independent model
(tests/correlate_model.py), byte for byte, on the edge lists of tests/correlate_cases.py; and the properties the
definitions promise, checked on the model's own output (CPU tier)."""
import numpy as np
import pytest

from tests import correlate_cases as K
from tests import correlate_model as M

CASES = K.all_cases()


@pytest.fixture(scope="module")
def wants():
    """The model's result per case, computed once."""
    return {name: M.correlate(fr, counts, w, base, lv) for name, fr, counts, w, base, lv in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_mirror_equals_model(lib, wants, case):
    name, fr, counts, w, base, lv = case
    M.same(lib.host_correlate(fr, counts, w, base, lv), wants[name], name)


def test_model_is_what_the_definitions_say(wants):
    """The expectations the issue spells out, on the model's own output: a wrong model would pass the comparisons."""
    by = wants
    m, _, r = by["chain gaps w=7"]
    assert m["n_receptions"].tolist() == [3, 2, 1, 2] and m["span"].tolist() == [14, 7, 0, 7]
    assert by["chain gaps w=0"][0]["n_receptions"].tolist() == [3, 2, 1, 2]
    assert by["chain gaps w=0"][0]["span"].tolist() == [0, 0, 0, 0]
    assert by["chain gaps w=4294967295"][0]["n_receptions"].tolist() == [3, 2, 1, 2]
    m = by["long chain"][0]
    assert len(m) == 1 and m["n_receptions"][0] == 120 and m["span"][0] == 119 * 5 and m["n_receivers"][0] == 3
    assert len(by["no chain"][0]) == 120
    m = by["key width"][0]
    assert len(m) == 16 and (m["n_receptions"] == 3).all() and (m["time"] == 500).all()
    keys = [bytes(b) for b in m["bytes"]]
    assert keys == sorted(keys) and keys[0] == bytes(14) and keys[-1] == bytes([0xFF] * 14)   # unsigned, all bytes
    m = by["256 receivers"][0]
    assert len(m) == 1 and m["n_receivers"][0] == 256 == m["n_receptions"][0]
    m = by["one receiver twice"][0]
    assert m["n_receptions"].tolist() == [3, 1] and m["n_receivers"].tolist() == [2, 1]
    m, _, r = by["equal T"]
    assert len(m) == 1 and m["first_receiver"][0] == 0 and m["fixed_bit"][0] == 0 and r["frame"].tolist() == [0, 1, 2, 3]
    m = by["status and levels"][0]
    assert m["status"].tolist() == [1, 0, 0, 0] and m["fixed_bit"].tolist() == [11, 0xFF, 0xFF, 0xFF]
    assert m["n_clean"].tolist() == [0, 2, 1, 2]
    assert m["best_receiver"].tolist() == [0, 1, 0xFFFF, 0] and m["best_signal_sum"].tolist() == [700, 100, 0, 0]
    assert (by["status, no levels"][0]["best_receiver"] == 0xFFFF).all()
    m = by["time width w=2"][0]
    assert (m["time"] > (1 << 63)).sum() >= 2 and ((m["time"] > (1 << 32)) & (m["time"] < (1 << 63))).sum() >= 2


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_result_invariants(wants, case):
    """Every list: messages ascending in (time, K) and unique in it, receptions a permutation owned message by message
    in (T, j) order, frames the messages' first 24 bytes."""
    name, fr, counts, w, base, lv = case
    msgs, fout, recs = wants[name]
    assert sorted(recs["frame"].tolist()) == list(range(len(fr)))
    order = [(int(t), bytes(b)) for t, b in zip(msgs["time"], msgs["bytes"])]
    assert order == sorted(order) and len(set(order)) == len(order)
    assert fout.tobytes() == b"".join(m.tobytes()[:24] for m in msgs)
    at = 0
    for m in msgs:
        assert m["first"] == at
        mine = recs[at:at + int(m["n_receptions"])]
        at += int(m["n_receptions"])
        assert [(int(t), int(j)) for t, j in zip(mine["time"], mine["frame"])] == \
            sorted((int(t), int(j)) for t, j in zip(mine["time"], mine["frame"]))
        assert mine["time"][0] == m["time"] and mine["time"][-1] - mine["time"][0] == m["span"]
        assert len(set(mine["receiver"].tolist())) == m["n_receivers"] and mine["receiver"][0] == m["first_receiver"]
        assert all(bytes(fr["bytes"][j]) == bytes(m["bytes"]) for j in mine["frame"])
    assert at == len(fr)
