"""The synthetic source against its NumPy model (tests/synth_model.py), on the CPU: adsb_synth_fill_host and
adsb_synth_slot == the model, for every configuration, start and channel the GPU tier (tests/test_gpu_synth.py) runs, and
each configuration shown -- on the model's output alone -- to reach what it is named for.  All comparisons are ==."""
import numpy as np
import pytest

import air_rs_amd as A
from tests import synth_model as M

TYPES = {"i8": A.ADSB_SAMPLE_I8, "i16": A.ADSB_SAMPLE_I16}
assert (M.I8, M.I16) == (A.ADSB_SAMPLE_I8, A.ADSB_SAMPLE_I16)


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (bad.size, bad[:5], got[bad[:3]], want[bad[:3]])


@pytest.fixture(scope="module")
def filled(lib):
    """name, type -> (cfg, model fill of the configuration's whole length), computed once."""
    return {(name, t): (A.synth_default(**over), M.reference(name, st))
            for name, (over, n) in M.CONFIGS.items() for t, st in TYPES.items()}


def test_model_defaults_are_the_librarys(lib):
    cfg = A.synth_default()
    assert {k: getattr(cfg, k) for k in M.DEFAULT} == M.DEFAULT and cfg.reserved == 0


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("name", M.CONFIGS)
def test_host_fill_equals_model(filled, name, t):
    cfg, want = filled[name, t]
    _same(A.synth_fill_host(cfg, TYPES[t], 0, 0, len(want)), want)


@pytest.mark.parametrize("t", TYPES)
def test_host_fill_equals_model_at_every_start_and_channel(lib, t):
    cfg = A.synth_default(seed=31, slot_len=700)
    for first in M.FIRSTS:
        for ch in M.CHANNELS:
            _same(A.synth_fill_host(cfg, TYPES[t], ch, first, 2000), M.fill(cfg, TYPES[t], ch, first, 2000))
    for n in (0, 1, 255, 256, 257):
        _same(A.synth_fill_host(cfg, TYPES[t], 3, 123457, n), M.fill(cfg, TYPES[t], 3, 123457, n))


@pytest.mark.parametrize("name", M.CONFIGS)
def test_slot_equals_model(lib, name):
    cfg = A.synth_default(**M.CONFIGS[name][0])
    numbers = np.array(list(range(2000)) + list(range(2**32 - 5, 2**32 + 5)) + [2**40, 2**63 // cfg.slot_len], dtype=np.uint64)
    for ch in (0, 2**32 - 1):
        t = M.slots(cfg, ch, numbers)
        for i, s in enumerate(numbers):
            got = A.synth_slot(cfg, ch, int(s))
            assert got == (bool(t["present"][i]), int(t["start"][i]), bytes(t["clean"][i]), bytes(t["sent"][i]),
                           int(t["kind"][i])), (name, ch, int(s))
    assert M.slot(cfg, 7, 12345) == A.synth_slot(cfg, 7, 12345)


def test_model_building_blocks(oracle):
    """The pieces against values that do not come from the generator: splitmix64's published first outputs for seed 0
    (mix64(0) is the first, mix64(golden-ratio increment) the second), the oracle's CRC, the pulse positions of the
    reference's gate (preamble 0, 2, 7, 9) and C's division."""
    assert int(M.mix64(0)[0]) == 0xE220A8397B1DCDAF
    assert int(M.mix64(0x9E3779B97F4A7C15)[0]) == 0x6E789E6AA1B965F4
    t = M.slots(A.synth_default(), 0, np.arange(50))
    for row in t["clean"]:
        assert oracle.get_adsb_crc(row[:11]) == int.from_bytes(bytes(row[11:]), "big")
    on = M.pulse_at(np.array([[0x80] + [0] * 12 + [0x01]], dtype=np.uint8))[0]
    assert list(np.nonzero(on[:16])[0]) == [0, 2, 7, 9]
    assert (on[16], on[17], on[18], on[19]) == (1, 0, 0, 1) and (on[238], on[239]) == (1, 0) and on.sum() == 4 + 112
    cfg = A.synth_default(noise_div=7)
    raw = M.noise(A.synth_default(noise_div=1), 0, np.arange(5000))
    assert (M.noise(cfg, 0, np.arange(5000)) == np.trunc(raw / 7.0)).all() and (raw < 0).any() and (raw % 7 != 0).any()


# ---- every configuration reaches what it is named for (the model's output only) ------------------------------------
def _table(name):
    over, n = M.CONFIGS[name]
    cfg = A.synth_default(**over)
    return cfg, n, M.slots(cfg, 0, np.arange(-(-n // cfg.slot_len)))


def test_cases_reach_their_edges(filled):
    for name, (over, n) in M.CONFIGS.items():
        cfg = filled[name, "i8"][0]
        assert n >= 40 * cfg.slot_len, name
    # clipping: i8 both ways at noise_div 1; i16 both ways at amp_shift 7, not at 0
    for name in ("noise1", "shift0noise1", "shift7noise1"):
        v = filled[name, "i8"][1]
        assert v.min() == -128 and v.max() == 127, name
    v = filled["shift7noise1", "i16"][1]
    assert v.min() == -32768 and v.max() == 32767
    v = filled["shift0noise1", "i16"][1]
    assert -32768 < v.min() < -128 and 127 < v.max() < 32767     # past the i8 range, unclipped
    assert (filled["default", "i16"][1] == filled["default", "i8"][1]).all()      # amp_shift 0, nothing clips
    cfg, v = filled["noise255", "i8"]
    quiet = M.noise(cfg, 0, np.arange(len(v)))
    assert set(np.unique(quiet)) <= {-2, -1, 0, 1, 2} and (quiet == 0).mean() > 0.8 and (quiet < 0).any()
    # kinds
    for name in ("kinds", "mix20_10_10"):
        cfg, n, t = _table(name)
        assert set(t["kind"][t["present"]]) == {0, 1, 2, 3}, name
    for name, k in (("mix100_0_0", 1), ("mix0_100_0", 2), ("mix0_0_100", 3)):
        cfg, n, t = _table(name)
        assert (t["kind"] == k).all(), name
        diff = np.unpackbits(t["clean"] ^ t["sent"], axis=1)
        assert (diff.sum(axis=1) == (2 if k == 3 else 1)).all()
        assert (diff[:, 88:].sum(axis=1) == (1 if k == 2 else 0)).all()
    # jitter: a frame as late as the rule allows (jitter == slot_len - 241), and one that starts the slot (both present).
    # jitter is taken mod slot_len - 240, so the latest frame's 240th sample is the slot's LAST BUT ONE: no frame of any
    # config reaches a slot's last sample, and none leaves its slot.
    cfg, n, t = _table("slot256")
    j = t["jitter"][t["present"]]
    assert cfg.slot_len - 241 == 15 and j.max() == 15 and j.min() == 0 and set(j) == set(range(16))
    ends = (t["start"][t["present"]] + np.uint64(239)) % np.uint64(cfg.slot_len)
    assert (ends == cfg.slot_len - 2).any() and ends.max() == cfg.slot_len - 2
    on, row, _ = M.pulses(cfg, 0, 0, n)
    last_of_slot = np.arange(cfg.slot_len - 1, n, cfg.slot_len)
    assert on[last_of_slot - 1].any() and not on[last_of_slot].any()      # (a frame's 240th position holds a pulse for a 0 bit)
    cfg, n, t = _table("slot100003")
    assert t["jitter"].max() > 65536 and t["present"].all()
    # frame_pct
    cfg, n, t = _table("pct0")
    assert not t["present"].any() and not M.pulses(cfg, 0, 0, n)[0].any()
    assert (filled["pct0", "i8"][1] == np.clip(M.noise(cfg, 0, np.arange(n)), -128, 127)).all()
    cfg, n, t = _table("pct100")
    assert t["present"].all() and M.pulses(cfg, 0, 0, n)[0].sum() == 116 * len(t["present"])
    cfg, n, t = _table("pct50")
    assert t["present"].any() and not t["present"].all()
    # every amplitude pair, every type-code range
    cfg, n, t = _table("kinds")
    assert len({tuple(a) for a in t["amp"]}) == 8
    tcs = set(t["clean"][:, 4] >> 3)
    assert tcs & set(range(1, 5)) and tcs & set(range(9, 19)) and tcs & set(range(19, 29)) and tcs <= set(range(1, 29)) - {5, 6, 7, 8}


def test_planted_frames_are_what_the_demodulator_finds(oracle):
    """The model's stream is the one DESIGN.md describes: the oracle finds the clean frame of every slot of kind 0 and 1
    (one flipped data bit is repaired) at the slot's start, at a noise level where nothing is lost."""
    cfg = A.synth_default(seed=41, slot_len=600, noise_div=60)
    n = 200 * 600
    t = M.slots(cfg, 0, np.arange(200))
    rc, frames, found = oracle.process_buffer(M.fill(cfg, M.I8, 0, 0, n))
    assert rc == 0
    by_offset = {int(f["offset"]): bytes(f["bytes"]) for f in frames}
    keep = t["present"] & (t["kind"] <= 1)
    assert keep.sum() > 150
    for start, clean in zip(t["start"][keep], t["clean"][keep]):
        assert by_offset.get(int(start)) == bytes(clean), int(start)


def test_rejected_configs_host(lib):
    import ctypes as C
    for over in M.REJECTED:
        cfg = A.synth_default(**over)
        buf = np.full((64, 2), 0x5A, dtype=np.int8)
        rc = A.load().adsb_synth_fill_host(C.byref(cfg), A.ADSB_SAMPLE_I8, 0, 0, 64, buf.ctypes.data)
        assert rc == A.ADSB_E_ARG and (buf == 0x5A).all(), over
