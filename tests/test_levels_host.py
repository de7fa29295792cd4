"""Per-frame signal and noise power, CPU tier: the 32-byte adsb_frame_level layout, the CPU mirror
(adsb_host_frame_levels) against fixed values of the committed fixtures and against the NumPy model
(tests/levels_model.py), adsb_level_dbfs, and the argument checks of the device entry points that need no device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import levels_cases as K
from tests import levels_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adsb_levels_device_async", "adsb_fetch_levels", "adsb_levels_device", "adsb_levels_of")
NEW_HOST = ("adsb_host_frame_levels", "adsb_level_dbfs")


def _same(got, want):
    assert got.dtype.itemsize == want.dtype.itemsize == 32 and len(got) == len(want), (len(got), len(want))
    bad = [k for k in range(len(got)) if got[k].tobytes() != want[k].tobytes()]
    assert not bad, (bad[:5], got[bad[:3]], want[bad[:3]])


def test_level_struct_layout(lib):
    from air_rs_amd import _lib
    assert C.sizeof(_lib.AdsbFrameLevel) == 32 and lib.LEVEL_DTYPE.itemsize == 32
    assert list(levels_model.OFFSETS.values()) == [0, 8, 16, 20, 24, 28, 30]
    for name, off in levels_model.OFFSETS.items():
        assert getattr(_lib.AdsbFrameLevel, name).offset == off, name
        assert lib.LEVEL_DTYPE.fields[name][1] == off, name
    assert lib.LEVEL_DTYPE == levels_model.MODEL_DTYPE
    assert lib.ADSB_LEVEL_VALID == 1 and (lib.LEVEL_PULSE_SAMPLES, lib.LEVEL_QUIET_SAMPLES) == (116, 124)


def test_level_declarations(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    hip = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    host = open(os.path.join(ROOT, "include", "adsb_host.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hip), name
    for name in NEW_HOST:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
        assert re.search(r"\b(int|double)\s+" + name + r"\s*\(", host), name
    assert re.search(r"#define ADSB_LEVEL_VALID\s+0x1u", hip)
    for method in ("levels", "levels_async", "levels_of", "levels_device"):
        assert callable(getattr(lib.AdsbDemod, method, None)), method


def test_mirror_fixed_values_ref_frames(lib):
    iq, fr = K.fixture("ref_frames_i8")
    lv = lib.host_frame_levels(iq, fr)
    assert len(lv) == 7 and (lv["flags"] == lib.ADSB_LEVEL_VALID).all()
    assert (lv["signal_sum"] == 986000).all()                    # 116 pulses of (90, 20): 116 x 8500
    assert (lv["peak"] == 8500).all() and (lv["pulse_min"] == 8500).all()
    assert (lv["quiet_max"] == 18).all() and (lv["weak_bits"] == 0).all()   # the floor is +-3: at most 9 + 9
    _same(lv, levels_model.levels(iq, fr))
    iq, fr = K.fixture("ref_frames_i16")
    lv = lib.host_frame_levels(iq, fr)
    assert len(lv) == 7 and (lv["signal_sum"] == 9860000000).all() and 9860000000 > 1 << 32   # the sum is 64 bits wide
    assert (lv["peak"] == 85000000).all() and (lv["pulse_min"] == 85000000).all() and (lv["weak_bits"] == 0).all()
    _same(lv, levels_model.levels(iq, fr))


def test_mirror_fixed_values_repaired_bit_and_shortest_buffer(lib):
    iq, fr = K.fixture("bit_errors_i8")
    assert len(fr) == 1 and fr[0]["status"] == 1 and fr[0]["fixed_bit"] == 43
    lv = lib.host_frame_levels(iq, fr)
    # the repaired bit's pulse sample, by the bytes AS RETURNED, is the floor sample the flipped bit left there
    assert (lv[0]["weak_bits"], lv[0]["pulse_min"], lv[0]["signal_sum"]) == (1, 5, 1127005)
    _same(lv, levels_model.levels(iq, fr))
    iq, fr = K.fixture("len241_i8")
    assert len(iq) == 241 and len(fr) == 1 and fr[0]["offset"] == 0
    lv = lib.host_frame_levels(iq, fr)
    assert lv[0]["signal_sum"] == 417600 and lv[0]["flags"] == 1  # 116 x 3600
    _same(lv, levels_model.levels(iq, fr))


def test_mirror_neighbouring_offsets_of_both_parities(lib):
    iq, fr = K.fixture("sqrt_ties_i8")
    assert len(fr) == 6 and set(int(o) % 2 for o in fr["offset"]) == {0, 1}
    assert np.abs(np.diff(fr["offset"].astype(np.int64))).min() == 1
    _same(lib.host_frame_levels(iq, fr), levels_model.levels(iq, fr))


@pytest.mark.parametrize("st", ["i8", "i16"])
def test_mirror_against_model_synthetic(lib, oracle, st):
    sample_type, dt = (lib.ADSB_SAMPLE_I8, np.int8) if st == "i8" else (lib.ADSB_SAMPLE_I16, np.int16)
    cfg = lib.synth_default(seed=0xC0FFEE, slot_len=1900)
    iq = lib.synth_fill_host(cfg, sample_type, 0, 0, 6000)
    assert iq.dtype == dt
    if st == "i8":
        want_iq, fr = K.fixture("synth_i8")                       # the committed fixture is this very buffer
        assert (iq == want_iq).all()
    else:
        rc, fr, n = oracle.process_buffer(iq)
        assert rc == 0
        fr = fr.astype(K.FRAME_DTYPE)
    assert len(fr) >= 2
    lv = lib.host_frame_levels(iq, fr)
    assert (lv["flags"] == 1).all() and (lv["signal_sum"] > lv["noise_sum"]).all()
    _same(lv, levels_model.levels(iq, fr))
    # the same frames as a slice of a longer stream
    _same(lib.host_frame_levels(iq[100:], _shift(fr, 10_000), first_sample=10_100),
          levels_model.levels(iq[100:], _shift(fr, 10_000), first_sample=10_100))


def _shift(fr, by):
    out = fr.copy()
    out["offset"] += np.uint64(by)
    return out


@pytest.mark.parametrize("dt", [np.int8, np.int16], ids=["i8", "i16"])
def test_mirror_full_scale(lib, dt):
    iq, fr, full = K.full_scale(dt)
    assert full == (32768 if dt == np.int8 else 1 << 31)
    lv = lib.host_frame_levels(iq, fr)
    assert (lv["peak"] == full).all() and (lv["pulse_min"] == full).all() and (lv["flags"] == 1).all()
    assert (lv["signal_sum"] == 116 * full).all() and (lv["quiet_max"] <= 18).all() and (lv["weak_bits"] == 0).all()
    _same(lv, levels_model.levels(iq, fr))


@pytest.mark.parametrize("dt", [np.int8, np.int16], ids=["i8", "i16"])
def test_mirror_invalid_frames_get_zeros(lib, dt):
    iq, fr, valid = K.invalid_list(dt)
    lv = lib.host_frame_levels(iq, fr, first_sample=K.INVALID_FIRST)
    assert (lv["flags"] == valid.astype(np.uint16)).all()
    zero = np.zeros((), dtype=lib.LEVEL_DTYPE).tobytes()
    assert all(lv[k].tobytes() == zero for k in np.nonzero(~valid)[0])
    assert (lv["signal_sum"][valid] > 0).all()
    _same(lv, levels_model.levels(iq, fr, first_sample=K.INVALID_FIRST))
    # 239 samples hold no window at all
    short = lib.host_frame_levels(iq[:239], K.frame_list([0, 1, 5000]), first_sample=0)
    assert all(r.tobytes() == zero for r in short)
    _same(short, levels_model.levels(iq[:239], K.frame_list([0, 1, 5000])))
    assert len(lib.host_frame_levels(iq, fr[:0])) == 0


def test_level_dbfs(lib):
    I8, I16 = lib.ADSB_SAMPLE_I8, lib.ADSB_SAMPLE_I16
    for n in (1, 116, 124, 240):
        assert lib.level_dbfs(I8, n * 32768, n) == 0.0
        assert lib.level_dbfs(I16, n << 31, n) == 0.0
    assert lib.level_dbfs(I8, 0, 116) == -math.inf and lib.level_dbfs(I16, 0, 124) == -math.inf
    assert math.isnan(lib.level_dbfs(2, 100, 116)) and math.isnan(lib.level_dbfs(-1, 100, 116))
    assert math.isnan(lib.level_dbfs(I8, 100, 0)) and math.isnan(lib.level_dbfs(I16, 0, 0))
    assert lib.level_dbfs(I8, 986000, 116) == pytest.approx(10 * math.log10(8500 / 32768), abs=1e-12)
    assert lib.level_dbfs(I16, 116 << 21, 116) == pytest.approx(-10 * math.log10(1024), abs=1e-12)


def test_mirror_bad_arguments(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    iq = np.zeros((300, 2), dtype=np.int8)
    fr = K.frame_list([0])
    out = (_lib.AdsbFrameLevel * 1)()
    out[0].peak = 77
    assert L.adsb_host_frame_levels(lib.ADSB_SAMPLE_I8, None, 300, 0, fr.ctypes.data, 1, out) == lib.ADSB_E_ARG
    assert L.adsb_host_frame_levels(lib.ADSB_SAMPLE_I8, iq.ctypes.data, 300, 0, None, 1, out) == lib.ADSB_E_ARG
    assert L.adsb_host_frame_levels(lib.ADSB_SAMPLE_I8, iq.ctypes.data, 300, 0, fr.ctypes.data, 1, None) == lib.ADSB_E_ARG
    assert L.adsb_host_frame_levels(2, iq.ctypes.data, 300, 0, fr.ctypes.data, 1, out) == lib.ADSB_E_ARG
    assert out[0].peak == 77                                      # untouched by a rejected call
    assert L.adsb_host_frame_levels(lib.ADSB_SAMPLE_I8, iq.ctypes.data, 300, 0, None, 0, None) == lib.ADSB_OK
    with pytest.raises(TypeError):
        lib.host_frame_levels(np.zeros((300, 2), dtype=np.float32), fr)


def test_device_entry_points_bad_arguments(lib):
    """What the device entry points reject before they touch a device (a context cannot exist without one)."""
    from air_rs_amd import _lib
    L = _lib.load()
    n = C.c_size_t(123)
    out = (_lib.AdsbFrameLevel * 2)()
    dev = C.c_void_p()
    fr = K.frame_list([0, 1])
    assert L.adsb_levels_device_async(None) == lib.ADSB_E_ARG
    assert L.adsb_fetch_levels(None, out, 2, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_fetch_levels(None, None, 0, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_levels_device(None, C.byref(dev)) == lib.ADSB_E_ARG
    assert L.adsb_levels_of(None, 4096, 1000, 0, fr.ctypes.data, 2, out) == lib.ADSB_E_ARG
    assert L.adsb_levels_of(None, None, 0, 0, None, 0, None) == lib.ADSB_E_ARG
    assert n.value == 123 and dev.value is None
