"""Wire input, CPU tier: struct sizes, constants and the argument errors of adsb_host_wire_parse (adsb_wire_in_of checks
the same, tests/test_gpu_wire_in.py)."""
import ctypes as C

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib as L
from air_rs_amd import demod as D
from tests import wire_model as W

FRAME = W.encode_one(W.BEAST, 7, W.KNOWN)


def test_struct_sizes_and_constants(lib):
    assert C.sizeof(L.AdsbWireInCfg) == 32 and C.sizeof(L.AdsbWireRx) == 16 and C.sizeof(L.AdsbWireInHeader) == 64
    assert D.WIRE_RX_DTYPE.itemsize == 16 and D.WIRE_IN_HEADER_DTYPE.itemsize == 64
    assert [D.WIRE_RX_DTYPE.fields[k][1] for k in ("ticks", "pos", "signal", "kind", "receiver")] == [0, 8, 12, 13, 14]
    assert (A.ADSB_WIRE_IN_CRC, A.ADSB_WIRE_IN_DF17) == (1, 2)
    header = open(L.LIB_PATH.replace("air_rs_amd/lib/libadsb_hip.so", "include/adsb_hip.h")).read()
    assert "#define ADSB_WIRE_IN_CRC 0x1u" in header and "#define ADSB_WIRE_IN_DF17 0x2u" in header
    assert "#define ADSB_ABI_VERSION 1\n" in header


def _call(cfg, data, ends, n_streams=None, n_bytes=None):
    fn = L.load().adsb_host_wire_parse
    e = None if ends is None else np.array(ends, dtype=np.uint64)
    hdr = L.AdsbWireInHeader()
    return fn(None if cfg is None else C.byref(cfg), data, len(data or b"") if n_bytes is None else n_bytes,
              None if e is None else e.ctypes.data, len(e) if n_streams is None else n_streams, None, None, None, 0, None,
              None, None, C.byref(hdr)), hdr


def test_error_codes(lib):
    ok = L.AdsbWireInCfg(L.ADSB_WIRE_BEAST, 0, 0, 0, 0, 0)
    rc, hdr = _call(ok, FRAME, [23])
    assert rc == A.ADSB_OK and hdr.total_found == 1 and hdr.n_frames == 1
    assert _call(None, FRAME, [23])[0] == A.ADSB_E_ARG
    assert _call(ok, None, [23], n_bytes=23)[0] == A.ADSB_E_ARG
    assert _call(ok, FRAME, None, n_streams=1)[0] == A.ADSB_E_ARG
    assert _call(L.AdsbWireInCfg(3, 0, 0, 0, 0, 0), FRAME, [23])[0] == A.ADSB_E_ARG              # unknown format
    assert _call(L.AdsbWireInCfg(0, 0, 1 << 48, 0, 0, 0), FRAME, [23])[0] == A.ADSB_E_ARG        # tick_bias >= 2^48
    assert _call(L.AdsbWireInCfg(0, 0, (1 << 48) - 1, 0, 0, 0), FRAME, [23])[0] == A.ADSB_OK
    assert _call(L.AdsbWireInCfg(0, 0, 0, 0, 2, 1), FRAME, [23])[0] == A.ADSB_E_ARG              # bad sample_type with levels
    assert _call(L.AdsbWireInCfg(0, 0, 0, 0, -1, 1), FRAME, [23])[0] == A.ADSB_E_ARG
    assert _call(L.AdsbWireInCfg(0, 0, 0, 0, 2, 0), FRAME, [23])[0] == A.ADSB_OK                 # ... ignored without
    assert _call(ok, FRAME, [23], n_streams=0)[0] == A.ADSB_E_ARG
    assert _call(ok, FRAME, [0] * 256 + [23])[0] == A.ADSB_E_ARG                                 # 257 streams
    assert _call(ok, FRAME, [0] * 255 + [23])[0] == A.ADSB_OK
    assert _call(ok, FRAME, [10, 5, 23])[0] == A.ADSB_E_ARG                                      # not ascending
    assert _call(ok, FRAME, [10, 22])[0] == A.ADSB_E_ARG                                         # does not end at n_bytes
    assert _call(ok, FRAME, [10, 24])[0] == A.ADSB_E_ARG
    assert _call(ok, FRAME, [1 << 32], n_bytes=1 << 32)[0] == A.ADSB_E_CAPACITY                  # checked before any read
    rc, hdr = _call(ok, b"", [0])
    assert rc == A.ADSB_OK and hdr.n_marks == 0
    assert _call(ok, None, [0, 0], n_bytes=0)[0] == A.ADSB_OK


def test_wrapper_errors(lib):
    with pytest.raises(A.AdsbError) as e:
        A.host_wire_parse(FRAME, [5])
    assert e.value.code == A.ADSB_E_ARG
    with pytest.raises(A.AdsbError):
        A.host_wire_parse(FRAME, tick_bias=1 << 48)
    with pytest.raises(KeyError):
        A.host_wire_parse(FRAME, format="sbs")
    got = A.host_wire_parse(np.frombuffer(FRAME, dtype=np.uint8), filter=A.ADSB_WIRE_IN_CRC | A.ADSB_WIRE_IN_DF17)
    assert len(got.frames) == 1 and got.levels is None and isinstance(got, A.WireIn)
