"""Clock sync's argument checks and record layouts on the CPU tier: what adsb_host_clock_sync and adsb_host_clock_apply
refuse (the device entry points share the checks' text), the sizes and offsets of the public records, and the exports."""
import ctypes as C

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from tests import clock_cases as CC
from tests import clock_model as CM


@pytest.fixture(scope="module")
def small(oracle):
    return CC.scenario(oracle, 4, 6, seed=5, p_heard=1.0)


def _sync(sc, cfg, receivers=None, n_receivers=None, lst=None, clocks=True, rx=True):
    lst = lst or sc["lst"]
    rcv = sc["rcv"] if receivers is None else receivers
    out = np.zeros(256, dtype=A.CLOCK_DTYPE)
    return _lib.load().adsb_host_clock_sync(
        C.byref(cfg) if cfg is not None else None, rcv.ctypes.data, len(rcv) if n_receivers is None else n_receivers,
        lst["msgs"].ctypes.data, len(lst["msgs"]), lst["recs"].ctypes.data, len(lst["recs"]),
        lst["rx"].ctypes.data if rx else None, len(lst["rx"]) if rx else 0, out.ctypes.data if clocks else None, None, None)


def test_records(lib):
    assert C.sizeof(_lib.AdsbClockCfg) == 64 and C.sizeof(_lib.AdsbClockHeader) == 64 and A.CLOCK_DTYPE.itemsize == 64
    assert A.CLOCK_DTYPE.fields["residual_rms_s"][1] == 24 and A.CLOCK_DTYPE.fields["flags"][1] == 40
    assert _lib.AdsbClockCfg.seconds_per_tick.offset == 16 and _lib.AdsbClockCfg.max_range_nm.offset == 40
    assert A.CLOCK_DTYPE == CM.CLOCK_DTYPE
    assert (A.ADSB_CLOCK_REFERENCE, A.ADSB_CLOCK_REACHED, A.ADSB_CLOCK_HAS_DRIFT) == (CM.REFERENCE, CM.REACHED, CM.HAS_DRIFT)
    assert (A.ADSB_CLOCK_HDR_BAD_INDEX, A.ADSB_CLOCK_HDR_DRIFT_DROPPED, A.ADSB_CLOCK_HDR_SINGULAR) == \
        (CM.HDR_BAD_INDEX, CM.HDR_DRIFT_DROPPED, CM.HDR_SINGULAR)
    per, parts = C.c_uint32(), C.c_uint32()
    assert _lib.load().adsb_debug_clock_geometry(C.byref(per), C.byref(parts)) == A.ADSB_OK
    assert (per.value, parts.value) == (16, 64)


def test_accepted(lib, small):
    assert _sync(small, A.demod._clock_cfg(**small["cfg"])) == A.ADSB_OK
    cfg = dict(small["cfg"], reference=3, min_rows=2, max_residual_s=1e-6, max_range_nm=180.0, drift=False)
    assert _sync(small, A.demod._clock_cfg(**cfg)) == A.ADSB_OK
    # RECEPTION: seconds_per_time = 0 means seconds_per_tick
    assert _sync(small, A.demod._clock_cfg(time_source="reception", seconds_per_tick=CC.SPT_12MHZ), rx=False) == A.ADSB_OK


@pytest.mark.parametrize("bad", [dict(reference=4), dict(seconds_per_time=0.0), dict(seconds_per_time=-1e-6),
                                 dict(seconds_per_time=float("nan")), dict(seconds_per_tick=-1.0),
                                 dict(seconds_per_tick=float("inf")), dict(seconds_per_tick=2.0), dict(max_residual_s=-1e-9),
                                 dict(max_residual_s=float("nan")), dict(max_range_nm=-1.0), dict(max_range_nm=181.0),
                                 dict(max_range_nm=float("inf")), dict(time_source=2),
                                 dict(time_source="reception", seconds_per_tick=0.0)])
def test_cfg_values(lib, small, bad):
    assert _sync(small, A.demod._clock_cfg(**dict(small["cfg"], **bad))) == A.ADSB_E_ARG


def test_other_arguments(lib, small):
    cfg = A.demod._clock_cfg(**small["cfg"])
    assert _sync(small, None) == A.ADSB_E_ARG
    assert _sync(small, cfg, n_receivers=0) == A.ADSB_E_ARG
    assert _sync(small, cfg, n_receivers=257) == A.ADSB_E_ARG
    assert _sync(small, cfg, clocks=False) == A.ADSB_E_ARG
    assert _sync(small, cfg, rx=False) == A.ADSB_E_ARG                    # TICKS without rx
    flagged = A.demod._clock_cfg(**small["cfg"])
    flagged.flags = A.ADSB_CLOCK_DRIFT | 2
    assert _sync(small, flagged) == A.ADSB_E_ARG                          # an unknown flag
    for field, value in (("latitude", 91.0), ("longitude", -181.0), ("height_m", 1e6), ("clock_offset_s", 2e6),
                         ("clock_offset_s", float("nan"))):
        rcv = small["rcv"].copy()
        rcv[field][2] = value
        assert _sync(small, cfg, receivers=rcv) == A.ADSB_E_ARG, field
    L = _lib.load()
    lst = small["lst"]
    assert L.adsb_host_clock_sync(C.byref(cfg), small["rcv"].ctypes.data, 4, None, 3, lst["recs"].ctypes.data, len(lst["recs"]),
                                  lst["rx"].ctypes.data, len(lst["rx"]), np.zeros(4, dtype=A.CLOCK_DTYPE).ctypes.data, None,
                                  None) == A.ADSB_E_ARG                    # NULL msgs with a count
    assert L.adsb_host_clock_sync(C.byref(cfg), small["rcv"].ctypes.data, 4, lst["msgs"].ctypes.data, 1 << 32, None, 0,
                                  lst["rx"].ctypes.data, len(lst["rx"]), np.zeros(4, dtype=A.CLOCK_DTYPE).ctypes.data, None,
                                  None) == A.ADSB_E_CAPACITY


def test_apply_arguments(lib, small):
    lst, L = small["lst"], _lib.load()
    cfg = A.demod._clock_cfg(**small["cfg"])
    clocks, _ = A.host_clock_sync(small["rcv"], lst["msgs"], lst["recs"], lst["rx"], **small["cfg"])
    out = np.zeros(len(lst["recs"]), dtype=A.RECEPTION_DTYPE)

    def apply(cfg=cfg, clocks=clocks.ctypes.data, n=4, corrected=out.ctypes.data):
        return L.adsb_host_clock_apply(C.byref(cfg) if cfg is not None else None, clocks, n, lst["msgs"].ctypes.data,
                                       len(lst["msgs"]), lst["recs"].ctypes.data, len(lst["recs"]), lst["rx"].ctypes.data,
                                       len(lst["rx"]), corrected)
    assert apply() == A.ADSB_OK and (out["receiver"] == lst["recs"]["receiver"]).all()
    assert apply(cfg=None) == A.ADSB_E_ARG and apply(clocks=None) == A.ADSB_E_ARG and apply(corrected=None) == A.ADSB_E_ARG
    assert apply(n=0) == A.ADSB_E_ARG
    bad = A.demod._clock_cfg(**dict(small["cfg"], seconds_per_time=0.0))
    assert apply(cfg=bad) == A.ADSB_E_ARG
