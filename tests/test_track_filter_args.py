"""Every argument error of the filter reserve's entry points that needs no device: NULL handles, a cfg the reserve
refuses (checked BEFORE the table is touched: the handle here is no table at all), and the CPU mirror's own checks.  The
ADSB_E_STATE paths need a table and are in tests/test_gpu_track_filter.py."""
import ctypes as C
import math

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib as L
from air_rs_amd import demod as D
from tests import track_filter_model as M

BAD = [dict(accel_h=-1.0), dict(accel_v=math.nan), dict(range_sigma_m=math.inf), dict(altitude_sigma_m=-0.5),
       dict(gate=-4.0), dict(reset_gap_s=-math.inf), dict(init_speed_sigma_h=math.nan), dict(init_speed_sigma_v=-30.0),
       dict(max_hdop=math.inf), dict(max_vdop=-1e-300)]


def _cfg(reserved=0, **kw):
    c = D._filter_cfg(**kw)
    c.reserved = reserved
    return c


def test_null_table():
    lib = L.load()
    n = C.c_size_t()
    rec, fr, op = (np.zeros(1, dtype=d) for d in (A.AIRCRAFT_FILTER_DTYPE, A.FRAME_FILTER_DTYPE, A.FILTER_OPERAND_DTYPE))
    assert lib.adsb_track_table_filter_reserve(None, None) == A.ADSB_E_ARG
    assert lib.adsb_track_table_filter_reserve(None, C.byref(_cfg())) == A.ADSB_E_ARG
    assert lib.adsb_track_table_fetch_filter(None, rec.ctypes.data_as(C.POINTER(L.AdsbAircraftFilter)), 1, C.byref(n)) == A.ADSB_E_ARG
    assert lib.adsb_track_table_filter_device(None, None) == A.ADSB_E_ARG
    assert lib.adsb_track_table_fetch_frame_filter(None, fr.ctypes.data_as(C.POINTER(L.AdsbFrameFilter)), 1, C.byref(n)) == A.ADSB_E_ARG
    assert lib.adsb_debug_track_filter_operands(None, op.ctypes.data_as(C.POINTER(L.AdsbFilterOperand)), 1, C.byref(n)) == A.ADSB_E_ARG


@pytest.mark.parametrize("bad", BAD + [dict(reserved=1)], ids=lambda d: next(iter(d)))
def test_a_refused_cfg_is_refused_before_the_table_is_touched(bad):
    """The handle points at zeros: a reserve that read it before judging the cfg would follow a NULL ctx."""
    lib = L.load()
    no_table = C.create_string_buffer(1 << 14)
    assert lib.adsb_track_table_filter_reserve(C.cast(no_table, C.c_void_p), C.byref(_cfg(**bad))) == A.ADSB_E_ARG
    assert no_table.raw == bytes(1 << 14)


def test_mirror_argument_checks():
    lib = L.load()
    fx = np.array([M.fix(47.0, 8.0)]).astype(A.MLAT_FIX_DTYPE)
    op, rec, fr = np.zeros(1, dtype=A.FILTER_OPERAND_DTYPE), D.filter_empty(1), np.zeros(1, dtype=A.FRAME_FILTER_DTYPE)
    fp, opp = fx.ctypes.data_as(C.POINTER(L.AdsbMlatFix)), op.ctypes.data_as(C.POINTER(L.AdsbFilterOperand))
    rp, frp = rec.ctypes.data_as(C.POINTER(L.AdsbAircraftFilter)), fr.ctypes.data_as(C.POINTER(L.AdsbFrameFilter))
    assert lib.adsb_host_track_filter_operand(None, fp, 1.0, 1, opp) == A.ADSB_OK
    assert lib.adsb_host_track_filter_operand(None, None, 1.0, 1, opp) == A.ADSB_E_ARG
    assert lib.adsb_host_track_filter_operand(None, fp, 1.0, 1, None) == A.ADSB_E_ARG
    assert lib.adsb_host_track_filter_step(None, rp, opp, frp) == A.ADSB_OK
    assert lib.adsb_host_track_filter_step(None, rp, opp, None) == A.ADSB_OK            # frame_out is optional
    assert lib.adsb_host_track_filter_step(None, None, opp, frp) == A.ADSB_E_ARG
    assert lib.adsb_host_track_filter_step(None, rp, None, frp) == A.ADSB_E_ARG
    for bad in BAD + [dict(reserved=7)]:
        c = _cfg(**bad)
        assert lib.adsb_host_track_filter_operand(C.byref(c), fp, 1.0, 1, opp) == A.ADSB_E_ARG, bad
        assert lib.adsb_host_track_filter_step(C.byref(c), rp, opp, frp) == A.ADSB_E_ARG, bad
    with pytest.raises(TypeError):
        D._filter_cfg(no_such_field=1.0)
    # the integers: 0 takes the default, anything else is taken (a start is then VELOCITY at once with min_run = 1)
    a, f = D.host_track_filter_step(D.filter_empty(1)[0], D.host_track_filter_operand(fx[0], 1.0), min_run=1)
    assert a["flags"] == M.RUNNING | M.VELOCITY | M.HEIGHT and f["flags"] == M.USABLE | M.INIT
    a, _ = D.host_track_filter_step(D.filter_empty(1)[0], D.host_track_filter_operand(fx[0], 1.0))
    assert a["flags"] == M.RUNNING | M.HEIGHT
