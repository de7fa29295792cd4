"""Comm-B registers, CPU tier: the argument errors of the host entry points (adsb_host_commb, adsb_host_commb_as), and
COMMB_DTYPE / COMMB_HEADER_DTYPE against the ctypes structures field by field, and those against the sizes and offsets
the header text gives."""
import ctypes as C

import numpy as np

from air_rs_amd import _lib as L
from tests import commb_cases as K
from tests import commb_model as M


def test_host_commb_arguments(lib):
    fn = L.load().adsb_host_commb
    fr = M.frame_list(K.KNOWN_FRAMES[:3])
    recs, hdr = np.full(4, 0xEE, dtype=np.uint8).repeat(32).view(M.REC_DTYPE), L.AdsbCommbHeader()
    assert fn(None, 3, recs.ctypes.data, C.byref(hdr)) == lib.ADSB_E_ARG
    assert fn(fr.ctypes.data, 1 << 32, recs.ctypes.data, C.byref(hdr)) == lib.ADSB_E_CAPACITY
    assert recs.tobytes() == b"\xee" * 128 and hdr.n == 0                        # rejected calls write nothing
    assert fn(fr.ctypes.data, 3, recs.ctypes.data, None) == lib.ADSB_OK         # each output is optional
    assert recs[:3].tobytes() == M.commb(fr)["recs"].tobytes() and recs[3:].tobytes() == b"\xee" * 32
    assert fn(fr.ctypes.data, 3, None, C.byref(hdr)) == lib.ADSB_OK and (hdr.n, hdr.n_one) == (3, 3)
    assert fn(fr.ctypes.data, 3, None, None) == lib.ADSB_OK
    hdr = L.AdsbCommbHeader(*([7] * 6))
    assert fn(None, 0, None, C.byref(hdr)) == lib.ADSB_OK and bytes(hdr) == bytes(128)   # n = 0: every byte written
    assert fn(fr.ctypes.data, 0, recs.ctypes.data, C.byref(hdr)) == lib.ADSB_OK and bytes(hdr) == bytes(128)


def test_host_commb_as_arguments(lib):
    fn = L.load().adsb_host_commb_as
    rec = np.full(32, 0xEE, dtype=np.uint8).view(M.REC_DTYPE)
    b = np.frombuffer(K.KNOWN_FRAMES[1], dtype=np.uint8).copy()                  # BDS 5,0 and nothing else
    assert fn(None, 0x50, rec.ctypes.data) == lib.ADSB_E_ARG and fn(b.ctypes.data, 0x50, None) == lib.ADSB_E_ARG
    for bds in (0, 1, 0x05, 0x10, 0x17, 0x20, 0x21, 0x30, 0x40, 0x44, 0x51, 0x60, 0x70, 0x150, 0xFFFFFFFF):
        assert fn(b.ctypes.data, bds, rec.ctypes.data) == lib.ADSB_E_ARG, hex(bds)
    assert rec.tobytes() == b"\xee" * 32                                         # ... and leave *rec alone
    assert fn(b.ctypes.data, 0x50, rec.ctypes.data) == lib.ADSB_OK and int(rec["bds"][0]) == 0x50
    for other in (M.frame(b[4:11].tobytes(), df=4), M.frame(b[4:11].tobytes(), df=17), M.frame(bytes(7))):
        o = np.frombuffer(other, dtype=np.uint8).copy()                          # not Comm-B, and an empty MB
        assert all(fn(o.ctypes.data, bds, rec.ctypes.data) == lib.ADSB_E_ARG for bds in M.REGISTERS)


def test_struct_sizes_and_offsets(lib):
    assert C.sizeof(L.AdsbCommbRec) == lib.COMMB_DTYPE.itemsize == M.REC_DTYPE.itemsize == 32
    assert C.sizeof(L.AdsbCommbHeader) == lib.COMMB_HEADER_DTYPE.itemsize == M.HEADER_DTYPE.itemsize == 128
    rec_offsets = dict(state=0, bds=1, candidates=2, n_candidates=3, status=4, reserved=6, value=8, word=28)
    hdr_offsets = dict(n=0, n_commb=8, n_empty=16, n_none=24, n_one=32, n_ambiguous=40, n_bds=48, reserved=104)
    for struct, dtype, offsets in ((L.AdsbCommbRec, lib.COMMB_DTYPE, rec_offsets), (L.AdsbCommbHeader, lib.COMMB_HEADER_DTYPE, hdr_offsets)):
        assert [f[0] for f in struct._fields_] == list(dtype.names) == list(offsets)
        for name in dtype.names:
            field = getattr(struct, name)
            assert field.offset == dtype.fields[name][1] == offsets[name], name
            assert field.size == dtype.fields[name][0].itemsize, name
    assert lib.COMMB_DTYPE.fields["value"][0].shape == (5,) and lib.COMMB_DTYPE.fields["value"][0].base == np.dtype("<i4")
    assert lib.COMMB_DTYPE == M.REC_DTYPE and lib.COMMB_HEADER_DTYPE == M.HEADER_DTYPE
    assert lib.COMMB_STATES == M.STATE_NAMES and lib.COMMB_REGISTERS == M.REGISTERS
    assert [getattr(lib, "ADSB_COMMB_" + s) for s in M.STATE_NAMES] == list(range(5))
    assert [getattr(lib, f"ADSB_COMMB_C{b:02X}") for b in M.REGISTERS] == [M.BIT[b] for b in M.REGISTERS]
