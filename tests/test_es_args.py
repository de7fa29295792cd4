"""Extended squitter status, CPU tier: the argument errors of the host entry point (adsb_host_es), the ctypes signatures
of the stage's entry points, and ES_DTYPE / ES_HEADER_DTYPE against the ctypes structures field by field, and those
against the sizes and offsets the header text gives."""
import ctypes as C
import os
import re

import numpy as np

from air_rs_amd import _lib as L
from tests import es_cases as K
from tests import es_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_es_arguments(lib):
    fn = L.load().adsb_host_es
    fr = M.frame_list(K.KNOWN_FRAMES[:3])
    recs, hdr = np.full(4, 0xEE, dtype=np.uint8).repeat(32).view(M.REC_DTYPE), L.AdsbEsHeader()
    assert fn(None, 3, recs.ctypes.data, C.byref(hdr)) == lib.ADSB_E_ARG
    assert fn(fr.ctypes.data, 1 << 32, recs.ctypes.data, C.byref(hdr)) == lib.ADSB_E_CAPACITY
    assert recs.tobytes() == b"\xee" * 128 and hdr.n == 0                        # rejected calls write nothing
    assert fn(fr.ctypes.data, 3, recs.ctypes.data, None) == lib.ADSB_OK         # each output is optional
    assert recs[:3].tobytes() == M.es(fr)["recs"].tobytes() and recs[3:].tobytes() == b"\xee" * 32
    assert fn(fr.ctypes.data, 3, None, C.byref(hdr)) == lib.ADSB_OK and (hdr.n, hdr.n_state[M.EMERGENCY]) == (3, 1)
    assert fn(fr.ctypes.data, 3, None, None) == lib.ADSB_OK
    hdr = L.AdsbEsHeader(7)
    assert fn(None, 0, None, C.byref(hdr)) == lib.ADSB_OK and bytes(hdr) == bytes(128)   # n = 0: every byte written
    assert fn(fr.ctypes.data, 0, recs.ctypes.data, C.byref(hdr)) == lib.ADSB_OK and bytes(hdr) == bytes(128)


def test_signatures(lib):
    """every entry point of the stage is in the library with the prototype the headers give it"""
    lib_handle = L.load()
    want = {"adsb_es_of": 3, "adsb_fetch_es": 4, "adsb_es_device": 3, "adsb_debug_es_geometry": 1, "adsb_host_es": 4,
            "adsb_host_es_integrity": 5}
    headers = "".join(open(os.path.join(ROOT, "include", n)).read() for n in ("adsb_hip.h", "adsb_host.h"))
    for name, n_args in want.items():
        restype, argtypes = L.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == n_args, name
        fn = getattr(lib_handle, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes), name
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", headers)
        assert m and len(m.group(1).split(",")) == n_args, name
    t = C.c_uint32()
    assert lib_handle.adsb_debug_es_geometry(C.byref(t)) == lib.ADSB_OK and t.value % 64 == 0 and t.value > 0
    assert lib_handle.adsb_debug_es_geometry(None) == lib.ADSB_OK
    # no context: an argument error before anything touches a device
    assert lib_handle.adsb_es_of(None, None, 0) == lib.ADSB_E_ARG
    assert lib_handle.adsb_fetch_es(None, None, 0, None) == lib.ADSB_E_ARG
    assert lib_handle.adsb_es_device(None, None, None) == lib.ADSB_E_ARG


def test_struct_sizes_and_offsets(lib):
    assert C.sizeof(L.AdsbEsRec) == lib.ES_DTYPE.itemsize == M.REC_DTYPE.itemsize == 32
    assert C.sizeof(L.AdsbEsHeader) == lib.ES_HEADER_DTYPE.itemsize == M.HEADER_DTYPE.itemsize == 128
    rec_offsets = dict(state=0, type_code=1, subtype=2, version=3, present=4, nic_a=8, nic_b=9, nic_c=10, nac_p=11, nac_v=12,
                       sil=13, sil_supplement=14, gva=15, sda=16, nic_baro=17, category=18, emergency=19, length_width=20,
                       reserved=21, flags=22, value=24, half=28)
    hdr_offsets = dict(n=0, n_state=8, n_version=88, reserved=120)
    for struct, dtype, offsets in ((L.AdsbEsRec, lib.ES_DTYPE, rec_offsets), (L.AdsbEsHeader, lib.ES_HEADER_DTYPE, hdr_offsets)):
        assert [f[0] for f in struct._fields_] == list(dtype.names) == list(offsets)
        for name in dtype.names:
            field = getattr(struct, name)
            assert field.offset == dtype.fields[name][1] == offsets[name], name
            assert field.size == dtype.fields[name][0].itemsize, name
    assert lib.ES_DTYPE == M.REC_DTYPE and lib.ES_HEADER_DTYPE == M.HEADER_DTYPE
    assert lib.ES_STATES == M.STATE_NAMES and lib.ES_PRESENT == M.PRESENT_NAMES and lib.ES_FLAGS == M.FLAG_NAMES
    assert [getattr(lib, "ADSB_ES_" + s) for s in M.STATE_NAMES] == list(range(10))
    assert [getattr(lib, "ADSB_ES_HAS_" + s) for s in M.PRESENT_NAMES] == [M.HAS[s] for s in M.PRESENT_NAMES]
    assert [getattr(lib, "ADSB_ES_" + s) for s in M.FLAG_NAMES] == [M.FLAG[s] for s in M.FLAG_NAMES]
    assert lib.ADSB_ES_VERSION_UNKNOWN == M.VERSION_UNKNOWN
    # ... and the header's #defines carry the same values
    text = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    defined = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (ADSB_ES_\w+) (\w+?)u\n", text)}
    ours = {k: getattr(lib, k) for k in dir(lib) if k.startswith("ADSB_ES_")}
    assert defined.pop("ADSB_ES_STATES") == 10 and defined == ours and len(ours) == 10 + 27 + 11 + 1
