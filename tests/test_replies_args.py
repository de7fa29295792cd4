"""Mode S replies from samples, CPU tier: the argument errors of the host entry points (adsb_host_replies,
adsb_host_merge_lists), the ctypes signatures of the stage's entry points against the headers, and the structures
against the sizes and offsets the header text gives."""
import ctypes as C
import os
import re

import numpy as np

import air_rs_amd as A
from air_rs_amd import _lib as L
from tests import replies_cases as K
from tests import replies_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call(iq, cfg=None, st=A.ADSB_SAMPLE_I8, nch=1, n=None, stride=None, known=None, out=None, header=None, counts=None):
    cfg = L.AdsbRepliesCfg() if cfg is None else cfg
    n = len(iq) // nch if n is None else n
    return L.load().adsb_host_replies(st, C.byref(cfg) if cfg else None, None if iq is None else iq.ctypes.data, nch, n,
                                      n if stride is None else stride, None if known is None else known.ctypes.data,
                                      0 if known is None else len(known), None if out is None else out.ctypes.data,
                                      0 if out is None else len(out), None, None if counts is None else counts.ctypes.data,
                                      None if header is None else C.byref(header))


def test_host_replies_arguments(lib):
    iq = np.zeros((600, 2), dtype=np.int8)
    M.render(iq, K.message(4), 10)
    out = np.full(2, 0xEE, dtype=np.uint8).repeat(24).view(A.FRAME_DTYPE)
    hdr, counts = L.AdsbRepliesHeader(7), np.full(1, 99, dtype=np.uint64)
    u32 = lambda *v: np.array(v, dtype=np.uint32)
    bad = [
        dict(iq=None, n=600),                                            # NULL samples
        dict(cfg=False),                                                 # NULL cfg
        dict(nch=0, n=600),
        dict(st=2),
        dict(cfg=L.AdsbRepliesCfg(2)), dict(cfg=L.AdsbRepliesCfg(0, 1)), dict(cfg=L.AdsbRepliesCfg(0, 0, 0, 0, 1)),
        dict(nch=2, n=300, stride=299),                                  # a stride below n_samples
        dict(known=u32(5, 5)), dict(known=u32(9, 5)), dict(known=u32(1 << 24)),   # not ascending, distinct, < 2^24
    ]
    for kw in bad:
        assert _call(**{"iq": iq, "out": out, "header": hdr, "counts": counts, **kw}) == lib.ADSB_E_ARG, kw
    assert L.load().adsb_host_replies(0, C.byref(L.AdsbRepliesCfg()), iq.ctypes.data, 1, 600, 600, None, 1, None, 0, None, None,
                                      None) == lib.ADSB_E_ARG       # NULL known with a count
    assert L.load().adsb_host_replies(0, C.byref(L.AdsbRepliesCfg()), iq.ctypes.data, 1, 600, 600, None, 0, None, 1, None, None,
                                      None) == lib.ADSB_E_ARG       # NULL out with a capacity
    assert _call(iq, n=25, out=out, header=hdr, counts=counts) == lib.ADSB_E_SHORT
    assert _call(iq, cfg=L.AdsbRepliesCfg(0, 0, 1 << 32), out=out, header=hdr, counts=counts) == lib.ADSB_E_CAPACITY
    assert out.tobytes() == b"\xee" * 48 and hdr.n_out == 7 and counts[0] == 99      # rejected calls write nothing
    assert _call(iq, n=26, header=hdr) == lib.ADSB_OK and bytes(hdr) == bytes(80)    # the shortest buffer: one offset
    assert _call(iq) == lib.ADSB_OK                                                 # every output is optional
    assert _call(iq, out=out, header=hdr, counts=counts) == lib.ADSB_OK
    assert (hdr.n_out, hdr.n_address_parity, counts[0], int(out[0]["offset"])) == (1, 1, 1, 10)
    assert out[1].tobytes() == b"\xee" * 24
    assert _call(iq, nch=2, n=300, stride=300, header=hdr) == lib.ADSB_OK and hdr.n_out == 1   # channels that touch
    assert _call(iq, nch=1, n=600, stride=1, header=hdr) == lib.ADSB_OK and hdr.n_out == 1     # one channel ignores the stride
    assert _call(iq, cfg=L.AdsbRepliesCfg(1), known=u32(), header=hdr) == lib.ADSB_OK and (hdr.n_out, hdr.n_not_known) == (0, 1)


def test_host_merge_arguments(lib):
    fn = L.load().adsb_host_merge_lists
    _, a, ca, b, cb = K.merge_cases()[0]
    ca, cb = np.array(ca, dtype=np.uint64), np.array(cb, dtype=np.uint64)
    out = np.full(10, 0xEE, dtype=np.uint8).repeat(24).view(A.FRAME_DTYPE)
    ok = (a.ctypes.data, ca.ctypes.data, b.ctypes.data, cb.ctypes.data, 1, out.ctypes.data, None, None)
    for k, v in ((1, None), (3, None), (4, 0), (4, (1 << 20) + 1), (0, None), (2, None), (5, None)):
        args = list(ok)
        args[k] = v
        assert fn(*args) == lib.ADSB_E_ARG, k
    huge = np.array([1 << 31], dtype=np.uint64)
    assert fn(a.ctypes.data, huge.ctypes.data, b.ctypes.data, cb.ctypes.data, 1, out.ctypes.data, None, None) == lib.ADSB_E_CAPACITY
    assert out.tobytes() == b"\xee" * 240                                            # rejected calls write nothing
    assert fn(*ok) == lib.ADSB_OK and out[9].tobytes() == b"\xee" * 24               # src and counts_out are optional
    zero = np.zeros(1, dtype=np.uint64)
    assert fn(None, zero.ctypes.data, None, zero.ctypes.data, 1, None, None, None) == lib.ADSB_OK   # nothing to merge


def test_signatures(lib):
    """every entry point of the stage is in the library with the prototype the headers give it"""
    h = L.load()
    want = {"adsb_replies_of": 8, "adsb_fetch_replies": 6, "adsb_replies_device": 4, "adsb_debug_replies_geometry": 2,
            "adsb_merge_lists_of": 9, "adsb_host_replies": 13, "adsb_host_merge_lists": 8}
    headers = "".join(open(os.path.join(ROOT, "include", n)).read() for n in ("adsb_hip.h", "adsb_host.h"))
    for name, n_args in want.items():
        restype, argtypes = L.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == n_args, name
        fn = getattr(h, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes), name
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", headers)
        assert m and len(m.group(1).split(",")) == n_args, name
    a, b = C.c_uint32(), C.c_uint32()
    assert h.adsb_debug_replies_geometry(C.byref(a), C.byref(b)) == lib.ADSB_OK
    assert a.value % 256 == 0 and b.value % 256 == 0 and a.value >= 256 and b.value >= 256
    assert h.adsb_debug_replies_geometry(None, None) == lib.ADSB_OK
    # no context: an argument error before anything touches a device
    assert h.adsb_replies_of(None, None, None, 1, 100, 100, None, 0) == lib.ADSB_E_ARG
    assert h.adsb_fetch_replies(None, None, 0, None, None, None) == lib.ADSB_E_ARG
    assert h.adsb_replies_device(None, None, None, None) == lib.ADSB_E_ARG
    assert h.adsb_merge_lists_of(None, None, None, None, None, 1, None, None, None) == lib.ADSB_E_ARG


def test_struct_sizes_and_offsets(lib):
    assert C.sizeof(L.AdsbRepliesCfg) == 32
    assert C.sizeof(L.AdsbRepliesHeader) == lib.REPLIES_HEADER_DTYPE.itemsize == M.HEADER_DTYPE.itemsize == 80
    cfg_offsets = dict(flags=0, reserved=4, max_frames=8, first_sample_index=16, reserved2=24)
    assert [f[0] for f in L.AdsbRepliesCfg._fields_] == list(cfg_offsets)
    for name, off in cfg_offsets.items():
        assert getattr(L.AdsbRepliesCfg, name).offset == off, name
    assert [f[0] for f in L.AdsbRepliesHeader._fields_] == list(lib.REPLIES_HEADER_DTYPE.names) == list(M.HEADER_FIELDS)
    for k, name in enumerate(M.HEADER_FIELDS):
        assert getattr(L.AdsbRepliesHeader, name).offset == lib.REPLIES_HEADER_DTYPE.fields[name][1] == 8 * k, name
    assert lib.REPLIES_HEADER_DTYPE == M.HEADER_DTYPE
    # ... and the header text says the same: the sizes in its comments, the fields in order, the #defines' values
    text = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    m = re.search(r"typedef struct adsb_replies_header \{\s*/\* (\d+) bytes \*/\s*uint64_t ([^;]*);", text)
    assert m and int(m.group(1)) == 80 and [s.strip() for s in m.group(2).split(",")] == list(M.HEADER_FIELDS)
    m = re.search(r"typedef struct adsb_replies_cfg \{\s*/\* (\d+) bytes \*/(.*?)\} adsb_replies_cfg;", text, flags=re.S)
    assert m and int(m.group(1)) == 32
    assert re.findall(r"uint\d+_t (\w+);", m.group(2)) == list(cfg_offsets)
    defined = {k: int(v, 0) for k, v in re.findall(r"#define (ADSB_REPLIES_\w+|ADSB_MERGE_\w+) (\w+?)u\n", text)}
    assert defined == {"ADSB_REPLIES_AP_KNOWN": lib.ADSB_REPLIES_AP_KNOWN, "ADSB_MERGE_FROM_B": lib.ADSB_MERGE_FROM_B}
    assert lib.ADSB_MERGE_FROM_B == M.FROM_B and lib.REPLIES_AP == {"all": 0, "known": lib.ADSB_REPLIES_AP_KNOWN}
