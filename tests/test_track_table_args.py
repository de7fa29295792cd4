"""The persistent track table's C entry points (adsb_track_table_*) reject bad arguments before touching a device
(CPU tier: no GPU is needed for any of these)."""
import ctypes as C

from air_rs_amd import _lib


def test_track_table_bad_arguments(lib):
    L = _lib.load()
    h = C.c_void_p()
    cfg = _lib.AdsbTrackTableCfg(_lib.ADSB_ABI_VERSION, 0, 1024, 0.5e-6)
    fake_ctx = C.create_string_buffer(64)           # never dereferenced: every check below fails first
    assert L.adsb_track_table_create(None, C.byref(cfg), C.byref(h)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_create(C.addressof(fake_ctx), None, C.byref(h)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_create(C.addressof(fake_ctx), C.byref(cfg), None) == lib.ADSB_E_ARG
    for bad in (_lib.AdsbTrackTableCfg(99, 0, 1024, 0.5e-6),              # wrong ABI version
                _lib.AdsbTrackTableCfg(_lib.ADSB_ABI_VERSION, 0, 0, 0.5e-6),  # no frames
                _lib.AdsbTrackTableCfg(_lib.ADSB_ABI_VERSION, 0, 1 << 32, 0.5e-6),
                _lib.AdsbTrackTableCfg(_lib.ADSB_ABI_VERSION, 0, 1024, 0.0),  # no time base
                _lib.AdsbTrackTableCfg(_lib.ADSB_ABI_VERSION, (1 << 24) + 1, 1024, 0.5e-6)):  # more than 2^24 ICAOs
        assert L.adsb_track_table_create(C.addressof(fake_ctx), C.byref(bad), C.byref(h)) == lib.ADSB_E_ARG
    n, flags = C.c_size_t(), C.c_uint32()
    assert L.adsb_track_table_update(None, None, 0, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_reset(None) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fetch_points(None, None, 0, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fetch(None, None, 0, C.byref(n), C.byref(flags)) == lib.ADSB_E_ARG
    L.adsb_track_table_destroy(None)


def test_track_table_flags_and_layout(lib):
    assert lib.ADSB_TRACK_UNTRACKED == 0x2 and lib.ADSB_TRACK_TABLE_FULL == 0x1
    assert lib.ADSB_TRACK_UNTRACKED & lib.ADSB_TRACK_NEW_POSITION == 0
    assert C.sizeof(_lib.AdsbTrackTableCfg) == 24 and _lib.AdsbTrackTableCfg.seconds_per_sample.offset == 16
    assert hasattr(lib, "TrackTable")
