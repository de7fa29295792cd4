"""The track bank's C entry points (adsb_track_bank_*) reject bad arguments before touching a device (CPU tier: no
GPU is needed for any of these)."""
import ctypes as C

from air_rs_amd import _lib


def _cfg(n_receivers=4, max_aircraft=0, max_frames=1024, sps=0.5e-6, abi=None, reserved=0):
    return _lib.AdsbTrackBankCfg(_lib.ADSB_ABI_VERSION if abi is None else abi, n_receivers, max_aircraft, reserved,
                                 max_frames, sps)


def test_track_bank_bad_arguments(lib):
    L = _lib.load()
    h = C.c_void_p()
    fake_ctx = C.create_string_buffer(64)           # never dereferenced: every check below fails first
    assert L.adsb_track_bank_create(None, C.byref(_cfg()), C.byref(h)) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_create(C.addressof(fake_ctx), None, C.byref(h)) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_create(C.addressof(fake_ctx), C.byref(_cfg()), None) == lib.ADSB_E_ARG
    for bad in (_cfg(abi=99),                       # wrong ABI version
                _cfg(reserved=1),
                _cfg(n_receivers=0), _cfg(n_receivers=257),
                _cfg(max_aircraft=(1 << 24) + 1),   # more than 2^24 ICAOs per receiver
                _cfg(max_frames=0), _cfg(max_frames=1 << 32),
                _cfg(sps=0.0), _cfg(sps=-1.0)):
        assert L.adsb_track_bank_create(C.addressof(fake_ctx), C.byref(bad), C.byref(h)) == lib.ADSB_E_ARG
    n, flags = C.c_size_t(), (C.c_uint32 * 4)()
    counts = (C.c_uint64 * 4)()
    assert L.adsb_track_bank_update(None, None, 0, None, None) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_update(None, None, 3, counts, None) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_update_launch(None, None) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_reset(None) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_fetch_points(None, None, 0, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_fetch(None, None, 0, C.byref(n), counts, flags) == lib.ADSB_E_ARG
    L.adsb_track_bank_destroy(None)


def test_track_bank_layout(lib):
    assert C.sizeof(_lib.AdsbTrackBankCfg) == 32
    assert _lib.AdsbTrackBankCfg.max_frames.offset == 16 and _lib.AdsbTrackBankCfg.seconds_per_sample.offset == 24
    assert hasattr(lib, "TrackBank")
