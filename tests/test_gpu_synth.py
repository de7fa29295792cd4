"""adsb_synth_fill_device (synth_kernel) byte for byte against adsb_synth_fill_host and the NumPy model of the source
(tests/synth_model.py): both sample types, lengths around the grid's thread count (adsb_debug_synth_geometry: past it a
thread goes round the kernel's loop), starts across 2^32 and at a rank's base 2^33 * rank, channels up to 2^32 - 1,
every configuration of tests/synth_model.py CONFIGS (tests/test_synth_model.py shows on the CPU what each reaches),
destinations at odd sample offsets inside a sentinel-filled buffer, a range written in two calls, rejected configs.
Every comparison is == ; every device write is checked for what it left outside its range."""
import ctypes as C

import numpy as np
import pytest

import air_rs_amd as A
from tests import synth_model as M

pytestmark = pytest.mark.gpu
TYPES = {"i8": A.ADSB_SAMPLE_I8, "i16": A.ADSB_SAMPLE_I16}
SENTINEL, GUARD = 0x5A, 64      # guard samples behind every range


@pytest.fixture(scope="module")
def dems(gpu):
    import torch
    # The framework's current stream is the default one, handle 0, and a context given 0 makes a non-blocking stream of
    # its own: nothing orders the framework's work against it.  device_fill waits for its sentinel fill before it generates.
    stream = torch.cuda.current_stream().cuda_stream
    with A.AdsbDemod(sample_type=A.ADSB_SAMPLE_I8, max_samples=4096, max_out=16, stream=stream, host_staging=False) as d8, \
         A.AdsbDemod(sample_type=A.ADSB_SAMPLE_I16, max_samples=4096, max_out=16, stream=stream, host_staging=False) as d16:
        yield {"i8": d8, "i16": d16}


@pytest.fixture(scope="module")
def threads(gpu):
    t = C.c_uint32()
    assert A.load().adsb_debug_synth_geometry(C.byref(t)) == A.ADSB_OK and A.load().adsb_debug_synth_geometry(None) == A.ADSB_OK
    assert 256 <= t.value <= 1 << 24 and t.value % 64 == 0, t.value     # (bounds the buffers below; the value itself is the library's)
    return t.value


def _same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:3]], want[bad[:3]])


def _bps(t):
    return 2 if t == "i8" else 4


def device_fill(dems, t, cfg, channel, first, n, at=0, cuts=()):
    """[first, first + n) generated on the device `at` samples into a sentinel buffer (in several calls cut at `cuts`):
    the range as an (n, 2) array, after checking that every byte before and behind it is still the sentinel."""
    import torch
    bps = _bps(t)
    buf = torch.full(((at + n + GUARD) * bps,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()       # the fill is done before the generator, on the context's stream, writes over it
    edges = [0, *cuts, n]
    for a, b in zip(edges[:-1], edges[1:]):
        dems[t].synth_fill_device(cfg, channel, first + a, b - a, buf.data_ptr() + (at + a) * bps)
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[:at * bps] == SENTINEL).all() and (raw[(at + n) * bps:] == SENTINEL).all(), "wrote outside its range"
    return raw[at * bps:(at + n) * bps].view(np.int8 if t == "i8" else np.int16).reshape(n, 2)


def check(dems, t, cfg, channel, first, n, want=None, **kw):
    got = device_fill(dems, t, cfg, channel, first, n, **kw)
    host = A.synth_fill_host(cfg, TYPES[t], channel, first, n)
    _same(got, host, "device != host")
    _same(host, M.fill(cfg, TYPES[t], channel, first, n) if want is None else want, "host != model")
    return got


# ---- lengths around the grid ------------------------------------------------------------------------------------------
LENGTH_CFG = dict(seed=51, slot_len=700, amp_shift=3)
LENGTH_AT = (3, 123457)      # channel, first


@pytest.fixture(scope="module")
def long_reference(threads):
    """The model over the longest range of the length cases, once per type; shorter lengths are its prefixes."""
    return {t: M.fill(M.config(**LENGTH_CFG), st, *LENGTH_AT, 2 * threads + 3) for t, st in TYPES.items()}


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("which", ["0", "1", "255", "256", "257", "T-1", "T", "T+1", "2T+3"])
def test_lengths(dems, threads, long_reference, which, t):
    n = {"T-1": threads - 1, "T": threads, "T+1": threads + 1, "2T+3": 2 * threads + 3}.get(which) or int(which)
    got = check(dems, t, A.synth_default(**LENGTH_CFG), *LENGTH_AT, n, want=long_reference[t][:n])
    assert len(got) == n
    if n >= 2 * threads:     # the samples of the second trip round the loop are not the first trip's
        assert (got[threads:2 * threads] != got[:threads]).any()


def test_zero_samples_writes_nothing_and_needs_no_buffer(dems):
    for t in TYPES:
        dems[t].synth_fill_device(A.synth_default(), 0, 0, 0, None)


# ---- starts and channels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
def test_starts_and_channels(dems, t):
    cfg = A.synth_default(seed=52, slot_len=700)
    for first in M.FIRSTS:
        for channel in M.CHANNELS:
            check(dems, t, cfg, channel, first, 2000)
    assert M.FIRSTS[2] < 2**32 < M.FIRSTS[2] + 2000


# ---- configurations ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("name", M.CONFIGS)
def test_configs(dems, name, t):
    over, n = M.CONFIGS[name]
    check(dems, t, A.synth_default(**over), 0, 0, n, want=M.reference(name, TYPES[t]))


# ---- placement: odd sample offsets into a larger buffer (an i8 destination is then 2-byte aligned only) -------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("at", [1, 3, 5])
def test_placement(dems, threads, at, t):
    cfg = A.synth_default(seed=53, slot_len=300, noise_div=4)
    for n in (1, 257, 70001):
        check(dems, t, cfg, 1, 2**33 * 7 - 100, n, at=at)


# ---- slices: what time-sharding relies on -----------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
def test_one_call_equals_two(dems, threads, t):
    cfg = A.synth_default(seed=54, slot_len=900)
    first, n = 2**33 * 3 - 40_000, 100_001
    whole = check(dems, t, cfg, 2, first, n)
    boundary = -first % 900                   # first + boundary is the first sample of a slot
    assert (first + boundary) % 900 == 0 and 0 < boundary < n
    for cut in (12_345, boundary, boundary + 1, boundary - 1, 1, n - 1):
        _same(device_fill(dems, t, cfg, 2, first, n, cuts=(cut,)), whole, cut)
    _same(device_fill(dems, t, cfg, 2, first, n, at=1, cuts=(boundary, boundary + 239, boundary + 240)), whole)


# ---- rejected configs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
def test_rejected_configs_leave_the_buffer_alone(dems, t):
    import torch
    n = 4096
    buf = torch.full((n * _bps(t),), SENTINEL, dtype=torch.uint8, device="cuda")
    lib = A.load()
    for over in M.REJECTED:
        cfg = A.synth_default(**over)
        host = np.full(n * _bps(t), SENTINEL, dtype=np.uint8)
        assert lib.adsb_synth_fill_host(C.byref(cfg), TYPES[t], 0, 0, n, host.ctypes.data) == A.ADSB_E_ARG, over
        assert (host == SENTINEL).all()
        assert lib.adsb_synth_fill_device(dems[t].handle, C.byref(cfg), 0, 0, n, buf.data_ptr()) == A.ADSB_E_ARG, over
        with pytest.raises(A.AdsbError) as e:
            dems[t].synth_fill_device(cfg, 0, 0, n, buf.data_ptr())
        assert e.value.code == A.ADSB_E_ARG
    assert lib.adsb_synth_fill_device(None, C.byref(A.synth_default()), 0, 0, n, buf.data_ptr()) == A.ADSB_E_ARG
    assert lib.adsb_synth_fill_device(dems[t].handle, C.byref(A.synth_default()), 0, 0, n, None) == A.ADSB_E_ARG
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == SENTINEL).all()
    # the same buffer, a config that is accepted: the call does write
    dems[t].synth_fill_device(A.synth_default(), 0, 0, n, buf.data_ptr())
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() != SENTINEL).any()
