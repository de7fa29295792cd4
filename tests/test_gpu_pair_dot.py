"""mags8_i8 forms the even sample of each dword from a masked dot and the odd sample from the difference of two dots inside
a packed FMA (air_rs_amd/csrc/adsb_kernels.hip; arithmetic model: tests/test_pair_dot_model.py).  Every (I, Q) an i8 stream
can carry goes through BOTH positions here, next to fixed and random partners, under each converter mode that is correct
on every device, and one synthetic buffer goes through the scan kernel at both alignments."""
import numpy as np
import pytest

import air_rs_amd as A

pytestmark = pytest.mark.gpu

PARTNERS = {"zero": (0, 0), "one": (1, 0), "max": (127, 127), "min": (-128, -128), "random": None}


def _all_iq():
    i, q = np.meshgrid(np.arange(-128, 128), np.arange(-128, 128), indexing="ij")
    return np.stack([i.ravel(), q.ravel()], axis=1).astype(np.int8)        # 65 536 samples


@pytest.fixture(scope="module")
def pair_cases(oracle):
    """{name: (iq int8 [131072, 2], expected magnitudes)}: sample 2p and 2p + 1 share a dword; 'odd/...' puts every (I, Q) in
    the odd position next to the named even partner, 'even/...' swaps the roles."""
    every = _all_iq()
    rng = np.random.default_rng(20240607)
    out = {}
    for name, fixed in PARTNERS.items():
        partner = (rng.integers(-128, 128, size=every.shape).astype(np.int8) if fixed is None
                   else np.broadcast_to(np.array(fixed, dtype=np.int8), every.shape))
        for role in ("odd", "even"):
            iq = np.empty((2 * every.shape[0], 2), dtype=np.int8)
            iq[(1 if role == "odd" else 0)::2] = every
            iq[(0 if role == "odd" else 1)::2] = partner
            out[f"{role}/{name}"] = (iq, oracle.get_magnitude(iq.astype(np.int16)))
    return out


@pytest.mark.parametrize("force", [None, 1, 2], ids=["probed", "mode1", "mode2"])
def test_every_iq_in_both_positions(gpu, pair_cases, monkeypatch, force):
    # mode 0 is correct only where the converter truncates natively: never forced.  ADSB_FORCE_MAG_MODE is read by adsb_create.
    if force is None:
        monkeypatch.delenv("ADSB_FORCE_MAG_MODE", raising=False)
    else:
        monkeypatch.setenv("ADSB_FORCE_MAG_MODE", str(force))
    with A.AdsbDemod(sample_type=A.ADSB_SAMPLE_I8, max_samples=1 << 18, max_out=1 << 10) as d:
        assert force is None or d.mag_mode == force
        for name, (iq, want) in pair_cases.items():
            got = d.magnitudes(iq)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (name, d.mag_mode, bad[:8], iq[bad[:8]].tolist(), got[bad[:8]], want[bad[:8]])


def _eq(got, want):
    assert len(got) == len(want), (len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:5], got[bad[:3]], want[bad[:3]])


@pytest.mark.parametrize("n", [16384 + 241, 2 * 16384 + 777])
def test_scan_at_both_alignments(gpu, oracle, monkeypatch, n):
    # iq and iq[1:]: every sample passes through the masked path in one run and the difference path in the other
    monkeypatch.delenv("ADSB_FORCE_MAG_MODE", raising=False)
    iq = A.synth_fill_host(A.synth_default(seed=4100 + n, slot_len=600), A.ADSB_SAMPLE_I8, 0, 0, n)
    with A.AdsbDemod(sample_type=A.ADSB_SAMPLE_I8, max_samples=1 << 18, max_out=1 << 12) as d:
        for buf in (iq, iq[1:]):
            frames, flags = d.demod(buf)
            rc, want, found = oracle.process_buffer(buf, max_out=d.max_out)
            assert rc == 0 and found <= d.max_out and not (flags & A.ADSB_FLAG_TRUNCATED)
            assert len(want) >= 1
            _eq(frames, want)
