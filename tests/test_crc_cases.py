"""tests/crc_cases.py against the CPU oracle: the model's verdict frame by frame, the figures of every class, the survivor
band of every tile.  What the device tests (tests/test_gpu_crc_paths.py, tests/ab_cases.py) rely on, checked without a GPU."""
import numpy as np
import pytest

from tests import crc_cases as C
from tests import survivor_cases as S

# (dtype, tile length): i8 and CS16 of the product, and the A/B `reg` kernel's tile
SHAPES = [(np.int8, 16384), (np.int16, 8192), (np.int8, 16128)]
_REF = {}


def _ref(oracle, dtype, tile, path):
    key = (np.dtype(dtype).name, tile, path)
    if key not in _REF:
        c = C.cases(oracle, tile, path)
        mag = C.magnitudes(c)
        rc, want, found = oracle.process_buffer(S.to_iq(mag, dtype), max_out=1 << 12)
        assert rc == 0 and found == len(want)
        _REF[key] = (c, mag, want)
    return _REF[key]


def test_the_syndrome_table(oracle):
    """the model's table is the oracle's CRC of a single set bit; the figures the cases are built on"""
    for j in range(88):
        assert C.SYN[j] == oracle.get_adsb_crc(C.flip(bytes(11), j))
    assert C.SYN[88:] == [1 << (111 - j) for j in range(88, 112)]
    assert len(set(C.DATA_SYN)) == 88 and 0 not in C.DATA_SYN
    assert C.SORTED_SYN[0] == 0x001C1B and C.SORTED_SYN[-1] == 0xFFF409
    assert len(C.NEIGHBOURS) == 178 and not set(C.NEIGHBOURS) & set(C.DATA_SYN) and 0 not in C.NEIGHBOURS
    assert not set(C.SYN[88:]) & set(C.DATA_SYN)
    assert set(C.EDGE_NEIGHBOURS) <= set(C.NEIGHBOURS) and len(C.EDGE_NEIGHBOURS) == 10


def test_the_verdict_of_a_frame(oracle):
    f = S.frame_bytes(oracle, 0)
    assert C.syndrome(f) == 0 and C.verdict(f) == (0, 0xFF, f)
    for j in range(88):
        assert C.verdict(C.flip(f, j)) == (1, j, f)
    for j in range(88, 112):
        assert C.verdict(C.flip(f, j)) is None
    for s in C.NEIGHBOURS:
        assert C.syndrome(C.xor_crc(f, s)) == s and C.verdict(C.xor_crc(f, s)) is None
    for i, k in C.ALIASES:
        r = C.xor_crc(C.flip(f, i), C.SYN[i] ^ C.SYN[k])
        st, bit, fixed = C.verdict(r)
        assert (st, bit) == (1, k) and fixed == C.flip(r, k) and fixed != f and C.syndrome(fixed) == 0


@pytest.mark.parametrize("path", C.PATHS)
@pytest.mark.parametrize("dtype,tile", SHAPES, ids=["i8", "cs16", "i8-reg"])
def test_layout_against_the_oracle(oracle, dtype, tile, path):
    c, mag, want = _ref(oracle, dtype, tile, path)
    # the oracle equals the model, frame by frame
    model = C.model_list(mag)
    got = [(int(r["offset"]), int(r["status"]), int(r["fixed_bit"]), r["bytes"].tobytes()) for r in want]
    assert got == model
    # every class's figures, on the frames this layout uses
    C.check_figures(c, want)
    C.check_coverage(c)
    C.check_mix(c)
    # every tile in its band
    counts = C.check_bands(c, mag)
    assert len(counts) < 32 and (path == "sparse" or len(counts) < 10)
    # every fixed_bit that can come out comes out, none that cannot
    fixed = set(int(b) for b in want["fixed_bit"][want["status"] == 1])
    assert fixed == {0, 4} | set(range(5, 88))
    assert (want["fixed_bit"][want["status"] == 0] == 0xFF).all() and set(want["status"]) == {0, 1}
    # and what comes out is the plants' own: nothing valid among the extra survivors or the stubs
    assert len(want) == sum(p.item.expect is not None for p in c.plants)


@pytest.mark.parametrize("path", C.PATHS)
def test_layout_is_what_build_takes(oracle, path):
    n, plants = C.layout(oracle, 8192, path)
    c, mag, _ = _ref(oracle, np.int16, 8192, path)
    assert n == c.n_samples and (S.build(n, plants) == mag).all()
    assert (S.to_iq(mag, np.int8)[:, 0] == S.to_iq(mag, np.int16)[:, 0]).all()  # both sample types see the same values
