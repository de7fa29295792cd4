"""The replies scan's device-only text (air_rs_amd/csrc/adsb_replies.hip) on the device: device == CPU mirror == NumPy
model, byte for byte, frames, counts and header, on every case of tests/replies_cases.py's device_text_cases: crowded
runs (several candidates and kept frames in one bitmap word, the filter and the capacity inside a word), ragged ends
sample by sample, the last examined offset, a frame in every tile of 1 to 17, 300 short channels, a frame at every
offset of a tile, and the merge with 5000 channels.  tests/test_replies_device_cases_host.py asserts, without a device,
that the cases hold what they claim.  profiles/replies_device_checks.txt has the mutants of the device text these
catch."""
import numpy as np
import pytest

import air_rs_amd as A
from tests import replies_cases as K
from tests import replies_model as M
from tests.test_gpu_replies import _dev, _st, run_device
from tests.test_replies_device_cases_host import check_capacity
from tests.test_replies_host import DTYPES, run_host, same

pytestmark = pytest.mark.gpu
WIDE = ("crowded", "ragged", "window", "tiles", "offsets")


@pytest.fixture(scope="module")
def ctx(gpu):
    """per sample type: a context for the long buffers, and one of its own for 300 short channels"""
    made = {}
    for name, dtype in DTYPES.items():
        made[name] = A.AdsbDemod(sample_type=_st(dtype), max_samples=241 * K.tile(dtype), max_out=1 << 15, max_channels=8,
                                 host_staging=False)
        made[name, "channels"] = A.AdsbDemod(sample_type=_st(dtype), max_samples=136, max_out=1 << 10, max_channels=K.MANY,
                                             host_staging=False)
    yield made
    for d in made.values():
        d.close()


def _check(d, st, name):
    c, want = K.device_text_case(DTYPES[st], name), K.device_text_model(DTYPES[st], name)
    if c.get("zeros_first"):               # nothing an earlier run left in tile[] or bitmap[] stands in for a tile
        f, counts, h = run_device(d, dict(c, iq=np.zeros_like(c["iq"]), kw={}))
        assert len(f) == 0 and not counts.any() and h.tobytes() == bytes(80)
    got = run_device(d, c)
    same(got, run_host(c), name + ": device against mirror")
    same(got, want, name + ": device against model")
    K.check_expectations(c, got[0], got[1])
    if "n_preamble" in c:
        assert int(got[2]["n_preamble"]) == c["n_preamble"], name
    if c["kw"].get("max_frames"):
        check_capacity(c, got)


@pytest.mark.parametrize("name", K.device_text_names(np.int8, WIDE))
def test_device_is_mirror_is_model_i8(ctx, name):
    _check(ctx["i8"], "i8", name)


@pytest.mark.parametrize("name", K.device_text_names(np.int16, WIDE))
def test_device_is_mirror_is_model_i16(ctx, name):
    _check(ctx["i16"], "i16", name)


@pytest.mark.parametrize("st", ["i8", "i16"])
@pytest.mark.parametrize("name", K.device_text_names(np.int8, ("channels",)))
def test_more_channels_than_threads(ctx, st, name):
    """counts[] of 300 channels, the header and the list; every tile is one short channel with its neighbour behind it.
    The two cases differ in every count that is not 0, so neither passes on what the other left in counts[]."""
    _check(ctx[st, "channels"], st, name)


def test_merge_with_many_channels_on_the_device(ctx):
    """5000 channels, runs of empty ones, one channel with 600 frames: frames, src and counts against model and mirror,
    from host lists and from device lists"""
    _, a, ca, b, cb = K.merge_many_channels()
    d = ctx["i8"]
    want, mirror = M.merge(a, ca, b, cb), A.host_merge_lists(a, ca, b, cb)
    da, db = _dev(a.view(np.uint8)), _dev(b.view(np.uint8))
    for got in (d.merge_lists(a, ca, b, cb), d.merge_lists((da.data_ptr(), len(a)), ca, (db.data_ptr(), len(b)), cb)):
        for other in (want, mirror):
            assert got[0].tobytes() == other[0].tobytes() and got[1].tolist() == other[1].tolist()
            assert got[2].tolist() == other[2].tolist()
    del da, db
