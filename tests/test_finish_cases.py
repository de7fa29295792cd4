"""tests/finish_cases.py on the CPU: the launches it deals can show a wrong `before` in finish_order.  Every assertion is a
condition on the inputs of tests/test_gpu_finish_exchange.py, none a measurement: the pool's lists are whole and fit a
tile's own slots, the workgroups' totals differ where groups meet, every workgroup has frames to misplace, and the model
of finish_block's exchange with one term missing (finish_cases.MUTANTS) never gives the expected list -- for every shape
the term is read in, whichever of two colliding tiles writes last."""
import numpy as np
import pytest

import air_rs_amd as A
from tests import finish_cases as FC

STS = {"i8": A.ADSB_SAMPLE_I8, "i16": A.ADSB_SAMPLE_I16}
# (sample type, shape): what tests/test_gpu_finish_exchange.py launches
LAUNCHES = [("i8", "flat"), ("i8", "first"), ("i8", "whole"), ("i8", "ragged"), ("i8", "big"), ("i16", "first")]


@pytest.fixture(scope="module")
def g(lib):
    return FC.geometry()


def test_geometry_and_shapes(g):
    assert all(v > 0 for v in g) and g.L % g.F == 0 and g.S % 64 == 0 and g.T <= 64 and g.F <= 64
    for name, (workgroups, last, n_samples) in FC.shapes(g).items():
        tiles = FC.tiles_of(g, workgroups, last)
        assert 1 <= last <= g.T and -(-tiles // g.T) == workgroups, name
        assert n_samples % 8 == 0 and n_samples > FC.WINDOW                # a channel stride; at least one offset
        assert (workgroups <= g.L) == (name == "flat")
        # only the big shape gives a workgroup more earlier groups than one round reads
        assert ((workgroups - 1) // g.F > g.S) == (name == "big")
    s = FC.shapes(g)
    assert s["first"][0] % g.F == 1 and s["whole"][0] % g.F == 0 and s["ragged"][0] % g.F == 1
    assert (s["big"][0] - 1) // g.F == g.S + 1


@pytest.mark.parametrize("st", STS)
@pytest.mark.parametrize("n_samples", [FC.SAMPLES, FC.SAMPLES_BIG, 1000])
def test_pool(oracle, st, n_samples):
    p = FC.pool(oracle, STS[st], n_samples)
    n_off = n_samples - FC.WINDOW
    assert p.iq.shape == (FC.POOL, n_samples, 2) and FC.POOL >= 64 and p.iq.dtype == FC.DTYPES[STS[st]]
    assert len({b.tobytes() for b in p.iq}) == FC.POOL
    for buf, want in zip(p.iq, p.lists):
        # the list is whole (room for one frame per offset and one more) and fits the tile's own slots
        rc, again, found = oracle.process_buffer(buf, max_out=n_off + 1)
        assert rc == 0 and found == len(want) <= min(FC.KQUOTA, n_off) and again.tobytes() == want.tobytes()
        assert (np.diff(want["offset"].astype(np.int64)) > 0).all() and (want["offset"] < n_off).all()
    kinds = set(p.counts.tolist())
    assert {0, 1} <= kinds and len(kinds) >= 4 and max(kinds) >= 8
    assert (2 in kinds) == (n_off >= FC.SLOT)
    # different frame bytes: every planted frame is another one
    planted = {bytes(f["bytes"]) for f in p.frames if f["bytes"].any()}
    assert len(planted) >= FC.POOL // 3
    assert {0, 1} <= set(p.frames["status"].tolist())                      # clean and repaired frames


@pytest.mark.parametrize("st,name", LAUNCHES)
def test_the_deal_can_show_a_wrong_prefix(oracle, g, st, name):
    c = FC.case(oracle, STS[st], name)
    workgroups, last, n_samples = FC.shapes(g)[name]
    assert len(c.perm) == FC.tiles_of(g, workgroups, last) and c.pool.iq.shape[1] == n_samples
    assert c.prefix[-1] == len(c.frames) == c.counts.sum() and len(set(c.counts.tolist())) >= 4
    # no period: no shift up to two groups of tiles maps the deal onto itself
    for shift in (1, g.T, g.F, g.T * g.F, 2 * g.T * g.F):
        assert (c.perm[shift:] != c.perm[:-shift]).mean() > 0.9, shift
    totals = FC.workgroup_totals(c.counts, g)
    assert len(totals) == workgroups and totals.min() > 0                  # any missing term moves a workgroup with frames
    assert c.counts[-1] >= 2
    sums = FC.group_sums(totals, g)
    assert (sums[1:] != sums[:-1]).all()                                   # no two adjacent groups have equal sums
    half = g.F // 2
    for edge in range(g.F, workgroups, g.F):                               # the 32 workgroups on either side of every edge
        near = totals[edge - half:min(edge + half, workgroups)]
        assert (near[1:] != near[:-1]).mean() >= 0.5, edge
    # the unchanged model gives the expected list: the concatenation in channel order
    assert FC.model_list(c, g).tobytes() == c.frames.tobytes()


@pytest.mark.parametrize("st,name", LAUNCHES)
def test_mutants(oracle, g, st, name):
    c = FC.case(oracle, STS[st], name)
    workgroups = FC.shapes(g)[name][0]
    ran = 0
    for wrong, applies in FC.MUTANTS:
        if not applies(workgroups, g):
            # the code it breaks does not run: the model is the unchanged one
            if (workgroups <= g.L) == wrong.startswith("flat"):
                assert FC.model_list(c, g, wrong).tobytes() == c.frames.tobytes(), wrong
            continue
        ran += 1
        for descending in (False, True):
            got = FC.model_list(c, g, wrong, descending)
            differ = int((got != c.frames).sum())
            print(f"{name:7s} {wrong:60s} {'descending' if descending else 'ascending ':10s} {differ} of {len(got)} places differ")
            assert differ > 0, (name, wrong, descending)
    assert ran == (2 if name == "flat" else 7 if name == "big" else 6)


def test_every_mutant_is_caught_by_a_launch(g):
    for wrong, applies in FC.MUTANTS:
        assert any(applies(FC.shapes(g)[name][0], g) for _, name in LAUNCHES), wrong
    beyond = FC.MUTANTS[-1]
    assert [name for _, name in LAUNCHES if beyond[1](FC.shapes(g)[name][0], g)] == ["big"]
