"""The streaming front end (adsb_feed_*, air_rs_amd.Feed) where its own tests do not go: ring slots reused under a list
that has to be rebuilt, the switch between the one-dispatch kernel and copy + scan + finish_order inside one feed, pops
shorter than the list, adsb_feed_ready, a close with launches in flight, CS16 through the dense and the short-buffer paths.

Everything goes through the C ABI and is compared with the CPU oracle byte for byte, every frame and every flag: in
per-buffer mode each buffer against the oracle on that buffer alone (and first_sample against the running sum), in carry
mode the concatenated pops against the oracle on the whole stream.  What a case relies on -- tiles over their quota,
frames straddling a cut, frame counts above and below a capacity -- is asserted from the oracle's lists first, so a change
of the synthetic generator cannot quietly turn these into sparse-traffic tests.  Every case prints one line: path, mode,
buffer sizes, frames compared."""
import os
import re
import time

import numpy as np
import pytest

import air_rs_amd as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I8, I16 = A.ADSB_SAMPLE_I8, A.ADSB_SAMPLE_I16
TILE = {I8: 16384, I16: 8192}
QUOTA = 32      # kQuota: a tile with more candidates takes its slots from the shared pool (none with pool_limit)
WINDOW = 240
NAME = {I8: "i8", I16: "i16"}
with open(os.path.join(ROOT, "air_rs_amd", "csrc", "adsb_kernels.h")) as _f:
    _TILES_PER_WG = re.search(r"constexpr\s+int\s+kFinishTilesPerWg\s*=\s*(\d+)\s*;", _f.read())
_REF = {}


def _limit(st):
    """The largest launch (samples) that still takes the one-dispatch kernel."""
    assert _TILES_PER_WG is not None, "kFinishTilesPerWg not found in adsb_kernels.h: the one-dispatch limit is unknown"
    return int(_TILES_PER_WG.group(1)) * TILE[st] + WINDOW


def _eq(got, want):
    assert len(got) == len(want), (len(got), len(want))
    if len(got):
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (bad[:5], got[bad[:3]], want[bad[:3]])


def _path(small):
    return "one-dispatch" if small == "1" else "three-kernels"


def _cached(key, make):
    """References are computed once, shared by the cases that need them, and never written to."""
    if key not in _REF:
        _REF[key] = make()
        for x in _REF[key]:
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    return _REF[key]


def _synth(st, seed, slot_len, n, amp_shift):
    cfg = A.synth_default(seed=seed, slot_len=slot_len)
    if st == I16:
        cfg.amp_shift = amp_shift
    return A.synth_fill_host(cfg, st, 0, 0, n)


def _per_buffer_refs(oracle, bufs):
    out = []
    for b in bufs:
        rc, want, n = oracle.process_buffer(b)
        assert rc == 0 and n == len(want)
        out.append(want)
    return out


def _check_per_buffer(bufs, refs, got):
    assert len(got) == len(bufs)
    pos = total = 0
    for b, want, (frames, flags, first) in zip(bufs, refs, got):
        assert flags == 0 and first == pos, (flags, first, pos)
        _eq(frames, want)
        pos += len(b)
        total += len(want)
    return total


# ---- 1, 2: two ring slots, dense buffers, the next buffer written into the slot before the pop ------------------------
DENSE_CHUNK, DENSE_BUFFERS, DENSE_LEN = 20_000, 12, 1500


def _dense_stream(oracle, st, carry):
    """12 buffers of 20 000 samples; every second one carries a constant stretch of 1500 samples (every offset of it is a
    frame), at another place in each, so that no two buffers that share a ring slot look alike anywhere.
    -> (stream, the oracle's lists: per buffer, or [the whole stream's])"""
    def make():
        data = _synth(st, 611, 500, DENSE_BUFFERS * DENSE_CHUNK, 5).copy()
        for k in range(1, DENSE_BUFFERS, 2):
            a = k * DENSE_CHUNK + 2000 + 1300 * (k // 2)
            data[a:a + DENSE_LEN] = (3, 4)
        if carry:
            rc, want, n = oracle.process_buffer(data)
            assert rc == 0 and n == len(want)
            refs = [want]
        else:
            refs = _per_buffer_refs(oracle, [data[k * DENSE_CHUNK:(k + 1) * DENSE_CHUNK] for k in range(DENSE_BUFFERS)])
        # the precondition: every dense buffer's LAUNCH has a tile with more than kQuota frames (so more candidates), which
        # loses its slots under pool_limit and is re-run from the launch's samples
        for k in range(1, DENSE_BUFFERS, 2):
            if carry:  # launch k covers the stream from 240 samples before the buffer; its offsets are absolute
                start = k * DENSE_CHUNK - WINDOW
                off = want["offset"].astype(np.int64)
                off = off[(off >= start) & (off < (k + 1) * DENSE_CHUNK - WINDOW)] - start
            else:
                off = refs[k]["offset"].astype(np.int64)
            per_tile = np.bincount(off // TILE[st])
            assert per_tile.max() > QUOTA and len(off) >= DENSE_LEN - WINDOW, (k, per_tile)
        return data, refs
    return _cached(("dense", st, carry), make)


def _run_two_slots_dense(oracle, st, small, carry):
    data, refs = _dense_stream(oracle, st, carry)
    chunk = DENSE_CHUNK
    bufs = [data[k * chunk:(k + 1) * chunk] for k in range(DENSE_BUFFERS)]
    got = []
    with A.AdsbDemod(sample_type=st, max_samples=chunk + WINDOW, max_out=1 << 14, host_staging=False) as d:
        d.pool_limit(True)
        try:
            with A.Feed(d, max_chunk=chunk, carry=carry, ring_slots=2) as f:
                for b in bufs:
                    if f.in_flight == 2:
                        # the slot of the OLDEST buffer in flight: the producer writes the next buffer into it at once,
                        # before that buffer is popped
                        slot = f.acquire()
                        slot[:chunk] = b
                        got.append(f.pop())
                        f.push_acquired(chunk)
                    else:
                        f.push(b)
                while f.in_flight:
                    got.append(f.pop())
        finally:
            d.pool_limit(False)
    if carry:
        assert len(got) == len(bufs) and all(fl == 0 for _, fl, _ in got)
        assert [first for _, _, first in got] == [k * chunk for k in range(len(bufs))]
        _eq(np.concatenate([fr for fr, _, _ in got]), refs[0])
        total = len(refs[0])
    else:
        total = _check_per_buffer(bufs, refs, got)
    print(f"\nfeed-edges two-slots-dense: path={_path(small)} mode={'carry' if carry else 'per-buffer'} {NAME[st]} "
          f"ring_slots=2 buffers={DENSE_BUFFERS}x{chunk} (every 2nd dense, pool off) frames compared={total}")


@pytest.mark.parametrize("carry", [False, True], ids=["per-buffer", "carry"])
@pytest.mark.parametrize("small", ["1", "0"])
def test_two_slots_dense_acquire_before_pop(gpu, oracle, monkeypatch, small, carry):
    """The rule of adsb_feed_cfg.ring_slots: a ring slot whose buffer went through the one-dispatch kernel is not handed
    out before that buffer is popped or its list is complete.  With two slots and two buffers in flight, acquire() returns
    the slot of the oldest, unpopped buffer; its launch lost slots (a constant stretch, the pool off) and is re-run from
    the slot's samples -- which the producer has replaced with the next buffer's by the time of the pop."""
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    _run_two_slots_dense(oracle, I8, small, carry)


@pytest.mark.parametrize("small", ["1", "0"])
def test_two_slots_dense_cs16(gpu, oracle, monkeypatch, small):
    """The same with CS16 samples (tiles of 8192 offsets, 4-byte samples), per-buffer mode."""
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    _run_two_slots_dense(oracle, I16, small, False)


# ---- 3: per-buffer mode, buffers on either side of the one-dispatch limit, two in flight -------------------------------
def _alternating(oracle, st):
    def make():
        n0 = _limit(st)
        sizes = [20_000, n0 + 1, 20_000, n0, n0 + 1, n0 + 1, 300, 20_000]
        data = _synth(st, 613, 500, sum(sizes), 5)
        cuts = np.concatenate([[0], np.cumsum(sizes)])
        bufs = [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        return data, sizes, _per_buffer_refs(oracle, bufs)
    return _cached(("alternating", st), make)


@pytest.mark.parametrize("ring_slots", [2, 3])
@pytest.mark.parametrize("st", [I8, I16], ids=["i8", "i16"])
def test_per_buffer_mode_alternates_paths(gpu, oracle, monkeypatch, st, ring_slots):
    """One feed, buffers just below, at and one sample above what the one-dispatch kernel takes: a small and a large launch
    in flight together, in either order, and one ring slot first read by a kernel (sequence word) and then by a DMA
    (event), and back."""
    monkeypatch.setenv("ADSB_SMALL_PATH", "1")
    data, sizes, refs = _alternating(oracle, st)
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    bufs = [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    got = []
    with A.AdsbDemod(sample_type=st, max_samples=max(sizes), max_out=1 << 15, host_staging=False) as d:
        with A.Feed(d, max_chunk=max(sizes), carry=False, ring_slots=ring_slots) as f:
            for b in bufs:
                f.push(b)
                if f.in_flight == 2:
                    got.append(f.pop())
            while f.in_flight:
                got.append(f.pop())
    total = _check_per_buffer(bufs, refs, got)
    assert total > 1000
    print(f"\nfeed-edges alternating-paths: path=one-dispatch up to {_limit(st)} samples, three-kernels above "
          f"mode=per-buffer {NAME[st]} ring_slots={ring_slots} buffers={sizes} frames compared={total}")


# ---- 4: carry mode, the one switch to copy + scan + finish_order ------------------------------------------------------
def _carry_switch(oracle, st):
    def make():
        n0 = _limit(st)
        sizes = [20_000, 20_000, n0 - WINDOW, n0 - WINDOW + 1, 20_000, 100, 20_000]
        data = _synth(st, 617, 500, sum(sizes), 4).copy()
        cuts = [int(c) for c in np.cumsum(sizes)[:-1]]
        # a frame across every cut: the 240 samples of a frame the oracle finds in the first buffer, copied so that they
        # begin `back` samples before the cut (the two cuts around the 100-sample buffer are 100 apart: their copies must
        # not overlap, and both must straddle)
        rc, first, n = oracle.process_buffer(data[:sizes[0]])
        assert rc == 0 and n > 0
        src = int(first["offset"][0])
        window = data[src:src + WINDOW].copy()
        for c, back in zip(cuts, [120, 120, 120, 120, 230, 80]):
            data[c - back:c - back + WINDOW] = window
        rc, want, n = oracle.process_buffer(data)
        assert rc == 0 and n == len(want)
        off = want["offset"].astype(np.int64)
        for c in cuts:  # the precondition: a frame that begins before the cut and ends behind it
            assert ((off > c - WINDOW) & (off < c)).any(), (c, cuts)
        return data, sizes, want
    return _cached(("carry-switch", st), make)


@pytest.mark.parametrize("producer", ["push", "acquire-2-slots"])
@pytest.mark.parametrize("st", [I8, I16], ids=["i8", "i16"])
def test_carry_mode_switches_to_three_kernels_once(gpu, oracle, monkeypatch, st, producer):
    """Carry mode: the third launch (tail + buffer) is the largest the one-dispatch kernel takes, the fourth is one sample
    longer -- its 240-sample tail travels from the pinned ring to a device staging slot, and from then on the tail lives on
    the device, so the small buffers that follow go through copy + scan + finish_order too.  The concatenated pops equal
    the oracle on the whole stream; a frame straddles each of the six cuts."""
    monkeypatch.setenv("ADSB_SMALL_PATH", "1")
    data, sizes, want = _carry_switch(oracle, st)
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    bufs = [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    parts, firsts = [], []
    with A.AdsbDemod(sample_type=st, max_samples=max(sizes) + WINDOW, max_out=1 << 15, host_staging=False) as d:
        with A.Feed(d, max_chunk=max(sizes), carry=True, ring_slots=2 if producer != "push" else 3) as f:
            def pop():
                frames, flags, first = f.pop()
                assert flags == 0
                parts.append(frames)
                firsts.append(first)
            for b in bufs:
                if producer == "push":
                    f.push(b)
                    if f.in_flight == 2:
                        pop()
                else:
                    if f.in_flight == 2:
                        pop()
                    slot = f.acquire()
                    slot[:len(b)] = b
                    f.push_acquired(len(b))
            while f.in_flight:
                pop()
    assert firsts == [int(c) for c in cuts[:-1]]
    _eq(np.concatenate(parts), want)
    assert len(want) > 1000
    print(f"\nfeed-edges carry-switch: path=one-dispatch for 3 launches, then three-kernels mode=carry {NAME[st]} "
          f"producer={producer} buffers={sizes} frames compared={len(want)}")


# ---- 5: carry mode, CS16, buffers shorter than the window --------------------------------------------------------------
def _ragged_cuts(n, rng, lo, hi):
    cuts, pos = [], 0
    while pos < n:
        step = int(rng.integers(lo, hi))
        cuts.append((pos, min(pos + step, n)))
        pos += step
    return cuts


@pytest.mark.parametrize("small", ["1", "0"])
def test_carry_mode_cs16_short_buffers(gpu, oracle, monkeypatch, small):
    """test_feed_carry_mode_equals_one_long_buffer's row of 1..599-sample buffers, with CS16 samples: tails shorter than
    240 samples of 4 bytes, starts aligned to 8 samples, frames spread over several buffers."""
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    st, lo, hi, n = I16, 1, 600, 60_000

    def make():
        data = _synth(st, 43, 500, n, 4)
        rc, want, cnt = oracle.process_buffer(data)
        assert rc == 0 and cnt == len(want)
        return data, want
    data, want = _cached(("short-cs16",), make)
    rng = np.random.default_rng(hi)
    cuts = _ragged_cuts(n, rng, lo, hi)
    assert min(b - a for a, b in cuts) < WINDOW < max(b - a for a, b in cuts)
    with A.AdsbDemod(sample_type=st, max_samples=hi + WINDOW, max_out=1 << 15, host_staging=False) as d:
        with A.Feed(d, max_chunk=hi, carry=True) as f:
            parts = []
            for (a, b) in cuts:
                f.push(data[a:b])
                if f.in_flight == 2:
                    parts.append(f.pop()[0])
            while f.in_flight:
                parts.append(f.pop()[0])
    _eq(np.concatenate(parts), want)
    assert len(want) > 50
    print(f"\nfeed-edges short-cs16: path={_path(small)} mode=carry i16 buffers={len(cuts)} of 1..599 samples "
          f"({n} in all) frames compared={len(want)}")


# ---- 6: pops shorter than the list ------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", ["1", "0"])
def test_short_pops(gpu, oracle, monkeypatch, small):
    """adsb_feed_pop with room for fewer frames than the buffer has (the host truncates), and a context with room for fewer
    (the device does): the first frames of the oracle's list, ADSB_FLAG_TRUNCATED exactly when something is missing, and
    nothing of it left for the buffers that follow."""
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    chunk = 40_000

    def make():
        data = _synth(I8, 619, 500, 2 * chunk, 0)
        return (data,) + tuple(_per_buffer_refs(oracle, [data[:chunk], data[chunk:]]))
    data, want_b, want_c = _cached(("short-pops-1",), make)
    buf_b, buf_c = data[:chunk], data[chunk:]
    n = len(want_b)
    assert n > 8 and len(want_c) > 8
    ks = [0, 1, n - 1, n, n + 1]
    pos = compared = 0
    with A.AdsbDemod(max_samples=chunk + WINDOW, max_out=1 << 14, host_staging=False) as d:
        with A.Feed(d, max_chunk=chunk, carry=False) as f:
            for k in ks:
                f.push(buf_b)
                f.push(buf_c)
                frames, flags, first = f.pop(max_out=k)         # (k = 0: no buffer at all)
                assert first == pos and flags == (A.ADSB_FLAG_TRUNCATED if k < n else 0), (k, n, flags)
                _eq(frames, want_b[:min(k, n)])
                frames, flags, first = f.pop()                  # the following buffer: whole, no flag
                assert first == pos + chunk and flags == 0, (k, flags)
                _eq(frames, want_c)
                pos += 2 * chunk
                compared += min(k, n) + len(want_c)
    print(f"\nfeed-edges short-pops host: path={_path(small)} mode=per-buffer i8 buffers=2x{chunk} per k, pop max_out k={ks} "
          f"of n={n} frames compared={compared}")

    # a context with room for 64 frames: buffers with more and with fewer, so that each of the two result sets holds a
    # truncated list and then a whole one
    cap, sizes = 64, [40_000, 20_000, 20_000, 40_000, 40_000, 20_000, 20_000, 40_000]

    def make2():
        data = _synth(I8, 621, 500, sum(sizes), 0)
        cuts = np.concatenate([[0], np.cumsum(sizes)])
        bufs = [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        return (data,) + tuple(_per_buffer_refs(oracle, bufs))
    ref2 = _cached(("short-pops-2",), make2)
    data, refs = ref2[0], ref2[1:]
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    bufs = [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    for size, want in zip(sizes, refs):
        assert (len(want) > cap) if size == 40_000 else (0 < len(want) < cap), (size, len(want))
    got = []
    with A.AdsbDemod(max_samples=max(sizes) + WINDOW, max_out=cap, host_staging=False) as d:
        with A.Feed(d, max_chunk=max(sizes), carry=False) as f:
            for b in bufs:
                f.push(b)
                if f.in_flight == 2:
                    got.append(f.pop())
            while f.in_flight:
                got.append(f.pop())
    assert len(got) == len(bufs)
    compared = 0
    for a, want, (frames, flags, first) in zip(cuts[:-1], refs, got):
        assert first == a and flags == (A.ADSB_FLAG_TRUNCATED if len(want) > cap else 0), (a, len(want), flags)
        _eq(frames, want[:cap])
        compared += min(len(want), cap)
    print(f"feed-edges short-pops device: path={_path(small)} mode=per-buffer i8 ctx max_out={cap} buffers={sizes} "
          f"oracle counts={[len(w) for w in refs]} frames compared={compared}")


# ---- 7: adsb_feed_ready -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", ["1", "0"])
def test_ready(gpu, oracle, monkeypatch, small):
    """adsb_feed_ready: ADSB_E_STATE with nothing in flight; true at some point after a push without anybody popping, and
    the pop then equals the oracle; a carry-mode buffer too short to launch anything is ready at once."""
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    chunk = 20_000

    def make():
        data = _synth(I8, 623, 500, chunk, 0)
        return (data,) + tuple(_per_buffer_refs(oracle, [data]))
    buf, want = _cached(("ready",), make)
    assert len(want) > 8
    with A.AdsbDemod(max_samples=chunk + WINDOW, max_out=1 << 14, host_staging=False) as d:
        with A.Feed(d, max_chunk=chunk, carry=False) as f:
            with pytest.raises(A.AdsbError) as e:
                f.ready
            assert e.value.code == A.ADSB_E_STATE
            t0 = time.perf_counter()
            f.push(buf)
            frames, flags, first = f.pop()
            blocking = time.perf_counter() - t0                 # what this buffer takes on this context, waiting included
            assert flags == 0 and first == 0
            _eq(frames, want)
            bound = max(2.0 * blocking, 5.0)
            f.push(buf)
            t0 = time.perf_counter()
            polls = 0
            while not f.ready:
                polls += 1
                assert time.perf_counter() - t0 < bound, (bound, polls)
            assert f.in_flight == 1                             # asking changes nothing
            frames, flags, first = f.pop()
            assert flags == 0 and first == chunk
            _eq(frames, want)
            with pytest.raises(A.AdsbError) as e:
                f.ready
            assert e.value.code == A.ADSB_E_STATE
        with A.Feed(d, max_chunk=chunk, carry=True) as f:
            f.push(buf[:100])                                   # fewer than 240 samples so far: no launch
            assert f.ready is True
            frames, flags, first = f.pop()
            assert len(frames) == 0 and flags == 0 and first == 0
    print(f"\nfeed-edges ready: path={_path(small)} mode=per-buffer, then carry i8 buffers=2x{chunk}, 100 "
          f"polls before ready={polls} frames compared={2 * len(want)}")


# ---- 8: close with launches in flight ---------------------------------------------------------------------------------
@pytest.mark.parametrize("carry", [False, True], ids=["per-buffer", "carry"])
@pytest.mark.parametrize("small", ["1", "0"])
def test_close_with_two_in_flight_then_reuse(gpu, oracle, monkeypatch, small, carry):
    """adsb_feed_close with two launches in flight waits for them, frees the ring they read and puts the stream base back
    to 0: the context then demodulates a buffer of its own with buffer-relative offsets, and a second feed on it starts at
    sample 0 with the first feed's first list."""
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    chunk = 20_000

    def make():
        data = _synth(I8, 627, 500, 4 * chunk, 0)
        return (data,) + tuple(_per_buffer_refs(oracle, [data[k * chunk:(k + 1) * chunk] for k in range(4)]))
    ref = _cached(("close",), make)
    data, refs = ref[0], ref[1:]
    bufs = [data[k * chunk:(k + 1) * chunk] for k in range(4)]
    assert all(len(w) > 8 for w in refs)
    with A.AdsbDemod(max_samples=chunk + WINDOW, max_out=1 << 14) as d:
        f = A.Feed(d, max_chunk=chunk, carry=carry)
        f.push(bufs[0])
        f.push(bufs[1])
        first_pop = f.pop()
        f.push(bufs[2])
        assert f.in_flight == 2
        f.close()
        assert first_pop[1] == 0 and first_pop[2] == 0
        _eq(first_pop[0], refs[0])                              # (a stream's first buffer: the same list in either mode)
        frames, flags = d.demod(bufs[3])
        assert flags == 0
        _eq(frames, refs[3])                                    # offsets from 0: no stream base left behind
        with A.Feed(d, max_chunk=chunk, carry=carry) as g:
            g.push(bufs[0])
            again = g.pop()
        assert again[1] == 0 and again[2] == 0
        _eq(again[0], first_pop[0])
        _eq(again[0], refs[0])
    print(f"\nfeed-edges close-in-flight: path={_path(small)} mode={'carry' if carry else 'per-buffer'} i8 "
          f"buffers=3x{chunk} fed (2 in flight at close), 1 demod, 1 fed again "
          f"frames compared={2 * len(refs[0]) + len(refs[3])}")
