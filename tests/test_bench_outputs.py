"""bench.py's --dump-outputs writer and its flags (CPU tier): the frame list goes out as float arrays, whole or as a fixed
sample within the byte budget."""
import os

import numpy as np


def _frames(lib, n):
    f = np.zeros(n, dtype=lib.FRAME_DTYPE)
    f["offset"] = np.arange(n, dtype=np.uint64) * 2000 + 17
    f["bytes"] = (np.arange(n * 14) % 251).reshape(n, 14)
    f["status"] = np.arange(n) % 2
    f["fixed_bit"] = np.where(np.arange(n) % 3 == 0, 255, np.arange(n) % 112)
    return f


def test_plain_by_default_full_and_dump_on_request(lib):
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_whole_list(lib, tmp_path):
    import bench
    f = _frames(lib, 1000)
    bench.dump_outputs(str(tmp_path), f, 1003, 0)
    got = {n[:-4]: np.load(os.path.join(tmp_path, n)) for n in os.listdir(tmp_path)}
    assert set(got) == {"frame_offset", "frame_bytes", "frame_status", "frame_fixed_bit", "counts"}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert got["frame_offset"].dtype == np.float64 and (got["frame_offset"] == f["offset"]).all()
    assert got["frame_bytes"].shape == (1000, 14) and (got["frame_bytes"] == f["bytes"]).all()
    assert (got["frame_status"] == f["status"]).all() and (got["frame_fixed_bit"] == f["fixed_bit"]).all()
    assert got["counts"].tolist() == [1000, 1003, 0]


def test_dump_outputs_samples_a_long_list_within_budget(lib, tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)
    f = _frames(lib, 50_000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), f, 50_000, 0, channel_counts=[20_000, 30_000])
    size = sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a"))
    assert size <= 200_000
    idx = np.load(tmp_path / "a" / "frame_index.npy")
    assert 0 < len(idx) < 50_000 and (np.diff(idx) > 0).all()
    assert (np.load(tmp_path / "a" / "frame_offset.npy") == f["offset"][idx.astype(np.int64)]).all()
    assert np.load(tmp_path / "a" / "counts.npy").tolist() == [50_000, 50_000, 0]
    assert np.load(tmp_path / "a" / "channel_counts.npy").tolist() == [20_000, 30_000]
    for n in os.listdir(tmp_path / "a"):   # the same sample every time
        assert (np.load(tmp_path / "a" / n) == np.load(tmp_path / "b" / n)).all(), n
