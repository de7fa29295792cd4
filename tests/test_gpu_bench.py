"""bench.py's plain run on the GPU: the headline line without the --full extras, exactly --steps timed steps, and
--dump-outputs writing the last step's frame list, which must be what the CPU oracle finds in the same synthetic buffer."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import air_rs_amd as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_frames(gpu, oracle, tmp_path):
    n = 1 << 22
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--samples", str(n), "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 7 and d["ms_per_step"] > 0 and d["value"] > 0 and d["higher_is_better"] is True
    assert d["unit"] == "Msamples/s" and d["dtype"] == "i8"
    for k in ("roofline", "cold_start", "per_rank", "feed", "cpu_baseline", "parity_check"):
        assert k not in d, k
    iq = A.synth_fill_host(A.synth_default(), A.ADSB_SAMPLE_I8, 0, 0, n)
    rc, want, found = oracle.process_buffer(iq)
    assert rc == 0 and found == len(want) == d["config"]["frames_per_step"] > 0
    for name in os.listdir(tmp_path):
        assert np.load(tmp_path / name).dtype in (np.float32, np.float64), name
    assert np.load(tmp_path / "counts.npy").tolist() == [found, found, 0]
    assert (np.load(tmp_path / "frame_offset.npy") == want["offset"]).all()
    assert (np.load(tmp_path / "frame_bytes.npy") == want["bytes"]).all()
    assert (np.load(tmp_path / "frame_status.npy") == want["status"]).all()
    assert (np.load(tmp_path / "frame_fixed_bit.npy") == want["fixed_bit"]).all()
