"""bench.py's plain run and --dump-outputs: the plain line times exactly --steps steps in one region and carries nothing of --full;
the PCM of the last timed step is written as float32 and is the same from run to run (same arguments, same inputs), so two builds
can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_keeps_small_arrays_and_samples_large_ones_the_same_way(tmp_path):
    import bench
    small = np.arange(-6, 6, dtype=np.int16).reshape(3, 4)
    big = np.arange(10000, dtype=np.int16).reshape(10, 1000)
    bench.dump_outputs(str(tmp_path / "a"), {"small": small, "big": big}, 4096)
    bench.dump_outputs(str(tmp_path / "b"), {"big": big}, 4096)
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small)
    b1, b2 = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert b1.dtype == np.float32 and 0 < b1.nbytes <= 4096 and np.array_equal(b1, b2)
    assert np.all(np.diff(b1) > 0) and np.all(np.isin(b1, big))          # sorted distinct elements of the array


def _plain(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "PMR_DEBUG_POISON")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                        "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.nopoison
def test_plain_run_times_the_given_steps_and_dumps_the_same_pcm_every_run(tmp_path):
    d = _plain(tmp_path / "a")
    assert d["steps"] == 5 and d["timed_regions"]["n"] == 1 and d["timed_regions"]["steps_each"] == 5
    assert d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    for k in ("also", "roofline", "one_open_channel", "parity_checked", "host_io", "cpu_baseline"):
        assert k not in d, k
    assert os.listdir(tmp_path / "a") == ["pcm.npy"]
    pcm = np.load(tmp_path / "a" / "pcm.npy")
    assert pcm.dtype == np.float32 and pcm.shape[0] == 1024 and abs(pcm.shape[1] - d["config"]["frames_per_step"]) <= 1
    assert np.abs(pcm).max() > 100 and np.array_equal(pcm, np.round(pcm))
    _plain(tmp_path / "b")
    assert np.array_equal(pcm, np.load(tmp_path / "b" / "pcm.npy"))
