"""`bench.py --dump-outputs DIR` on the GPU: a small bench run writes the sequences of its last timed step, and a second run with
the same arguments writes the same values (every input of the bench is seeded)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 3B dims, 2 frames at 224x420 (S = 440 prompt tokens), 16 new tokens, headline leg only
ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--model", "3b", "--frames", "2", "--new-tokens", "16",
        "--no-cpu-baseline", "--no-batched", "--no-roofline", "--no-rollout", "--no-fp8"]


def _bench_dump(out_dir):
    env = dict(os.environ, O3V_BENCH_SOLO_GROUP="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.listdir(out_dir) == ["sequences.npy"]
    return np.load(os.path.join(out_dir, "sequences.npy"))


def test_bench_dump_outputs_repeat(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import bench
    from open_o3_video_amd.config import O3VConfig, qwen25vl_3b_dict
    cfg = O3VConfig.from_dict(qwen25vl_3b_dict())
    ids = bench.build_prompt(cfg, 2, (224 // 28) * (420 // 28), 2 * ((224 // 28) * (420 // 28) + 15) + 170)
    a = _bench_dump(tmp_path / "a")
    assert a.dtype == np.float64 and a.shape == (1, len(ids) + 16)
    assert np.array_equal(a[0, :len(ids)], ids)
    gen = a[0, len(ids):]
    assert (gen == np.round(gen)).all() and (gen >= 0).all() and (gen < cfg.text.vocab_size).all()
    b = _bench_dump(tmp_path / "b")
    assert np.array_equal(a, b)
