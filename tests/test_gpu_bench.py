"""`bench.py --dump-outputs DIR` on the GPU: a small bench run writes the sequences of its last timed step, and a second run with
the same arguments writes the same values (every input of the bench is seeded).  A plain run's line carries the headline alone;
`--full` adds the other measurements."""
import json
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


# what a plain run's line must carry, and what only `--full` adds
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}
FULL_ONLY = {"stage_ms", "decode_tokens_per_sec_per_gpu", "decode_step_hbm", "rollout", "batched_videos", "roofline", "fp8_decode",
             "cpu_baseline"}
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--model", "3b", "--frames", "2", "--new-tokens", "16"]


def _bench_line(args):
    env = dict(os.environ, O3V_BENCH_SOLO_GROUP="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, env=env,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_plain_run_is_the_headline_only():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    rec = _bench_line(SMALL)
    assert HEADLINE <= rec.keys() and not (FULL_ONLY & rec.keys()), sorted(rec)
    assert rec["metric"] == "grounded_cot_tokens_per_sec" and rec["unit"] == "tokens/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["ms_per_step"] > 0 and rec["value"] == pytest.approx(16 * 1e3 / rec["ms_per_step"], rel=2e-3)


def test_bench_full_run_adds_the_extras():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    # the CPU baselines are left out here (tens of seconds on the host cores); every other part of --full runs at the small size
    rec = _bench_line([*SMALL, "--full", "--no-cpu-baseline", "--rollout-tokens", "16"])
    assert HEADLINE <= rec.keys() and FULL_ONLY - {"cpu_baseline"} <= rec.keys() and "cpu_baseline" not in rec, sorted(rec)
    assert rec["stage_ms"]["decode_ms"] > 0 and rec["rollout"]["G"] == 8 and rec["rollout"]["max_completion_length"] == 16
    assert rec["batched_videos"]["videos_per_step"] == 32 and rec["roofline"]["achieved"] > 0
    assert rec["fp8_decode"]["decode_ms_per_step"] > 0
