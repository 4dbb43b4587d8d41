"""bench.py --dump-outputs / --full on one rank: the dump holds what the last timed step gave its
caller, two runs with the same arguments dump the same arrays, --steps sets the number of timed
steps, and --full is accepted."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(model, out_dir, *extra, env=None):
    env = {k: v for k, v in dict(os.environ, **(env or {})).items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", model,
                        "--steps", "3", "--warmup", "1", "--batch-per-gpu", "4", "--prompt-len", "16",
                        "--dump-outputs", str(out_dir), *extra], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    res = json.loads(lines[0])
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
    return res, arrays


def _check(res, arrays):
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["value"] > 0
    assert sorted(res["dumped_outputs"]) == sorted(arrays)
    assert arrays["seq_ids"].shape == (4,) and arrays["new_tokens"].shape == (4,)
    for v in arrays.values():
        assert v.dtype in (np.float32, np.float64) and np.isfinite(v).all()
    assert sum(v.nbytes for v in arrays.values()) <= 64 << 20


def test_dump_outputs_cpu(tmp_path):
    env = dict(OMP_NUM_THREADS="2", BFLY_FORCE_CPU="1")
    res, a = _bench("llama-tiny", tmp_path / "a", env=env)
    _check(res, a)
    assert sorted(a) == ["new_tokens", "seq_ids"]      # the CPU path keeps no logits
    res2, b = _bench("llama-tiny", tmp_path / "b", "--full", env=env)
    _check(res2, b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


@pytest.mark.gpu
def test_dump_outputs_gpu(tmp_path):
    """The hipGraph decode path also dumps its logits and the ids its sampler drew from them
    (greedy: a maximum of the row); a second run reproduces the tokens exactly and the logits to
    bf16 rounding."""
    from butterfly_amd.config import ModelConfig

    vocab = ModelConfig.from_preset("llama-small").vocab_size
    res, a = _bench("llama-small", tmp_path / "a")
    _check(res, a)
    assert res["config"]["hipgraph"] and res["config"]["async_decode"]
    assert a["logits"].shape == (4, vocab) and a["logits"].dtype == np.float32
    nxt = a["next_tokens"].astype(np.int64)
    assert nxt.shape == (4,) and ((0 <= nxt) & (nxt < vocab)).all()
    np.testing.assert_array_equal(a["logits"][np.arange(4), nxt], a["logits"].max(axis=-1))
    res2, b = _bench("llama-small", tmp_path / "b")
    for k in ("seq_ids", "new_tokens", "next_tokens"):
        np.testing.assert_array_equal(a[k], b[k])
    # same inputs, same kernels: only the order of split-K / atomic accumulation may differ, a
    # few bf16 ulps (2^-8 relative) of the logits' scale
    scale = np.abs(a["logits"]).max()
    assert np.abs(a["logits"] - b["logits"]).max() <= 4 * 2.0 ** -8 * scale
