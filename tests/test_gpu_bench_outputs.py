"""``bench.py --dump-outputs`` on the HIP kernels: a plain run (no ``--full``) of the N = 1
full-batch line and of the cfg5 mini-batch line writes the last timed step's loss, parameters,
gradients and (full batch) a row sample of both embedding tables; two runs with the same
arguments start from the same inputs, so their files agree to float32 summation-order noise
(the scatter kernels add with atomics)."""
import json

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

LR = 1e-3   # bench.py's Adam


def _run(tmp_path, tag, argv):
    out = tmp_path / f"{tag}.json"
    bench.main(argv + ["--dump-outputs", str(tmp_path / tag), "--json-out", str(out)])
    line = json.loads(out.read_text())
    return line, {f.name[:-len(".npy")]: np.load(f) for f in (tmp_path / tag).iterdir()}


def _check_pair(runs, steps):
    (la, a), (lb, b) = runs
    assert a.keys() == b.keys()
    for line, files in runs:
        assert line["steps"] == steps and line["ms_per_step"] > 0
        assert line["kernels"] == {} and line["roofline"] is None and line["cpu_baseline"] is None
        assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all()
                   for v in files.values())
        assert sum(v.nbytes for v in files.values()) <= 64 * 2 ** 20
        assert float(files["loss"][0]) == line["loss"]
    for n in a:
        if n.startswith("param."):
            # Adam moves a parameter by at most ~lr per step whatever its gradient's size, so a
            # gradient that is rounding noise around zero may move it either way
            np.testing.assert_allclose(b[n], a[n], rtol=0, atol=2 * LR * (steps + 1))
        else:
            scale = float(np.abs(a[n]).max()) or 1.0
            np.testing.assert_allclose(b[n], a[n], rtol=1e-4, atol=1e-5 * scale)


def test_full_batch_dump_is_reproducible(tmp_path):
    argv = ["--config", "cfg2", "--scale", "0.02", "--steps", "2", "--warmup", "1"]
    runs = [_run(tmp_path, t, argv) for t in ("a", "b")]
    _check_pair(runs, 2)
    files = runs[0][1]
    cfg = bench.synth.scaled("cfg2", 0.02)
    # the embedding tables: a fixed sample of DUMP_SAMPLE_ROWS rows of the larger one
    assert files["out.user"].shape == (min(cfg.num_users, bench.DUMP_SAMPLE_ROWS), cfg.hidden)
    assert files["out.post"].shape == (min(cfg.num_posts, bench.DUMP_SAMPLE_ROWS), cfg.hidden)
    assert cfg.num_users > bench.DUMP_SAMPLE_ROWS       # the sampling path ran
    assert sum(n.startswith("param.") for n in files) == 12
    assert all("grad." + n[len("param."):] in files for n in files if n.startswith("param."))
    assert any(np.abs(files[n]).max() > 0 for n in files if n.startswith("grad."))


def test_minibatch_dump_is_reproducible(tmp_path):
    argv = ["--config", "cfg5", "--scale", "0.005", "--batch-seeds", "128", "--steps", "4",
            "--warmup", "1"]
    runs = [_run(tmp_path, t, argv) for t in ("a", "b")]
    _check_pair(runs, 4)
    files = runs[0][1]
    assert sum(n.startswith("param.") for n in files) == 24    # 2 layers x 4 relations x 3
    assert any(np.abs(files[n]).max() > 0 for n in files if n.startswith("grad."))
