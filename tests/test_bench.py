"""bench.py: --steps is the number of timed steps, and --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _bench(args, timeout):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("steps,repeats,depth", [(1, 21, 32), (20, 21, 32), (1920, 21, 32), (4096, 21, 32), (100001, 21, 32),
                                                 (100000, 1, 32), (5000, 7, 4), (70000, 21, 1)])
def test_region_sizes_add_up_to_the_steps(steps, repeats, depth):
    sizes = bench.region_sizes(steps, repeats, depth)
    assert sum(sizes) == steps and 1 <= len(sizes) <= repeats
    assert all(n % depth == 0 for n in sizes[:-1])
    if len(sizes) > 1:
        assert min(sizes) >= bench.MIN_REGION_LAUNCHES * depth


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--dry-run"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr


def test_dump_outputs_samples_rows_beyond_the_cap(tmp_path):
    import torch
    y = torch.arange(64 * 200000, dtype=torch.float64).reshape(64, 200000)        # 102 MB
    info = bench.dump_outputs(str(tmp_path / "a"), y)
    bench.dump_outputs(str(tmp_path / "b"), y)
    p = tmp_path / "a" / "y.npy"
    assert os.path.getsize(p) <= 64 * 10 ** 6
    a, b = np.load(p), np.load(tmp_path / "b" / "y.npy")
    assert a.dtype == np.float64 and a.shape[0] == 64 and np.array_equal(a, b)        # the same sample every time
    rows = a[0].astype(np.int64)
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, y.numpy()[:, rows])
    assert info["shape"] == [64, 200000] and info["rows"].startswith("%d of 200000" % a.shape[1])
    small = torch.ones((3, 5), dtype=torch.float64)
    assert bench.dump_outputs(str(tmp_path / "c"), small)["rows"] == "all"
    assert np.array_equal(np.load(tmp_path / "c" / "y.npy"), small.numpy())


def test_dry_run_dumps_the_last_timed_step(tmp_path):
    # the dry run's problem, restated: a random 37 x 501 CSR (seed 7); rank 0's fields (seed 100) + 1e-3 * step index
    import scipy.sparse
    M = scipy.sparse.random(37, 501, density=0.05, random_state=np.random.default_rng(7), format="csr")
    x = np.random.default_rng(100).standard_normal((64, 501))
    steps, warmup = 3, 2
    outs = []
    for d in ("a", "b"):
        out = _bench(["--gpus", "1", "--dry-run", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / d)], 300)
        assert out["dump_outputs"]["shape"] == [64, 37] and out["gather_check"]["pass"]
        outs.append(np.load(tmp_path / d / "y.npy"))
    assert outs[0].dtype == np.float64 and outs[0].shape == (64, 37)
    assert np.array_equal(outs[0], (M @ (x + 1e-3 * (warmup + steps - 1)).T).T)
    assert not np.array_equal(outs[0], (M @ (x + 1e-3 * (warmup + steps - 2)).T).T)
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.gpu
def test_bench_dump_is_the_last_timed_step(tmp_path):
    """A small bench run: exactly --steps steps are timed, and y.npy is the apply of the last one's field batch (step
    warmup + steps - 1 of the rotation over the resident batches), against the oracle."""
    from icebin_amd import synthetic as syn
    from oracle import oracle as orc
    steps, warmup = 100, 7
    out = _bench(["--gpus", "1", "--config", "g20", "--steps", str(steps), "--warmup", str(warmup), "--repeats", "3",
                  "--no-cpu-baseline", "--no-extras", "--dump-outputs", str(tmp_path)], 900)
    assert out["steps"] == steps and sum(out["repeats"]["steps_per_region"]) == steps and out["ms_per_step"] > 0
    y = np.load(tmp_path / "y.npy")
    g = syn.make_grids("g20")
    o = orc.Regridder(g).matrix_d("AvI", syn.dome_elevmask(g), scale=True, correctA=True)
    nf, ncol = out["config"]["fields_per_gpu"], out["config"]["ncol_d"]
    b = (warmup + steps - 1) % out["config"]["field_batches"]
    x = syn.fields(nf, ncol, seed=syn.SEED)
    ref = o.apply(x if b == 0 else x + 1e-3 * b)
    assert y.dtype == np.float64 and y.shape == ref.shape == (nf, out["config"]["nrow_d"])
    assert np.max(np.abs(y - ref)) <= 1e-12 * np.max(np.abs(ref))
