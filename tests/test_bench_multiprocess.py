"""The N>1 launch contract of bench.py (one process per GPU, barrier, MAX over ranks, one
all-gather of timings) exercised on CPU with the gloo backend, world_size 2."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(nproc, port):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
           "--gpus", str(nproc), "--steps", "5", "--warmup", "1", "--cpu-dry-run", "--full"]
    res = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "rank 0 must print exactly one JSON line"
    return json.loads(lines[0])


def test_two_ranks_gloo():
    out = _run(2, 29641)
    assert out["n_gpus"] == 2 and out["steps"] == 5 and out["scaling"] == "weak"
    # per-step sleep is 2 ms on rank 0 and 4 ms on rank 1: MAX over ranks must see the slow one
    assert out["ms_per_step"] >= 3.9
    # whole-job aggregate: both ranks' units over the max time
    assert abs(out["value"] - 2 * 5 / (out["ms_per_step"] * 5e-3)) < 1e-6 * out["value"]
    assert out["per_rank_ms"] == [[1.0, 2.0, 3.0], [2.0, 3.0, 4.0]]  # the single timing all-gather
    # the scaling curve's own denominator, measured in the same run (rank 0 alone between two barriers), and the fields that make a
    # slow box visible in the line
    assert abs(out["per_gpu_value"] - out["value"] / 2) < 1e-9 * out["value"]
    assert out["c5_shape_per_gpu"]["value"] > 0 and out["c5_shape_per_gpu"]["steps"] == 3
    assert abs(out["efficiency_vs_c5_shape_per_gpu"] - out["per_gpu_value"] / out["c5_shape_per_gpu"]["value"]) < 1e-9
    # rank 0 alone sleeps 2 ms per step, the pair is paced by rank 1's 4 ms: the dry run's "efficiency" is about one half
    assert 0.3 < out["efficiency_vs_c5_shape_per_gpu"] < 0.7
    for key in ("ms_per_factorize", "ms_per_factorize_min", "ms_per_factorize_median"):
        assert key in out
    assert set(out["clocks"]) == {"before_timed_region", "after_timed_region"}


def test_single_rank_no_process_group():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-dry-run", "--steps", "3",
                          "--warmup", "1"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][0])
    assert out["n_gpus"] == 1 and out["metric"].startswith("IP iterations/sec")


def test_self_spawn_without_launcher():
    """`python bench.py --gpus 2` with no WORLD_SIZE in the environment starts its own two ranks
    (the command the driver would issue must not exit with "launch with torch.distributed.run")
    and defaults to BASELINE config C5's 16 instances per GPU."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--cpu-dry-run", "--steps", "3",
                          "--warmup", "1", "--full"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["batch_per_gpu"] == 16
    assert out["per_rank_ms"] == [[1.0, 2.0, 3.0], [2.0, 3.0, 4.0]]


def test_batch_defaults():
    sys.path.insert(0, ROOT)
    import bench
    old = sys.argv
    try:
        sys.argv = ["bench.py"]
        assert bench.parse_args().batch == 1
        sys.argv = ["bench.py", "--gpus", "8"]
        assert bench.parse_args().batch == 16
        sys.argv = ["bench.py", "--gpus", "8", "--batch", "4"]
        assert bench.parse_args().batch == 4
    finally:
        sys.argv = old


HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}


def test_plain_run_prints_the_headline_only():
    """Without --full the line carries the headline and the run's description, none of the measurements that take runs of their own
    (per-phase timings, clocks, the solo C5-shape phase of N > 1)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--cpu-dry-run", "--steps", "4",
                          "--warmup", "1"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert HEADLINE <= set(out) and out["steps"] == 4 and out["n_gpus"] == 2
    assert abs(out["value"] - 2 * 4 / (out["ms_per_step"] * 4e-3)) < 1e-6 * out["value"]
    for key in ("per_rank_ms", "ms_per_factorize", "clocks", "c5_shape_per_gpu", "per_gpu_value", "roofline"):
        assert key not in out, key


def test_dump_outputs_is_refused_by_the_dry_run():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-dry-run", "--steps", "2", "--dump-outputs",
                          os.path.join(ROOT, "unused")], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert res.returncode != 0 and "--dump-outputs" in res.stderr
    assert not os.path.exists(os.path.join(ROOT, "unused"))


def test_write_outputs_float64_within_budget_and_reproducible(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(5)
    arrays = {"x": rng.standard_normal(1000), "inertia": np.array([7, 0, 0]), "kkt_nzval": rng.standard_normal(3000).astype(np.float32)}
    # under the budget: every array whole, as float64
    assert bench.write_outputs(str(tmp_path / "a"), arrays) == {"x": 1000, "inertia": 3, "kkt_nzval": 3000}
    for k, v in arrays.items():
        got = np.load(tmp_path / "a" / f"{k}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, v.astype(np.float64))
    # over the budget: the same fraction of every array, a fixed sample (same files twice), at most the budget in all
    n1 = bench.write_outputs(str(tmp_path / "b"), arrays, budget_bytes=8 * 2000)
    n2 = bench.write_outputs(str(tmp_path / "c"), arrays, budget_bytes=8 * 2000)
    assert n1 == n2 and 8 * sum(n1.values()) <= 8 * 2000 and n1 == {"x": 1000 * 2000 // 4003, "inertia": 3 * 2000 // 4003, "kkt_nzval": 3000 * 2000 // 4003}
    for k in arrays:
        b, c = np.load(tmp_path / "b" / f"{k}.npy"), np.load(tmp_path / "c" / f"{k}.npy")
        assert b.dtype == np.float64 and np.array_equal(b, c)
        assert np.isin(b, arrays[k].astype(np.float64)).all()


@pytest.mark.gpu
def test_plain_gpu_run_dumps_what_the_last_step_computed(tmp_path):
    """`bench.py --steps 2 --warmup 1 --dump-outputs DIR` on the GPU: a headline-only line, and the files hold the last step's
    solution, inertia and KKT values -- the dumped x solves the dumped matrix for the bench's right-hand side."""
    from madnlp_jl_amd.problems import OPF_CASES, opf_shaped
    from oracle.sparse_condensed import SparseCondensedKKTSystem as OracleSC
    d = tmp_path / "out"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert HEADLINE <= set(out) and out["steps"] == 2 and out["dtype"] == "f64" and out["higher_is_better"] is True
    assert "roofline" not in out and "cpu_baseline" not in out and "ms_per_factorize" not in out
    assert sorted(os.listdir(d)) == ["inertia.npy", "kkt_nzval.npy", "x.npy"]
    seed = OPF_CASES["case1354pegase"][0]
    P = opf_shaped("case1354pegase", seed=seed, du=1e-8)
    x, inertia, nz = (np.load(d / f"{k}.npy") for k in ("x", "inertia", "kkt_nzval"))
    assert x.dtype == inertia.dtype == nz.dtype == np.float64
    assert inertia.tolist() == [P.n, 0, 0]
    ko = OracleSC(P.n, P.m, P.jac_I, P.jac_J, P.hess_I, P.hess_J, P.ind_ineq, P.ind_lb, P.ind_ub, lambda A: None)
    import scipy.sparse as sp
    Kl = sp.csc_matrix((nz, ko.aug_com.rowval, ko.aug_com.colptr), shape=(P.n, P.n))
    K = Kl + sp.tril(Kl, -1).T
    b = np.random.default_rng(seed).standard_normal(P.n)
    res = np.abs(K @ x - b).max() / (abs(K).sum(1).max() * np.abs(x).max() + np.abs(b).max())
    assert res < 1e-12, res
