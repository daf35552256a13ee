"""GPU tests of bench.py's contract: the plain single-GPU line with its output dump, the `--full` line and the self-spawned
two-rank run (ranks share the one GPU of the test box over gloo: the control flow, the rank count and the gradient all-reduce
section are what is checked - the measured configuration is one rank per GPU over RCCL)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, extra_env=None, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra_env or {})
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_two_ranks_self_spawned():
    r = _run(["--gpus", "2", "--steps", "6", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-policy"], {"DRLGX_BENCH_BACKEND": "gloo"})
    assert r["n_gpus"] == 2 and r["ranks_in_process_group"] == 2 and r["collective_backend"] == "gloo"
    assert r["steps"] == 6 and r["scaling"] == "weak" and r["value"] > 0
    t = r["train_allreduce"]
    assert t["ranks"] == 2 and t["allreduce_ms"] > 0 and t["train_step_ms"] > t["allreduce_ms"] * 0.0
    assert t["env_steps_per_sec_while_training"] > 0
    assert "cpu_baseline" not in r  # N = 1 only


def test_bench_single_gpu_line():
    r = _run(["--steps", "10", "--warmup", "2", "--full", "--no-policy", "--no-cpu-baseline"])
    assert r["n_gpus"] == 1 and r["dtype"] == "f64" and r["unit"] == "env-steps/sec" and r["vs_baseline"] is None
    assert r["roofline"]["bound"] == "hbm" and 0 < r["roofline"]["frac"] < 1 and r["roofline"]["kernel"] == "k_step"
    assert r["train_allreduce"]["ranks"] == 1 and r["train_allreduce"]["allreduce_ms"] == 0.0


def test_bench_plain_line_and_output_dump(tmp_path):
    """A plain run times the headline steps and nothing else: the line holds the headline keys and none of `--full`'s sections.
    `--dump-outputs` writes the belief of the last timed step as finite float64 .npy files (one row per env, at most 64 MB in all),
    and a second run with the same arguments writes the same arrays."""
    dumps = []
    for k in range(2):
        d = tmp_path / ("out%d" % k)
        r = _run(["--steps", "7", "--warmup", "1", "--dump-outputs", str(d)])
        assert r["n_gpus"] == 1 and r["steps"] == 7 and r["warmup"] == 1 and r["dtype"] == "f64" and r["vs_baseline"] is None
        assert r["unit"] == "env-steps/sec" and r["higher_is_better"] is True and r["metric"].startswith("env-steps/sec")
        assert r["ms_per_step"] > 0 and r["value"] == pytest.approx(256 * 1e3 / r["ms_per_step"], rel=1e-9)
        assert not {"roofline", "kernels", "slam_path", "train_allreduce", "policy_path", "cpu_baseline"} & set(r)
        dumps.append({f.name: np.load(f) for f in sorted(d.glob("*.npy"))})
    a, b = dumps
    assert {"utility.npy", "metrics.npy", "pose_xyt.npy", "landmark_xy.npy", "vm_prob.npy", "vm_info.npy"} <= set(a) and set(a) == set(b)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert a["pose_xyt.npy"].shape == (256, 37, 3) and np.all(a["counts.npy"][:, 0] == 37)  # the snapshot's 36 poses + the timed step's
    nl = a["counts.npy"][:, 1].astype(int)
    assert a["landmark_xy.npy"].shape[1] == nl.max() and all(np.all(a["landmark_keys.npy"][i, nl[i]:] == -1) for i in range(256))
    for name, x in a.items():
        assert x.dtype == np.float64 and x.shape[0] == 256, name
        assert np.all(np.isfinite(x)), name
        np.testing.assert_array_equal(x, b[name], err_msg=name)
