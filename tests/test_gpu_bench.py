"""A plain `bench.py --steps K --warmup W` run: ONE block of exactly K timed steps, the headline fields and nothing of --full;
`--dump-outputs` writes the same arrays in every run with the same arguments, and --full times the same computation; any number
of steps stays finite."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], capture_output=True, text=True,
                       timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_plain_run_times_the_given_steps_and_dumps_reproducible_outputs(tmp_path):
    a, b, full = (str(tmp_path / d) for d in ("a", "b", "full"))
    line = _bench("--steps", "40", "--warmup", "5", "--dump-outputs", a)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 40 and line["repeats"] == 1 and len(line["block_ms"]) == 1 and line["dtype"] == "f64"
    assert abs(line["ms_per_step"] * 40 - line["block_ms"][0]) < 1e-2 and abs(line["value"] * line["ms_per_step"] - 1e3) < 1e-6
    assert not {"roofline", "stages_us", "cpu_baseline", "elbo"} & set(line)
    out = _load(a)
    assert {"scalar_elbo", "scalar_adam_t", "param_amplitude", "grad_amplitude"} <= set(out)
    assert all(v.dtype in (np.float32, np.float64) for v in out.values())
    assert sum(v.nbytes for v in out.values()) <= 64 << 20
    assert np.isfinite(out["scalar_elbo"]) and out["scalar_adam_t"] >= 45
    _bench("--steps", "40", "--warmup", "5", "--dump-outputs", b)
    again = _load(b)
    assert set(again) == set(out) and all(np.array_equal(out[k], again[k]) for k in out)
    # --full adds its parity gate before and its measurements after the timed region: the timed steps compute the same
    line = _bench("--steps", "40", "--warmup", "5", "--repeats", "1", "--full", "--no-cpu-baseline", "--dump-outputs", full)
    assert "roofline" in line and "stages_us" in line and line["elbo_rel_err_gpu_vs_oracle"] < 1e-3
    f = _load(full)
    assert set(f) == set(out) and all(np.array_equal(out[k], f[k]) for k in out)


@pytest.mark.gpu
def test_plain_run_of_many_steps_stays_finite(tmp_path):
    """More steps than the synthetic GECO problem survives in one go (~4 000): the restarts keep every timed step finite."""
    line = _bench("--steps", "6000", "--warmup", "10", "--dump-outputs", str(tmp_path))
    assert line["steps"] == 6000 and len(line["block_ms"]) == 1 and line["ms_per_step"] > 0
    out = _load(str(tmp_path))
    assert all(np.isfinite(v).all() for v in out.values())
    assert 1 <= out["scalar_adam_t"] <= 2000
