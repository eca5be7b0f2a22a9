"""Records tests/golden/stage_batched_<b>_<m>_<L>.npz for tests/test_gpu_stage_batched.py: theta, the state vector, every gradient and
the scalars after three Adam steps at each of the test's shapes, from the library built in THIS checkout, on the GPU.

The fixtures are the results of the commit BEFORE the batched staging, so the script refuses to run unless `git rev-parse HEAD` of
the checkout it stands in is that commit (copy this file and tests/test_gpu_stage_batched.py into a checkout of it, build, run).
usage: python tools/make_stage_batched_golden.py [output directory, default tests/golden]"""
import os
import subprocess
import sys

PARENT = "3aa483baf90402e9a95784a55cd9c17b5e33680d"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
    if head.returncode != 0 or not head.stdout.strip().startswith(PARENT):
        sys.exit(f"refusing to record: HEAD of {ROOT} is {head.stdout.strip() or head.stderr.strip()!r}, not the parent commit {PARENT}")
    import numpy as np

    from tests import test_gpu_stage_batched as T
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    os.makedirs(out, exist_ok=True)
    for b, m, L in T.SHAPES:
        _, got = T.three_steps(b, m, L)
        path = os.path.join(out, os.path.basename(T.golden_path(b, m, L)))
        np.savez(path, **got)
        print(f"{path}: {os.path.getsize(path)} bytes, elbo {float(got['sc_elbo'])!r}", flush=True)


if __name__ == "__main__":
    main()
