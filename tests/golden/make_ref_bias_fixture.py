"""BUILD CONTAINER ONLY.  Runs the reference's own `utils.compute_bias_variance_mean_estimators` (utils.py:922-948, numpy
only) on random inputs and stores inputs + returned values as tests/golden/ref_bias_fixture.npz.

    python tests/golden/make_ref_bias_fixture.py

The reference is imported the way make_ref_host_fixtures.py imports it (inert stand-ins for the modules this image lacks);
nothing of its source travels, only the arrays below.  tests/test_bias_host_cpu.py compares the product's
`svgp_vae_amd.utils.compute_bias_variance_mean_estimators` with them bit for bit.

Cases (B, L, m): (1, 1, 1), (3, 2, 5), (7, 16, 32).  The reference receives what its driver hands it
(MNIST_experiment.py:342, 358-362): a list of B lists of L arrays (m,), and a list of L arrays (m,).  It adds into the
arrays of the first step, so it gets copies and the stored inputs are the originals.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_ref_host_fixtures import import_reference  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_bias_fixture.npz")
CASES = [(1, 1, 1), (3, 2, 5), (7, 16, 32)]


def main():
    U, _ = import_reference()
    fx = {}
    for k, (B, L, m) in enumerate(CASES):
        rs = np.random.RandomState(100 + k)
        batch = rs.randn(B, L, m) * 3.0 + rs.randn(1, L, m)          # steps scatter around a common vector, like an epoch's
        full = batch.mean(0) + 0.05 * rs.randn(L, m)
        bias = U.compute_bias_variance_mean_estimators([[batch[b, l].copy() for l in range(L)] for b in range(B)],
                                                       [full[l].copy() for l in range(L)])
        fx[f"batch_{k}"], fx[f"full_{k}"], fx[f"bias_{k}"] = batch, full, np.float64(bias)
    np.savez_compressed(OUT, **fx)
    print("wrote", OUT, {k: np.asarray(v).shape for k, v in fx.items()})


if __name__ == "__main__":
    main()
