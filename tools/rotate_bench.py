"""Seconds to rotate N digits (28 x 28) to 16 angles: scipy.ndimage.rotate on the host, as the reference's generator does it
(utils.py:564-576), against svgp_vae_amd.utils.rotate_images (csrc/rotate.hip) including the upload of the digits and the copy
of the rotations back to the host, which is what generate_rotated_MNIST waits for.  N = 400 (--dataset 3) and 2000 (--dataset
13679).  Information only, no threshold; it needs a GPU and fails without one.

    python tools/rotate_bench.py [--reps 5] [--out profiles/rotate_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    from scipy import ndimage

    from svgp_vae_amd.utils import rotate_images
    angles = np.linspace(0, 360, 17)[:-1]
    rs = np.random.RandomState(0)
    rows = []
    for N in (400, 2000):
        x = rs.rand(N, 28, 28) * (rs.rand(N, 28, 28) < 0.2)
        t0 = time.perf_counter()
        ref = np.stack([np.stack([ndimage.rotate(im, a, reshape=False) for a in angles]) for im in x])
        t_scipy = time.perf_counter() - t0
        got = rotate_images(x, angles).cpu().numpy()                       # warm-up: code object load, allocator
        err = float(np.abs(got - ref).max())
        total, kernel = [], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = rotate_images(x, angles).cpu().numpy()                   # upload + kernel + copy back (the copy synchronises)
            total.append(time.perf_counter() - t0)
            d = torch.as_tensor(x, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rotate_images(d, angles)
            e1.record()
            torch.cuda.synchronize()
            kernel.append(e0.elapsed_time(e1) * 1e-3)                      # device events around the launch alone
        row = dict(N=N, rotations=N * len(angles), scipy_s=t_scipy, device_total_s=float(np.median(total)),
                   device_kernel_s=float(np.median(kernel)), max_abs_err=err, reps=args.reps)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return rows


if __name__ == "__main__":
    main()
