"""ms per step of the Casale GP-VAE step (svgp_vae_amd.GPVAE_Casale_model.CasaleStepEngine) per regime, with per-stage times
from HIP events, at the size of the reference's default run: N 4050, H 120, L 16, batch 256.  Rows are synthetic images on the
real (object, angle) structure of the train set (tests/golden/mnist_train_ids_mask.npz) with the PCA object vectors of the
golden inputs.  Information only: bench.py measures the flagship workload.

    python tools/casale_bench.py [--steps 200] [--warmup 20] [--out profiles/casale_bench.json]
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


def build_problem(L=16):
    gold = os.path.join(ROOT, "tests", "golden")
    mask = np.load(os.path.join(gold, "mnist_train_ids_mask.npz"))["train_ids_mask"].reshape(360, 15)
    gin = np.load(os.path.join(gold, "mnist_cfg2_inputs.npz"))
    rows = gin["train_aux"]
    ids, angles = np.sort(np.unique(rows[:, 0])), np.sort(np.unique(rows[:, 1]))
    jj, rr = np.nonzero(mask)
    N = len(jj)
    aux = np.stack([np.arange(N, dtype=np.float64), ids[jj], angles[rr]], 1)
    rng = np.random.RandomState(0)
    images = np.clip(0.142 + 0.316 * rng.randn(N, 28, 28, 1), -0.2, 1.2)
    return images, aux, gin["object_vectors"]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--L", type=int, default=16)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    from svgp_vae_amd.GPVAE_Casale_model import CasaleStepEngine, casaleGP
    from svgp_vae_amd.VAE_utils import mnistVAE
    images, aux, ov = build_problem(args.L)
    N = len(aux)
    GP = casaleGP(False, ov, False, True)
    eng = CasaleStepEngine(mnistVAE(L=args.L), GP, images, aux, batch_size=args.batch, beta=0.001, clipping_qs=True)
    dev = eng.dev
    eps_f = torch.randn(N, args.L, dtype=torch.float64, device=dev)
    eps_b = torch.randn(args.batch, args.L, dtype=torch.float64, device=dev)
    starts = [lo for lo in range(0, N - args.batch + 1, args.batch)]
    res = dict(N=N, H=eng.stage.H, L=args.L, batch=args.batch, steps=args.steps, warmup=args.warmup, regimes={})
    for regime in ("joint", "GP", "VAE"):
        run = lambda i: eng.step(regime, starts[i % len(starts)], starts[i % len(starts)] + args.batch, eps_full=eps_f,
                                 eps_batch=eps_b, adam=True)
        for i in range(args.warmup):
            run(i)
        eng.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            run(i)
        eng.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        eng.enable_stage_timing(True)
        acc = {}
        for i in range(args.steps):
            run(i)
            for k, v in eng.stage_times_ms().items():
                acc.setdefault(k, []).append(v)
        eng.enable_stage_timing(False)
        stages = {k: float(np.median(v)) for k, v in acc.items()}
        res["regimes"][regime] = dict(ms_per_step=ms, stage_ms_median=stages, elbo=eng.scalars()["elbo"])
        top = max(stages, key=stages.get)
        print(f"{regime}: {ms:.3f} ms/step; stages (median ms) " + ", ".join(f"{k} {v:.3f}" for k, v in stages.items()) +
              f"; largest: {top}", flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
