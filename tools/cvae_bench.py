"""us per training step of the VAE / CVAE step (svgp_vae_amd.CVAE_model.VaeStepEngine: two launches) at b = 256, L = 16, and beside
it, in the same call, the composed sequence of older entry points that the VAE regime of CasaleStepEngine issues for the same
plain-VAE step (ten entry points, a device copy, Adam, finalize).  That composed code is the yardstick; it is not changed by
the VAE / CVAE feature.  Information only: bench.py measures the flagship workload.

Every variant is warmed up, then timed in `--rounds` alternating windows of `--steps` steps each (device events around a window,
which ends in a synchronise); the figure is the median window, the spread its min .. max.  Before timing, the new VAE step and
the composed one are compared on the same rows and draws (elbo and every gradient).

    python tools/cvae_bench.py [--steps 200] [--rounds 5] [--warmup 20] [--out profiles/cvae_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--L", type=int, default=16)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/cvae_bench.py times HIP kernels and needs a GPU")
    from svgp_vae_amd.CVAE_model import VaeStepEngine, mnistCVAE
    from svgp_vae_amd.GPVAE_Casale_model import CasaleStepEngine, casaleGP
    from svgp_vae_amd.VAE_utils import mnistVAE
    b, L = args.batch, args.L
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    images = torch.tensor(np.clip(0.142 + 0.316 * rng.randn(b, 28, 28, 1), -0.2, 1.2), dtype=torch.float64, device=dev)
    obj, ang = np.repeat(np.arange(b // 8 + 1), 8)[:b], np.tile(np.arange(8) * 0.7, b // 8 + 1)[:b]
    aux3 = np.stack([np.arange(b, dtype=np.float64), obj.astype(np.float64), ang], 1)          # sorted [row, object, angle]
    aux2 = torch.tensor(aux3[:, 1:], dtype=torch.float64, device=dev).contiguous()
    eps = torch.randn(b, L, dtype=torch.float64, device=dev)
    new_vae = VaeStepEngine(mnistVAE(L=L, seed=1), b_max=b, lr=1e-3, store=False)
    new_cvae = VaeStepEngine(mnistCVAE(L=L, seed=1), b_max=b, lr=1e-3, store=False)
    GP = casaleGP(False, np.ones((int(obj.max()) + 1, 2)), False, True)
    old = CasaleStepEngine(mnistVAE(L=L, seed=1), GP, images, aux3, batch_size=b, beta=1.0, clipping_qs=False)
    # same rows, same draws, same parameters: the two plain-VAE steps must agree
    new_vae.step(images, aux2, eps, adam=False)
    old.step("VAE", 0, b, eps_batch=eps, adam=False)
    e_new, e_old = new_vae.scalars()["elbo"], old.scalars()["elbo"]
    g_new, g_old = new_vae.grads(), old.grads()
    gerr = max(float((g_new[k] - g_old[k]).abs().max() / g_old[k].abs().max()) for k in g_new)
    variants = dict(new_VAE=lambda: new_vae.step(images, aux2, eps, adam=True),
                    composed_VAE=lambda: old.step("VAE", 0, b, eps_batch=eps, adam=True),
                    new_CVAE=lambda: new_cvae.step(images, aux2, eps, adam=True))
    for run in variants.values():
        for _ in range(args.warmup):
            run()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, run in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(torch.cuda.current_stream(dev))
            for _ in range(args.steps):
                run()
            for eng in (new_vae, new_cvae, old):
                eng.synchronize()
            e1.record(torch.cuda.current_stream(dev))
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / args.steps)
    res = dict(batch=b, L=L, steps=args.steps, rounds=args.rounds, warmup=args.warmup, route=new_vae.route(),
               agreement=dict(elbo_new=e_new, elbo_composed=e_old, max_grad_relerr=gerr),
               us_per_step={k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in times.items()})
    res["ratio_composed_over_new_VAE"] = res["us_per_step"]["composed_VAE"]["median"] / res["us_per_step"]["new_VAE"]["median"]
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "wt"), indent=1)
    return res


if __name__ == "__main__":
    main()
