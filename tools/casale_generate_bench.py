"""ms per call of the Casale posterior cache build, of `generate` from it and of CasaleStepEngine.predict on the same rows, at
the size of the reference's default run: N 4050, Q 15, M 8 (H 120), L 16, T = 450 query rows.  Train rows are synthetic images
on the real (object, angle) structure of the train set with the PCA object vectors of the golden inputs (tools/casale_bench.py);
the query rows are train objects at uniform angles.  Information only: bench.py measures the flagship workload.

Each figure is a host clock around calls that end in a stream synchronise, after warm-up calls of the same shape; the three
are timed in alternation, `--repeats` windows each, and the median window and the spread are printed.

    python tools/casale_generate_bench.py [--calls 20] [--warmup 3] [--repeats 5] [--out profiles/casale_generate_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=450)
    ap.add_argument("--L", type=int, default=16)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    from casale_bench import build_problem
    from svgp_vae_amd import generate as G
    from svgp_vae_amd.GPVAE_Casale_model import CasaleStepEngine, casaleGP
    from svgp_vae_amd.VAE_utils import mnistVAE
    if not torch.cuda.is_available():
        raise SystemExit("casale_generate_bench needs a HIP device: a timing taken elsewhere says nothing")
    images, aux, ov = build_problem(args.L)
    N, L, T = len(aux), args.L, args.rows
    GP = casaleGP(False, ov, False, True)
    eng = CasaleStepEngine(mnistVAE(L=L), GP, images, aux, batch_size=256, beta=0.001, clipping_qs=True)
    dev = eng.dev
    rng = np.random.RandomState(0)
    torch.manual_seed(0)
    ids = aux[rng.randint(0, N, T), 1]
    q = torch.tensor(np.concatenate([np.stack([ids, rng.uniform(0, 2 * np.pi, T)], 1), ov[ids.astype(int)]], 1),
                     dtype=torch.float64, device=dev)
    test_images = torch.zeros(T, 28, 28, 1, dtype=torch.float64, device=dev)
    eps_f = torch.randn(N, L, dtype=torch.float64, device=dev)
    cache = eng.posterior_cache(eps_full=eps_f)
    work = dict(cache_build=lambda: eng.posterior_cache(eps_full=eps_f),
                generate=lambda: G.generate(cache, q),
                predict=lambda: eng.predict(test_images, q, take_mean=True, eps_full=eps_f))
    # the two paths compute the same images (take_mean): checked at the size that is timed
    a, b = work["generate"](), work["predict"]()[0]
    err = float((a - b).abs().max() / b.abs().max())
    windows = {k: [] for k in work}
    for k, f in work.items():
        for _ in range(args.warmup):
            f()
    for _ in range(args.repeats):
        for k, f in work.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                f()
            torch.cuda.synchronize()
            windows[k].append((time.perf_counter() - t0) * 1e3 / args.calls)
    res = dict(N=N, H=eng.stage.H, L=L, rows=T, calls=args.calls, repeats=args.repeats, route=G.route(cache),
               generate_vs_predict_relerr=err,
               ms_per_call={k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in windows.items()})
    for k, v in res["ms_per_call"].items():
        print(f"{k}: {v['median']:.3f} ms per call (windows {v['min']:.3f} .. {v['max']:.3f})", flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
