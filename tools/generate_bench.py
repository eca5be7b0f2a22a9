"""Conditional generation on rotated MNIST: the existing predict path against the posterior cache, per query batch.

  (a) bacthing_predict_SVGPVAE_rotated_mnist per query batch: kernel matrices and statistics over all N train rows, the factor
      stage, the row stage and the decoder (an engine sized for max(N, batch) rows; a call takes at most N query rows, so a
      batch of more rows is two calls of half of them)
  (b) PosteriorCache.build once (device-resident train rows in chunks of --chunk; it contains the encoder over all N rows, so
      (a) is charged the train encodings once as well: `encode_train_s`), with the construction of its private engine and the
      host-to-device copy of the train images timed on their own, then
  (c) generate per query batch (m <= 64: one launch; no train row)

at the config-2 shape (N = 4050, m = 32, L = 16, M = 8) and at m = 256, M = 32, N = 16384, for query batches of 256 and 4096 rows.
(a) and (c) alternate inside one process, every call ends in a stream synchronise, medians over --reps calls after a warm-up of
each shape.  Also, without touching the GPU: the engine workspace at b_max = chunk against b_max = N (svgp_mnist_ws_layout_get).
Information only, no threshold; the timings need a GPU and fail without one.

    python tools/generate_bench.py [--reps 20] [--chunk 1024] [--out profiles/generate_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/generate_bench.py --build-only --reps 10
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [dict(name="config 2", N=4050, m=32, L=16, M=8, n_obj=400), dict(name="m = 256", N=16384, m=256, L=16, M=32, n_obj=400)]
QUERY_ROWS = (256, 4096)


def workspace_bytes(sh, b_max):
    from svgp_vae_amd._lib import MnistCfg, WsLayout, call
    wl = WsLayout()
    cfg = MnistCfg(b=b_max, b_global=b_max, b_cap=b_max, m=sh["m"], L=sh["L"], M=sh["M"], n_obj=sh["n_obj"], clip_qs=1,
                   train_ip=1, train_gp=1, train_ov=1, N_train=float(sh["N"]), jitter=1e-6, kappa_squared=0.02, alpha=0.99,
                   rep_weight=1.0)
    call("svgp_mnist_ws_layout_get", C.byref(cfg), C.byref(wl))
    return 8 * int(wl.total)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--build-only", dest="build_only", action="store_true",
                    help="--reps cache builds per shape and nothing else: the program of a `rocprofv3 --kernel-trace --stats` run")
    args = ap.parse_args(argv)
    rows = []
    for sh in SHAPES:
        row = dict(shape=sh["name"], N=sh["N"], m=sh["m"], L=sh["L"], M=sh["M"], chunk=args.chunk,
                   ws_bytes_chunk=workspace_bytes(sh, args.chunk), ws_bytes_N=workspace_bytes(sh, sh["N"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if not torch.cuda.is_available():
        raise SystemExit("the timings need a GPU")
    from svgp_vae_amd import generate as G
    from svgp_vae_amd.engine import MnistStepEngine
    from svgp_vae_amd.SVGPVAE_model import bacthing_predict_SVGPVAE_rotated_mnist, batching_encode_SVGPVAE, mnistSVGP
    from svgp_vae_amd.VAE_utils import mnistVAE
    for sh in SHAPES:
        rs = np.random.RandomState(0)
        N, m, L, M, n_obj = sh["N"], sh["m"], sh["L"], sh["M"], sh["n_obj"]
        rows_of = lambda n: np.hstack([rs.randint(0, n_obj, (n, 1)).astype(float), rs.rand(n, 1) * 6.28, np.zeros((n, M))])
        ip = np.hstack([np.arange(m)[:, None].astype(float), rs.rand(m, 1) * 6.28, rs.randn(m, M) * 1.5])
        vae = mnistVAE(L=L)
        svgp = mnistSVGP(False, False, ip, False, rs.randn(n_obj, M) * 1.5, "main", 1e-6, float(N), L)
        img = torch.as_tensor(np.clip(0.142 + 0.316 * rs.randn(N, 28, 28, 1), 0, 1))
        aux = torch.as_tensor(rows_of(N))
        d_img, d_aux = img.cuda(), aux.cuda()

        def encode():                                                  # what (a) needs before its first batch: the train encodings
            mu, var = [], []
            for lo in range(0, N, 1024):
                a, b, _ = batching_encode_SVGPVAE((d_img[lo:lo + 1024], d_aux[lo:lo + 1024]), vae, clipping_qs=True)
                mu.append(a); var.append(b)
            return torch.cat(mu), torch.cat(var)

        # (b): device-resident train rows in, as (a) gets them; the encoder over all N rows is inside the build, so (a) is charged
        # `encode` once as well.  The pieces of the build's host side are timed on their own: the private engine it constructs
        # (workspace of `chunk` rows zero-filled, stream, parameter copy) and, for a caller that holds the rows on the host, the copy.
        build = lambda: G.PosteriorCache.build(vae, svgp, d_img, d_aux, chunk=args.chunk)
        engine = lambda: MnistStepEngine(m, L, M, n_obj, N_train=float(N), b_max=min(args.chunk, N))
        mu, var = encode()
        cache = build()
        engine()
        if args.build_only:                                            # for a kernel trace of the build alone
            for _ in range(args.reps):
                build()
            torch.cuda.synchronize()
            continue
        enc_s, build_s, eng_s, h2d_s = [], [], [], []
        for _ in range(args.reps):
            enc_s.append(timed(encode)); build_s.append(timed(build)); eng_s.append(timed(engine))
            h2d_s.append(timed(lambda: img.cuda()))
        med = lambda v: float(np.median(v))
        for q in QUERY_ROWS:
            qa = torch.as_tensor(rows_of(q))
            eps = torch.as_tensor(rs.randn(q, L))
            zeros = torch.zeros(q, 28, 28, 1, dtype=torch.float64, device="cuda")
            d_qa, d_eps = qa.cuda(), eps.cuda()
            # the existing path takes at most N query rows per call (b <= b_global): more rows are two calls of half of them
            step = q if q <= N else q // 2
            old = lambda: torch.cat([bacthing_predict_SVGPVAE_rotated_mnist((zeros[lo:lo + step], d_qa[lo:lo + step]), vae, svgp, mu,
                                                                            var, d_aux, epsilon=d_eps[lo:lo + step])[0]
                                     for lo in range(0, q, step)])
            new = lambda: G.generate(cache, d_qa, eps=d_eps)
            ra, rn = old(), new()                                     # warm-up of both paths at this shape; and the same images
            err = float((ra - rn).abs().max() / ra.abs().max())
            ta, tc = [], []
            for _ in range(args.reps):                                # alternating, as two versions are compared in one call
                ta.append(timed(old)); tc.append(timed(new))
            a_s, c_s = med(ta), med(tc)
            # batches k from which build + k generate <= encode + k predict (0: from the first batch on)
            ahead = max(0.0, (med(build_s) - med(enc_s)) / max(a_s - c_s, 1e-12))
            row = dict(shape=sh["name"], N=N, m=m, L=L, M=M, query_rows=q, predict_calls=q // step, reps=args.reps, rel_diff_images=err,
                       predict_call_s=a_s, predict_call_min_s=float(np.min(ta)), predict_images_per_s=q / a_s,
                       generate_call_s=c_s, generate_call_min_s=float(np.min(tc)), generate_images_per_s=q / c_s,
                       encode_train_s=med(enc_s), cache_build_s=med(build_s), cache_build_min_s=float(np.min(build_s)),
                       engine_construct_s=med(eng_s), train_images_h2d_s=med(h2d_s),
                       batches_until_build_is_ahead=ahead, route=G.route(cache))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return rows


if __name__ == "__main__":
    main()
