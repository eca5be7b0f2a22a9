"""SPRITES: the GP stage of animating a new character, existing path against the one-launch entry, per batch of target rows.

  (a) approximate_posterior_params_precomputed_GP_posterior_params, then the clamp, square root and draw of
      predict_SVGPVAE_sprites_test_character in torch: kernel matrices, X = Sigma^-1 - K_mm^-1 rebuilt, the batched GEMM into the
      (L, b, m) product, the (L, b, m) element-wise product and its row sums, the element-wise tail
  (b) the same kernel matrices, then ONE call of svgp_sprites_posterior_rows on X formed once (the posterior cache of animate.py)

at (m = 72, L = 64) and (m = 800, L = 64) for 288 target rows (4 test characters x 72 actions).  (a) and (b) alternate inside one
process, every call ends in a device synchronise, medians over --reps calls after a warm-up of each; the kernel matrices both
share are timed on their own as well, and the new entry alone between device events (its achieved FP64 rate: 2 b m^2 L flops,
against L m^2 doubles of X read).  The outputs of the two are compared at the timed size.  Information only, no threshold; needs a
GPU and fails without one.

    python tools/animate_bench.py [--reps 50] [--out profiles/animate_bench.json]
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

SHAPES = [dict(m=72, L=64), dict(m=800, L=64)]
ROWS, LA, LC, N_ACT = 288, 8, 16, 72
CLIP = (1e-4, 100.0)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("the timings need a GPU")
    from svgp_vae_amd import _lib
    from svgp_vae_amd import animate as A
    from svgp_vae_amd import sprites as S
    rows = []
    for sh in SHAPES:
        m, L, b = sh["m"], sh["L"], ROWS
        rs = np.random.RandomState(0)
        svgp = S.spritesSVGP(False, True, rs.randn(m, LA + LC) * 1.5, "main", 0.01, 50000.0, LA, rs.randn(N_ACT, LA) * 1.5, LC, L,
                             K_SE=True)
        eng = S.SpritesStepEngine(S.spritesVAE(L), S.sprites_representation_network(LC), svgp, b_max=b, seg_len=1,
                                  params=dict(se=torch.tensor([5.0, 1.4, 7.0, 1.2], dtype=torch.float64)))
        svgp._engine = eng
        dev = eng.dev
        t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev).contiguous()
        aux = t(np.hstack([rs.randint(0, N_ACT, (b, 1)).astype(float), rs.randn(b, LC) * 1.5]))
        mt = t(rs.randn(L, m))
        # Sigma^-1 and K_mm^-1 stand-ins of the right size: X = Si - Ki of order 1 / m, so that p_v stays inside the clip range
        Si, Ki = t(rs.randn(L, m, m) / m), t(rs.randn(m, m) / m)
        eps = t(rs.randn(b, L))
        X = (Si - Ki[None]).contiguous()                      # formed once: what the posterior cache holds
        cfg = _lib.PosteriorRowsCfg(b=b, m=m, L=L, clip_lo=CLIP[0], clip_hi=CLIP[1])
        p_m, p_v, z = (torch.empty(b, L, dtype=torch.float64, device=dev) for _ in range(3))
        n_work = int(_lib.load_library().svgp_sprites_posterior_rows_workspace_elems(C.byref(cfg)))
        work = torch.empty(max(n_work, 1), dtype=torch.float64, device=dev)

        def old():
            pm, B = S.approximate_posterior_params_precomputed_GP_posterior_params(svgp, aux, mt, Si, Ki, engine=eng)
            pv = torch.clamp(B, *CLIP)
            return pm, pv, pm + eps * torch.sqrt(pv)

        def entry(Kb, kbb, stream):
            _lib.call("svgp_sprites_posterior_rows", C.byref(cfg), Kb.data_ptr(), kbb.data_ptr(), mt.data_ptr(), X.data_ptr(),
                      eps.data_ptr(), p_m.data_ptr(), p_v.data_ptr(), z.data_ptr(), work.data_ptr(), stream)

        def new():
            _, Kb, kbb = eng.kernel_matrices(aux)
            entry(Kb, kbb, torch.cuda.current_stream(dev).cuda_stream)
            return p_m, p_v, z

        ref, got = old(), new()                                # warm-up of both paths at this shape; and the same numbers
        torch.cuda.synchronize()
        err = {k: float((g - r).abs().max() / r.abs().max()) for k, r, g in zip(("p_m", "p_v", "z"), ref, got)}
        inside = float(((ref[1] > CLIP[0]) & (ref[1] < CLIP[1])).double().mean())
        t_old, t_new, t_km = [], [], []
        for _ in range(args.reps):                             # alternating, as two versions are compared in one call
            t_old.append(timed(old)); t_new.append(timed(new)); t_km.append(timed(lambda: eng.kernel_matrices(aux)))
        _, Kb, kbb = eng.kernel_matrices(aux)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        s = torch.cuda.current_stream(dev)
        for e0, e1 in ev:
            e0.record(s); entry(Kb, kbb, s.cuda_stream); e1.record(s)
        torch.cuda.synchronize()
        t_dev = [e0.elapsed_time(e1) * 1e-3 for e0, e1 in ev]
        med = lambda v: float(np.median(v))
        flops, x_bytes = 2.0 * b * m * m * L, 8.0 * L * m * m
        row = dict(m=m, L=L, rows=b, reps=args.reps, rel_diff=err, p_v_inside_clip=inside,
                   existing_path_s=med(t_old), existing_path_min_s=float(np.min(t_old)),
                   new_path_s=med(t_new), new_path_min_s=float(np.min(t_new)),
                   kernel_matrices_s=med(t_km), entry_device_s=med(t_dev), entry_device_min_s=float(np.min(t_dev)),
                   entry_tflops=flops / med(t_dev) / 1e12, entry_x_gbytes_per_s=x_bytes / med(t_dev) / 1e9,
                   product_bytes_removed=8.0 * L * b * m, workspace_bytes=8.0 * n_work, route=A.route(dict(m=m, L=L), rows=b))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del eng, svgp, X, Si
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return rows


if __name__ == "__main__":
    main()
