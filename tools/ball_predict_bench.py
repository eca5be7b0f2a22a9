"""Moving-ball predictor: the GP launch alone and the whole `BallPredictor.predict`, per batch.

Shapes (B videos, T frames, m inducing points, Q query times): the reference batch at its own frame rate (35, 30, 15, 30) and at
eight times that rate (35, 30, 15, 240), the largest fused shape (256, 64, 64, 512), and one shape of the large route
(35, 64, 256, 128).  Frames 32 x 32, hidden 500, 40 % of the frames dropped.  The GP stage is timed between device events (its own
launches only, inputs resident), `predict` by the wall clock around a call that ends in a device synchronise; medians and minima
over --reps calls after a warm-up of each.  Information only, no threshold; needs a GPU and fails without one.

    python tools/ball_predict_bench.py [--reps 30] [--out profiles/ball_predict_bench.json]
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

SHAPES = [(35, 30, 15, 30), (35, 30, 15, 240), (256, 64, 64, 512), (35, 64, 256, 128)]
PX, HIDDEN = 32, 500


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("the timings need a GPU")
    from svgp_vae_amd import ball
    from svgp_vae_amd.ball_predict import BallPredictor
    rows = []
    for B, T, m, Q in SHAPES:
        rs = np.random.RandomState(0)
        ls = min(2.0, 0.75 * (T - 1) / (m - 1))
        params = dict(ball.truncated_normal_mlp_params(PX, PX, HIDDEN, 0))
        params.update(ip_x=np.linspace(1, T, m), ip_y=np.linspace(1, T, m), l_x=[ls], l_y=[ls / 1.1])
        pred = BallPredictor(params, tmax=T, m=m, hidden=HIDDEN, px=PX, py=PX, jitter=1e-9, clip_qs=True)
        _, vid = ball.Make_Video_batch(tmax=T, px=PX, py=PX, lt=2, batch=B, seed=0)
        vid = torch.as_tensor(vid, dtype=torch.float64, device=pred.dev)
        observed = rs.rand(B, T) >= 0.4
        observed[:, 0] = True
        tq = np.linspace(1.0, float(T), Q)
        f64 = dict(dtype=torch.float64, device=pred.dev)
        mu = [torch.randn(T, B, **f64) for _ in range(2)]
        var = [torch.rand(T, B, **f64) * 0.5 + 1e-3 for _ in range(2)]
        times, tqd = torch.arange(1, T + 1, **f64), torch.as_tensor(tq, **f64)
        mask = torch.as_tensor(observed, **f64).t().contiguous()

        def gp():
            with torch.cuda.stream(pred.stream):
                pred._gp(mu, var, times, tqd, mask, None)

        def whole():
            pred.predict(vid, tq, observed=observed)

        gp(); whole()                                          # warm-up: workspaces grow once, code objects load
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for e0, e1 in ev:
            e0.record(pred.stream); gp(); e1.record(pred.stream)
        torch.cuda.synchronize()
        t_gp = [e0.elapsed_time(e1) * 1e-3 for e0, e1 in ev]
        t_all = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            whole()
            t_all.append(time.perf_counter() - t0)
        route = pred.route(B, T, Q)
        row = dict(B=B, T=T, m=m, Q=Q, reps=args.reps, gp_device_s=float(np.median(t_gp)), gp_device_min_s=float(np.min(t_gp)),
                   predict_s=float(np.median(t_all)), predict_min_s=float(np.min(t_all)), gp_launches=len(route),
                   route=route if len(route) <= 4 else route[:3] + ["..."])
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pred
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return rows


if __name__ == "__main__":
    main()
