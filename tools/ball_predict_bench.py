"""Moving-ball predictor: the GP launch alone and the whole `BallPredictor.predict`, per batch.

Shapes (B videos, T frames, m inducing points, Q query times): the reference batch at its own frame rate (35, 30, 15, 30) and at
eight times that rate (35, 30, 15, 240), the largest fused shape (256, 64, 64, 512), and one shape of the large route
(35, 64, 256, 128).  Beside each, the exact-GP predictor (PearcePredictor) at the same (B, T, Q): svgp_pearce_predict for these
T <= 64, and svgp_pearce_predict_long forced onto the same shape; plus one shape only the long entry takes, (35, 256, -, 512).
Frames 32 x 32, hidden 500, 40 % of the frames dropped.  The GP stage is timed between device events (its own
launches only, inputs resident), `predict` by the wall clock around a call that ends in a device synchronise; medians and minima
over --reps calls after a warm-up of each.  Information only, no threshold; needs a GPU and fails without one.

--joint: instead, the GP stage of the marginal entries (p_m, p_v, an independent draw) against that of the joint entries (p_m, the
full covariance, its Cholesky factor's path) at (35, 30, 15, 60) through the one-launch and through the
workspace entries, and at (35, 30, 15, 1024) through the workspace entries, which alone take that Q.

--state: instead, the streamed posterior state against the one-shot entry, GP stage only, at (35, 30, 15, 30),
(2, 2048, 64, 4096) and (2, 2048, 256, 4096): (a) svgp_ball_predict / svgp_ball_predict_large, (b) svgp_ball_state_update + finalize +
query from an empty state, (c) svgp_ball_state_query alone on the finished state.

    python tools/ball_predict_bench.py [--joint | --state] [--reps 30] [--out profiles/ball_predict_bench.json]
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
PEARCE_LONG_ONLY = [(35, 256, 512)]
JOINT_SHAPES = [((35, 30, 15, 60), False), ((35, 30, 15, 60), True), ((35, 30, 15, 1024), True)]      # (shape, workspace entries)
STATE_SHAPES = [(35, 30, 15, 30), (2, 2048, 64, 4096), (2, 2048, 256, 4096)]
PX, HIDDEN = 32, 500


def _device_times(stream, fn, reps):
    """Seconds between device events around `fn`, per call, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record(stream); fn(); e1.record(stream)
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) * 1e-3 for e0, e1 in ev]


def pearce_rows(B, T, Q, reps, vid=None, observed=None):
    """The exact-GP predictor at (B, T, Q): the GP stage of each entry that takes T, and the whole predict."""
    import ctypes as C

    from svgp_vae_amd import _lib, ball
    from svgp_vae_amd.ball_predict import PEARCE_FUSED_T_MAX, PearcePredictor
    rs = np.random.RandomState(0)
    params = dict(ball.truncated_normal_mlp_params(PX, PX, HIDDEN, 0))
    params.update(l_x=[2.0], l_y=[2.0 / 1.1])
    pred = PearcePredictor(params, tmax=T, hidden=HIDDEN, px=PX, py=PX)
    f64 = dict(dtype=torch.float64, device=pred.dev)
    if observed is None:
        observed = rs.rand(B, T) >= 0.4
        observed[:, 0] = True
    tq = np.linspace(1.0, float(T), Q)
    mu = [torch.randn(T, B, **f64) for _ in range(2)]
    var = [torch.rand(T, B, **f64) * 0.5 + 1e-3 for _ in range(2)]
    times, tqd = torch.arange(1, T + 1, **f64), torch.as_tensor(tq, **f64)
    mask = torch.as_tensor(observed, **f64).t().contiguous()
    out = [torch.empty(Q, B, **f64) for _ in range(6)]
    lh = torch.empty(2, B, **f64)
    cfg = _lib.PearcePredictCfg(B=B, T=T, Q=Q, q_slices=0)
    q = _lib.PearcePredictBufs()
    q.times, q.tq, q.mask, q.lh = times.data_ptr(), tqd.data_ptr(), mask.data_ptr(), lh.data_ptr()
    for c, cn in enumerate("xy"):
        setattr(q, f"ls_{cn}", pred.params[f"l_{cn}"].data_ptr())
        setattr(q, f"mu_{cn}", mu[c].data_ptr()); setattr(q, f"var_{cn}", var[c].data_ptr())
        setattr(q, f"p_m_{cn}", out[c].data_ptr()); setattr(q, f"p_v_{cn}", out[2 + c].data_ptr()); setattr(q, f"z_{cn}", out[4 + c].data_ptr())
    work = torch.empty(int(pred.lib.svgp_pearce_predict_long_workspace_elems(C.byref(cfg))), **f64)
    s = pred.stream.cuda_stream
    row = dict(model="exact-GP", B=B, T=T, Q=Q, reps=reps)
    if T <= PEARCE_FUSED_T_MAX:
        t = _device_times(pred.stream, lambda: _lib.call("svgp_pearce_predict", C.byref(cfg), C.byref(q), s), reps)
        row.update(gp_lds_device_s=float(np.median(t)), gp_lds_device_min_s=float(np.min(t)))
    t = _device_times(pred.stream, lambda: _lib.call("svgp_pearce_predict_long", C.byref(cfg), C.byref(q), work.data_ptr(), s), reps)
    buf = C.create_string_buffer(1 << 16)
    _lib.call("svgp_pearce_predict_route", C.byref(cfg), 1, buf, len(buf))
    names = buf.value.decode().split()
    row.update(gp_long_device_s=float(np.median(t)), gp_long_device_min_s=float(np.min(t)), gp_long_launches=len(names))
    if vid is None:
        _, vid = ball.Make_Video_batch(tmax=T, px=PX, py=PX, lt=2, batch=B, seed=0)
        vid = torch.as_tensor(vid, dtype=torch.float64, device=pred.dev)
    pred.predict(vid, tq, observed=observed)
    t_all = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pred.predict(vid, tq, observed=observed)
        t_all.append(time.perf_counter() - t0)
    row.update(predict_s=float(np.median(t_all)), predict_min_s=float(np.min(t_all)), route=pred.route(B, T, Q)[:3])
    return row


def joint_rows(reps):
    """Marginal against joint GP stage, device time between events, inputs resident."""
    from svgp_vae_amd import ball
    from svgp_vae_amd.ball_predict import BallPredictor
    rows = []
    for (B, T, m, Q), large in JOINT_SHAPES:
        rs = np.random.RandomState(0)
        ls = min(2.0, 0.75 * (T - 1) / (m - 1))
        params = dict(ball.truncated_normal_mlp_params(PX, PX, HIDDEN, 0))
        params.update(ip_x=np.linspace(1, T, m), ip_y=np.linspace(1, T, m), l_x=[ls], l_y=[ls / 1.1])
        pred = BallPredictor(params, tmax=T, m=m, hidden=HIDDEN, px=PX, py=PX, jitter=1e-9, clip_qs=True)
        f64 = dict(dtype=torch.float64, device=pred.dev)
        observed = rs.rand(B, T) >= 0.4
        observed[:, 0] = True
        mu = [torch.randn(T, B, **f64) for _ in range(2)]
        var = [torch.rand(T, B, **f64) * 0.5 + 1e-3 for _ in range(2)]
        eps = [torch.randn(Q, B, **f64) for _ in range(2)]
        times, tqd = torch.arange(1, T + 1, **f64), torch.as_tensor(np.linspace(1.0, float(T), Q), **f64)
        mask = torch.as_tensor(observed, **f64).t().contiguous()

        def marginal():
            with torch.cuda.stream(pred.stream):
                pred._gp(mu, var, times, tqd, mask, eps, force_large=large)

        def joint():
            with torch.cuda.stream(pred.stream):
                pred._gp_joint(mu, var, times, tqd, mask, eps, 1e-6, force_large=large)

        t_m, t_j = _device_times(pred.stream, marginal, reps), _device_times(pred.stream, joint, reps)
        row = dict(B=B, T=T, m=m, Q=Q, reps=reps, entries="workspace" if large else "one-launch",
                   marginal_device_s=float(np.median(t_m)), marginal_device_min_s=float(np.min(t_m)),
                   joint_device_s=float(np.median(t_j)), joint_device_min_s=float(np.min(t_j)),
                   joint_launches=len(pred.route(B, T, Q, joint=True)) if not large else None)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pred
        torch.cuda.empty_cache()
    return rows


def state_rows(reps):
    """One-shot entry against update + finalize + query and against the query alone, device time between events, inputs resident."""
    from svgp_vae_amd import ball
    from svgp_vae_amd.ball_predict import BallPredictor
    rows = []
    for B, T, m, Q in STATE_SHAPES:
        rs = np.random.RandomState(0)
        ls = min(2.0, 0.75 * (T - 1) / (m - 1))
        params = dict(ball.truncated_normal_mlp_params(PX, PX, HIDDEN, 0))
        params.update(ip_x=np.linspace(1, T, m), ip_y=np.linspace(1, T, m), l_x=[ls], l_y=[ls / 1.1])
        pred = BallPredictor(params, tmax=T, m=m, hidden=HIDDEN, px=PX, py=PX, jitter=1e-9, clip_qs=True)
        f64 = dict(dtype=torch.float64, device=pred.dev)
        observed = rs.rand(B, T) >= 0.4
        observed[:, 0] = True
        mu = [torch.randn(T, B, **f64) for _ in range(2)]
        var = [torch.rand(T, B, **f64) * 0.5 + 1e-3 for _ in range(2)]
        times, tqd = torch.arange(1, T + 1, **f64), torch.as_tensor(np.linspace(1.0, float(T), Q), **f64)
        mask = torch.as_tensor(observed, **f64).t().contiguous()
        state = pred.state(B)

        def one_shot():
            with torch.cuda.stream(pred.stream):
                pred._gp(mu, var, times, tqd, mask, None)

        def streamed():
            with torch.cuda.stream(pred.stream):
                state.stats.zero_()
                state._update(mu, var, times, mask)
                state._finalize()
                state._query(tqd, None)

        def query_only():
            with torch.cuda.stream(pred.stream):
                state._query(tqd, None)

        t_a, t_b = _device_times(pred.stream, one_shot, reps), _device_times(pred.stream, streamed, reps)
        t_c = _device_times(pred.stream, query_only, reps)
        med = lambda t: float(np.median(t))
        row = dict(B=B, T=T, m=m, Q=Q, reps=reps, one_shot_device_s=med(t_a), one_shot_device_min_s=float(np.min(t_a)),
                   update_finalize_query_device_s=med(t_b), update_finalize_query_device_min_s=float(np.min(t_b)),
                   query_device_s=med(t_c), query_device_min_s=float(np.min(t_c)),
                   launches={op: len(state.route(op, T=T, Q=Q)) for op in ("update", "finalize", "query")})
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pred, state
        torch.cuda.empty_cache()
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--joint", action="store_true", help="time the marginal against the joint GP stage instead")
    ap.add_argument("--state", action="store_true", help="time the streamed posterior state against the one-shot entry instead")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("the timings need a GPU")
    if args.joint or args.state:
        rows = joint_rows(args.reps) if args.joint else state_rows(args.reps)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(rows, f, indent=1)
        return rows
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
        rows.append(pearce_rows(B, T, Q, args.reps, vid=vid, observed=observed))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    for B, T, Q in PEARCE_LONG_ONLY:
        rows.append(pearce_rows(B, T, Q, args.reps))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return rows


if __name__ == "__main__":
    main()
