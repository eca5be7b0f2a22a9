"""Information-only timing of the exact per-video GP baselines against the sparse SVGP-VAE as the videos get longer: the
moving-ball step at the reference's 35 videos, 32x32 frames, MLP 500, float64, for tmax in 64, 128, 256, 512, 1024.

  exact   PearceLongStepEngine (pearce_long.hip) per --elbo VAE | GPVAE_Pearce --GP_joint | NP --GP_joint at every tmax
  lds     PearceStepEngine (k_pearce_fwd / k_pearce_bwd) at tmax = 64 only, the last size it takes
  sparse  the engine ball.sparse_engine_class picks (BallStepEngine up to m = 64, BallLargeStepEngine above), SVGPVAE_Hensman, at
          every tmax twice: with the old m = 15 and with --m inducing points -- by default one per model length scale,
          m = ceil(tmax / 2) capped at 2048 (`--m N`: N at every tmax), so that the sparse model can represent a length-scale-2
          path as the exact one does

Every configuration runs in a child process of its own under a time limit; the first child that fails ends the run (nothing
more is started on the device after a fault).  A child warms up, then times `--blocks` blocks of `--steps` steps with device
events on the engine's stream (one fixed device-synthesised batch, so the window holds the step alone) and reports the median,
minimum and maximum block.  `--stages TMAX` adds, for the exact engines at that tmax, the time between events placed around the
GP-regression calls of one step (forward / reverse, full set / context set); the rest of the step is MLP, reconstruction term,
Adam.  There is no pass / fail number.

    python tools/ball_long_bench.py [--tmax 64 128 256 512 1024] [--m auto] [--kinds exact lds sparse] [--stages 256] \
        > profiles/ball_long.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXACT = {"VAE": [], "GPVAE_Pearce": ["--GP_joint"], "NP": ["--GP_joint"]}


def sparse_m(rule, tmax):
    """--m: `auto` = one inducing point per model length scale (2 frames), at most 2048; or a number."""
    return min(-(-tmax // 2), 2048) if rule == "auto" else int(rule)


def _engine(kind, elbo, tmax, m=15):
    from svgp_vae_amd import BALL_experiment as BE, ball
    if kind == "sparse":
        flags = ["--elbo", "SVGPVAE_Hensman", "--m", str(m), "--tmax", str(tmax), "--ip_max", str(tmax), "--clip_qs", "--jitter",
                 "1e-6", "--GP_joint", "--ip_joint"]
        return BE.build_engine(BE.build_parser().parse_args(flags))
    args = BE.build_parser().parse_args(["--elbo", elbo, "--tmax", str(tmax)] + EXACT[elbo])
    cls = ball.PearceStepEngine if kind == "lds" else ball.PearceLongStepEngine
    return cls(elbo, 0.001 if elbo == "VAE" else args.modellt, 0.5, args.GP_joint, args.GP_init, batch=35, tmax=tmax, px=32,
               py=32, hidden=500)


def worker(a):
    import torch
    from svgp_vae_amd import ball
    eng = _engine(a.kind, a.elbo, a.tmax, int(a.m))
    vid = ball.VideoBatchSource(tmax=a.tmax, px=32, py=32, lt=2, batch=35, seed=1, r=3)()
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        eng.step(vid, None, adam=True)
    eng.stream.synchronize()
    ms = []
    for _ in range(a.blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(eng.stream)
        for _ in range(a.steps):
            eng.step(vid, None, adam=True)
        e1.record(eng.stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / a.steps)
    res = dict(kind=a.kind, elbo=a.elbo, tmax=a.tmax, m=int(a.m) if a.kind == "sparse" else None, engine=type(eng).__name__,
               ms_per_step_median=statistics.median(ms), ms_per_step_min=min(ms),
               ms_per_step_max=max(ms), blocks=a.blocks, steps_per_block=a.steps, elbo_after=eng.scalars()["elbo"])
    if a.stages and a.kind != "sparse":
        marks = []

        def wrap(name, fn):
            def run(q, *rest):
                tag = f"{name}_{'full' if q.idx is None else 'context'}"
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record(eng.stream); fn(q, *rest); ev[1].record(eng.stream)
                marks.append((tag, ev))
            return run
        eng._gp_fwd, eng._gp_bwd = wrap("gp_fwd", eng._gp_fwd), wrap("gp_bwd", eng._gp_bwd)
        acc, total = {}, []
        for _ in range(a.steps):
            marks.clear()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(eng.stream); eng.step(vid, None, adam=True); e1.record(eng.stream)
            e1.synchronize()
            total.append(e0.elapsed_time(e1))
            for tag, ev in marks:
                acc.setdefault(tag, []).append(ev[0].elapsed_time(ev[1]))
        st = {k: statistics.median(v) for k, v in acc.items()}
        st["step"] = statistics.median(total)
        st["rest"] = st["step"] - sum(v for k, v in st.items() if k != "step")
        res["stages_ms_median_single_steps"] = st
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tmax", type=int, nargs="+", default=[64, 128, 256, 512, 1024])
    ap.add_argument("--elbo", nargs="+", default=list(EXACT))
    ap.add_argument("--m", default="auto", help="inducing points of the second sparse column: auto = ceil(tmax / 2) <= 2048, or a number")
    ap.add_argument("--kinds", nargs="+", default=["exact", "lds", "sparse"], choices=["exact", "lds", "sparse"])
    ap.add_argument("--stages", type=int, default=0, help="tmax at which the per-stage event times are taken too (0: none)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="time limit of one configuration, seconds")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--kind", default="exact")
    a = ap.parse_args()
    if a.worker:
        a.elbo, a.tmax = a.elbo[0], a.tmax[0]
        return worker(a)
    jobs = []
    for T in a.tmax:
        if "exact" in a.kinds:
            jobs += [("exact", e, T, 0) for e in a.elbo]
        if T == 64 and "lds" in a.kinds:
            jobs += [("lds", e, T, 0) for e in a.elbo]
        if "sparse" in a.kinds:
            jobs += [("sparse", "SVGPVAE_Hensman", T, m) for m in dict.fromkeys((15, sparse_m(a.m, T)))]
    rows = []
    for kind, elbo, T, m in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--kind", kind, "--elbo", elbo, "--tmax", str(T), "--m", str(m), "--steps",
               str(a.steps), "--blocks", str(a.blocks), "--warmup", str(a.warmup), "--stages", str(int(a.stages == T))]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"{kind} {elbo} tmax {T}: no answer within {a.limit} s; stopping", file=sys.stderr)
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{kind} {elbo} tmax {T}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            break
        rows.append(json.loads(line[0][7:]))
        print(f"{kind:6s} {elbo:16s} tmax {T:5d} m {m:4d}: {rows[-1]['ms_per_step_median']:9.3f} ms/step "
              f"[{rows[-1]['ms_per_step_min']:.3f}, {rows[-1]['ms_per_step_max']:.3f}]", file=sys.stderr, flush=True)
    print(json.dumps(dict(workload="moving ball, batch 35, 32x32, MLP 500, float64; device-event time of the step alone, median "
                                   "[min, max] over blocks", rows=rows)))
    return 0 if len(rows) == len(jobs) else 1


if __name__ == "__main__":
    sys.exit(main())
