"""The stream routing of the sparse-GP block of a step that the host enqueues stage by stage (SpritesStepEngine.phases,
MnistStepEngine.sharded_stages): gp_block_route plans it as data, run_gp_route walks the plan.  No torch, no library at import:
tests/test_sprites_route_cpu.py pins the routes and drives the executor with recording stand-ins.  (The MNIST step's own launch
plan is the library's, csrc/step_plan.hpp.)

A route is a tuple of steps:
  ("launch", entry, lane, part)   entry point of the library on lane "main" / "side0" / "side1"; part: a name of _lib.FWD_PART /
                                  BWD_PART for the two *_channels_part entries, else None
  ("fork", lane)                  the lane waits for main            ("join", lane)   main waits for the lane
  ("chain", lane, other)          the lane waits for the other side lane
  ("exchange", k)                 the caller's exchange point: "statA" / "statB" (all-reduces), 1..4 (ShardedExchange.point)
  ("networks",)                   the caller's decoder forward + reverse, between the row stage and the reverse statistics
  ("pack_window",)                ShardedExchange.pack_window
"""
import functools

from ._lib import BWD_PART, FWD_PART, SvgpError, call

SHARD_NEEDS = "channel_shard needs m > 64, L divisible by the number of ranks and the Hensman branch"
# entries whose argument list has no state pointer in front of the stream
_NO_STATE = {"svgp_gp_stats_fwd", "svgp_gp_titsias_stats", "svgp_gp_factor_fwd", "svgp_gp_factor_fwd_defer_aji",
             "svgp_gp_factor_fwd_aji_tail", "svgp_gp_factor_fwd_channels_part"}


def _launch(stage, lane="main", part=None):
    return ("launch", "svgp_gp_" + stage, lane, part)


@functools.lru_cache(maxsize=None)
def gp_block_route(m, titsias, sharded, n_side, kbar_branch):
    """The ordered route of the GP block: forward statistics ... reverse row stage.  n_side: side streams at hand (0, 1, 2).

    The side work of the forward factor stage -- its tail ((A_hat + jI)^-1, log det, KL_l: a whole batched inverse that only the
    reverse factor stage and the final scalars need; include/svgpvae_hip.h: svgp_gp_factor_fwd_aji_tail) and the early half of the
    reverse factor stage (no reverse statistic needed) -- runs beside the row stage, the decoder and the reverse statistics.  It is
    FORKED right behind the head of the stage (sharded: in front of exchange point 2) but ISSUED behind the row stage
    (svgp_gp_posterior_fwd): its launches (two blocked factorisations) take the host ~0.5 ms to enqueue, and the caller's stream
    must not run dry meanwhile; enqueued in front of the collective, the branch's GEMMs fill the chip and the collective's kernel
    waits for a slot.  The branch has the slack."""
    if sharded and (m <= 64 or titsias):
        raise SvgpError(SHARD_NEEDS)
    fork = ("fork", "side0")
    join = ("join", "side0")
    r = [_launch("stats_fwd")] + [_launch("titsias_stats")] * bool(titsias)
    if sharded:
        side = "side0" if n_side else "main"
        r += [("exchange", 1), _launch("factor_fwd_channels_part", part="HEAD"), ("pack_window",)] + [fork] * bool(n_side)
        r += [("exchange", 2), _launch("posterior_fwd"), _launch("factor_fwd_channels_part", side, "TAIL")]
        r += [_launch("factor_bwd_channels_part", side, "EARLY")] * bool(n_side)
        late = [("exchange", 3)] + [join] * bool(n_side)
        late += [_launch("factor_bwd_channels_part", part="LATE" if n_side else "ALL"), ("exchange", 4)]
    elif m > 64 and n_side and not titsias:
        # (not with titsias: svgp_gp_titsias_fwd inverts through the same scratch, ws.scr_inv, on the main stream)
        r += [("exchange", "statA"), _launch("factor_fwd_defer_aji"), fork] + [("fork", "side1")] * (n_side > 1)
        r += [_launch("posterior_fwd"), _launch("factor_fwd_aji_tail", "side0")]
        if n_side > 1:      # the first part of the early reverse half beside the tail (it does not need the tail's inverse)
            r += [_launch("factor_bwd_early_a", "side1"), ("chain", "side0", "side1"), _launch("factor_bwd_early_b", "side0")]
        else:
            r += [_launch("factor_bwd_early", "side0")]
        # late_a: the part of the late half that reads nothing the side branch writes -- the vector chain and, with all rows local, X
        # and the two full products Si X, (Si X) Si: 2.3 ms at m = 800 -- BEFORE the join: the caller's stream used to wait 0.8 ms
        # there for the second inverse + early half with that work ready.  Then (as csrc/api.hip does for the MNIST step) the
        # single-matrix chain of the gradient of Ki on the branch that has just been joined, beside the channel block
        late = [("exchange", "statB"), _launch("factor_bwd_late_a"), join]
        if kbar_branch:
            late += [fork, _launch("factor_bwd_late_b_kbar", "side0"), _launch("factor_bwd_late_b_channels"), join,
                     _launch("factor_bwd_late_b_final")]
        else:
            late += [_launch("factor_bwd_late_b")]
    else:
        r += [("exchange", "statA"), _launch("factor_fwd"), _launch("posterior_fwd")]
        late = [("exchange", "statB"), _launch("factor_bwd")]
    r += [_launch("titsias_fwd")] * bool(titsias) + [("networks",), _launch("stats_bwd")] + late
    return tuple(r + [_launch("posterior_bwd")] + [_launch("titsias_bwd")] * bool(titsias))


def run_gp_route(route, lanes, cp, ws, st, *, eps=None, window=None, networks, pack_window=None, call=call):
    """Walks `route`: a generator that yields k at ("exchange", k) -- the caller runs that point and resumes.
    lanes: lane -> torch stream; cp, ws, st: the MnistCfg reference and the workspace / state pointers; eps: the noise of the
    row stage or None; window() -> (l0, nl), the rank's channels, asked for at a *_channels_part entry; networks, pack_window:
    called at their markers."""
    main = lanes["main"]
    for kind, *a in route:
        if kind == "launch":
            entry, lane, part = a
            args = [cp]
            if part is not None:
                args += [*window(), (FWD_PART if "_fwd_" in entry else BWD_PART)[part]]
            if entry == "svgp_gp_posterior_fwd":
                args.append(eps)
            args.append(ws)
            if entry not in _NO_STATE:
                args.append(st)
            call(entry, *args, lanes[lane].cuda_stream)
        elif kind == "fork":
            lanes[a[0]].wait_stream(main)
        elif kind == "join":
            main.wait_stream(lanes[a[0]])
        elif kind == "chain":
            lanes[a[0]].wait_stream(lanes[a[1]])
        elif kind == "exchange":
            yield a[0]
        elif kind == "networks":
            networks()
        else:
            pack_window()
