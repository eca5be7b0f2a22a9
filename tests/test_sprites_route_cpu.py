"""The stream routing of the sparse-GP block as the host enqueues it (svgp_vae_amd.gp_route: SpritesStepEngine.phases and
MnistStepEngine.sharded_stages), pinned without a GPU and without the library: which stage entry runs on which lane, where the side
lanes are forked, chained and joined, where the exchange points, the networks and the window packing go.

The expected routes were read by hand from SpritesStepEngine._phases_body and MnistStepEngine.sharded_stages as they stood before
the planner existed; they are not output of the planner.  Notation of tests/test_step_route_cpu.py: one word per entry (ABBR),
`s0:` / `s1:` put a launch on side lane 0 / 1, `fork0` / `join0`, `x:ARG` appends the part; here also `chain01` (side0 waits for
side1), `X:statA` / `X1` (exchange points), `NETS` (decoder forward + reverse) and `pack_window`."""
import itertools

import pytest

import svgp_vae_amd
from svgp_vae_amd.gp_route import gp_block_route, run_gp_route

ABBR = {
    "stats": "svgp_gp_stats_fwd", "tstats": "svgp_gp_titsias_stats", "fwd": "svgp_gp_factor_fwd", "bwd": "svgp_gp_factor_bwd",
    "defer": "svgp_gp_factor_fwd_defer_aji", "tail": "svgp_gp_factor_fwd_aji_tail", "bigf": "svgp_gp_factor_fwd_channels_part",
    "bigb": "svgp_gp_factor_bwd_channels_part", "post": "svgp_gp_posterior_fwd", "tfwd": "svgp_gp_titsias_fwd",
    "stats_bwd": "svgp_gp_stats_bwd", "early": "svgp_gp_factor_bwd_early", "early_a": "svgp_gp_factor_bwd_early_a",
    "early_b": "svgp_gp_factor_bwd_early_b", "late_a": "svgp_gp_factor_bwd_late_a", "late_b": "svgp_gp_factor_bwd_late_b",
    "kbar": "svgp_gp_factor_bwd_late_b_kbar", "channels": "svgp_gp_factor_bwd_late_b_channels",
    "final": "svgp_gp_factor_bwd_late_b_final", "post_bwd": "svgp_gp_posterior_bwd", "tbwd": "svgp_gp_titsias_bwd",
}


def expand(route):
    steps = []
    for tok in route.split():
        lane = "main"
        if tok[:3] in ("s0:", "s1:"):
            lane, tok = "side" + tok[1], tok[3:]
        if tok in ("fork0", "fork1", "join0"):
            steps.append((tok[:4], "side" + tok[4]))
        elif tok == "chain01":
            steps.append(("chain", "side0", "side1"))
        elif tok == "NETS":
            steps.append(("networks",))
        elif tok == "pack_window":
            steps.append(("pack_window",))
        elif tok[0] == "X":
            steps.append(("exchange", tok[2:] if tok[1] == ":" else int(tok[1:])))
        else:
            head, *part = tok.split(":")
            steps.append(("launch", ABBR[head], lane, part[0] if part else None))
    return tuple(steps)


PLAIN = "stats X:statA fwd post NETS stats_bwd X:statB bwd post_bwd"
PLAIN_TIT = "stats tstats X:statA fwd post tfwd NETS stats_bwd X:statB bwd post_bwd tbwd"
LATE, LATE_INLINE = "late_a join0 fork0 s0:kbar channels join0 final post_bwd", "late_a join0 late_b post_bwd"
LARGE2 = "stats X:statA defer fork0 fork1 post s0:tail s1:early_a chain01 s0:early_b NETS stats_bwd X:statB "
LARGE1 = "stats X:statA defer fork0 post s0:tail s0:early NETS stats_bwd X:statB "
SHARDED = "stats X1 bigf:HEAD pack_window fork0 X2 post s0:bigf:TAIL s0:bigb:EARLY NETS stats_bwd X3 join0 bigb:LATE X4 post_bwd"
SHARDED_INLINE = "stats X1 bigf:HEAD pack_window X2 post bigf:TAIL NETS stats_bwd X3 bigb:ALL X4 post_bwd"

# (expected, m, titsias, sharded, n_side, kbar_branch)
CASES = [(PLAIN, m, False, False, n, k) for m in (8, 64) for n in (0, 1, 2) for k in (True, False)] + \
        [(PLAIN, m, False, False, 0, k) for m in (65, 800) for k in (True, False)] + \
        [(PLAIN_TIT, m, True, False, n, k) for m in (8, 64, 65, 800) for n in (0, 1, 2) for k in (True, False)] + \
        [(LARGE2 + LATE, m, False, False, 2, True) for m in (65, 800)] + \
        [(LARGE2 + LATE_INLINE, m, False, False, 2, False) for m in (65, 800)] + \
        [(LARGE1 + LATE, m, False, False, 1, True) for m in (65, 800)] + \
        [(LARGE1 + LATE_INLINE, m, False, False, 1, False) for m in (65, 800)] + \
        [(SHARDED, m, False, True, n, k) for m in (65, 800) for n in (1, 2) for k in (True, False)] + \
        [(SHARDED_INLINE, m, False, True, 0, k) for m in (65, 800) for k in (True, False)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "m{} titsias={} sharded={} n_side={} kbar={}".format(*c[1:]))
def test_every_class_takes_its_route(case):
    assert gp_block_route(*case[1:]) == expand(case[0])


def test_every_argument_combination_is_covered_or_refused():
    covered = {c[1:] for c in CASES}
    for args in itertools.product((64, 65), (False, True), (False, True), (0, 1, 2), (False, True)):
        m, titsias, sharded = args[:3]
        if sharded and (m <= 64 or titsias):
            with pytest.raises(svgp_vae_amd.SvgpError, match="channel_shard needs m > 64, L divisible by the number of ranks and "
                                                              "the Hensman branch"):
                gp_block_route(*args)
        else:
            assert args in covered
    used = {s[1] for c in CASES for s in expand(c[0]) if s[0] == "launch"}
    assert used == set(ABBR.values())


def test_route_changes_at_m_64_only_where_the_table_says():
    for titsias, n_side, kbar in itertools.product((False, True), (0, 1, 2), (False, True)):
        lo, hi = gp_block_route(64, titsias, False, n_side, kbar), gp_block_route(65, titsias, False, n_side, kbar)
        assert (lo != hi) == (not titsias and n_side > 0)
        assert lo == expand(PLAIN_TIT if titsias else PLAIN)


def test_titsias_never_yields_a_side_launch():
    for m, n_side, kbar in itertools.product((8, 64, 65, 800), (0, 1, 2), (False, True)):
        route = gp_block_route(m, True, False, n_side, kbar)
        assert all(s[0] in ("launch", "exchange", "networks") and (s[0] != "launch" or s[2] == "main") for s in route)


# ---- the executor, with recording stand-ins -------------------------------------------------------------------------------------
class _Stream:
    """Stands in for a torch stream: logs who waits for whom."""

    def __init__(self, lane, log):
        self.cuda_stream, self.log = lane, log

    def wait_stream(self, other):
        self.log.append(("wait", self.cuda_stream, other.cuda_stream))


def _execute(route, window=(3, 2)):
    """What run_gp_route does with `route`, spelled as route steps again: a launch from the entry and the stream handle the fake
    `call` saw (the part read back from its position in the argument list), fork / join / chain from the logged waits."""
    from svgp_vae_amd._lib import BWD_PART, FWD_PART
    log = []
    lanes = {lane: _Stream(lane, log) for lane in ("main", "side0", "side1")}

    def call(entry, *args):
        part = None
        if entry.endswith("_channels_part"):
            assert args[1:3] == window
            part = {v: k for k, v in (FWD_PART if "_fwd_" in entry else BWD_PART).items()}[args[3]]
        want = ("cp",) + (window + (args[3],) if part else ()) + (("eps",) if entry == "svgp_gp_posterior_fwd" else ()) + ("ws",)
        assert args[:-1] in (want, want + ("st",)), (entry, args)        # (which entries take the state: the library's header)
        log.append(("launch", entry, args[-1], part))

    for k in run_gp_route(route, lanes, "cp", "ws", "st", eps="eps", window=lambda: window, call=call,
                          networks=lambda: log.append(("networks",)), pack_window=lambda: log.append(("pack_window",))):
        log.append(("exchange", k))
    out = []
    for step in log:
        if step[0] == "wait":
            _, waiter, other = step
            step = ("fork", waiter) if other == "main" else ("join", other) if waiter == "main" else ("chain", waiter, other)
        out.append(step)
    return tuple(out)


@pytest.mark.parametrize("route", [LARGE2 + LATE, SHARDED, SHARDED_INLINE, LARGE1 + LATE_INLINE, PLAIN_TIT],
                         ids=["two side streams, kbar on", "sharded", "sharded in line", "one side stream, kbar off", "titsias"])
def test_executor_issues_the_route_in_order(route):
    """Every launch on its lane's stream, every wait between the launches where the route has it: the side work is forked behind
    the head of the forward factor stage and issued behind svgp_gp_posterior_fwd."""
    assert _execute(expand(route)) == expand(route)


def test_state_pointer_follows_the_header():
    """The entries run_gp_route calls without the state pointer are those the header declares without one."""
    import os
    import re
    from svgp_vae_amd import gp_route
    header = open(os.path.join(os.path.dirname(svgp_vae_amd.__file__), "..", "include", "svgpvae_hip.h")).read()
    for entry in ABBR.values():
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % entry, header).group(1)
        assert ("state" in decl) == (entry not in gp_route._NO_STATE), (entry, decl)
