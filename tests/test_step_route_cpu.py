"""The launch schedule of the MNIST step (csrc/step_plan.hpp: step_plan, read back as text through svgp_mnist_step_route), pinned
without a GPU: which stage entry runs on which lane, where a side branch is forked and joined, where a collective is issued -- for
the stand-alone phases, the single-GPU step and the data-parallel step (three all-reduces, split gradient exchange, channel-sharded),
on either side of every shape predicate and under every schedule switch of DESIGN.md 6.4 that the step consults.

The expected routes were read by hand from the phase switch of csrc/api.hip and the data-parallel step of csrc/comm.hip as they stood
before the planner existed, and from DESIGN.md 6.1; they are not output of the planner.  ROUTES holds them in a short notation
(ABBR: one word per entry point; `s0:` / `s1:` put an op on side branch 0 / 1, everything else is on the caller's stream; `x:ARG`
appends an argument); the routes of test_routes_spelled_out are written in full."""
import ctypes as C
import os

import pytest

import svgp_vae_amd
from svgp_vae_amd import _lib

PHASE, STEP, DP = 0, 1, 2
SWITCHES = ["SVGP_DEC_SPLIT", "SVGP_ENC_KM_MERGE", "SVGP_SUM_MERGE", "SVGP_STAT_MERGE", "SVGP_AJI_DEC", "SVGP_DEC_FUSE",
            "SVGP_STAT_FOUR", "SVGP_KONLY_BRANCH", "SVGP_KBAR_BRANCH", "SVGP_STREAM_PROBE", "SVGP_SIDE_STREAMS", "SVGP_DP_PACK"]
MERGES = ["SVGP_DEC_SPLIT", "SVGP_ENC_KM_MERGE", "SVGP_SUM_MERGE", "SVGP_STAT_MERGE", "SVGP_AJI_DEC", "SVGP_DEC_FUSE"]

ABBR = {
    "enc": "svgp_mnist_encoder_kernel_matrix_fwd", "stats": "svgp_gp_stats_fwd", "tstats": "svgp_gp_titsias_stats",
    "pieces": "svgp_gp_factor_fwd_pieces", "defer": "svgp_gp_factor_fwd_defer_aji", "tail": "svgp_gp_factor_fwd_aji_tail",
    "bigf": "svgp_big_factor_fwd", "bigb": "svgp_big_factor_bwd",
    "post": "svgp_gp_posterior_fwd", "post_aji": "svgp_gp_posterior_fwd_with_aji", "tfwd": "svgp_gp_titsias_fwd",
    "dec_fused_aji": "svgp_mnist_decoder_fwd_bwd_data_pre_aji", "dec_fused": "svgp_mnist_decoder_fwd_bwd_data_pre",
    "dec_fwd_pre": "svgp_mnist_decoder_fwd_pre", "dec_bwd_pre_aji": "svgp_mnist_decoder_bwd_data_pre_aji",
    "dec_bwd_pre": "svgp_mnist_decoder_bwd_data_pre", "dec_fwd": "svgp_mnist_decoder_fwd", "dec_bwd": "svgp_mnist_decoder_bwd",
    "stats_bwd": "svgp_gp_stats_bwd", "early": "svgp_gp_factor_bwd_early", "late_a": "svgp_gp_factor_bwd_late_a",
    "late_b": "svgp_gp_factor_bwd_late_b", "kbar": "svgp_gp_factor_bwd_late_b_kbar", "channels": "svgp_gp_factor_bwd_late_b_channels",
    "final": "svgp_gp_factor_bwd_late_b_final", "sfw": "svgp_gp_stats_factor_bwd_wgrad", "nfw": "svgp_gp_factor_bwd_nofinal_wgrad",
    "nf": "svgp_gp_factor_bwd_nofinal", "rows": "svgp_gp_posterior_bwd_rows", "pbf": "svgp_gp_posterior_bwd_with_final",
    "post_bwd": "svgp_gp_posterior_bwd", "tbwd": "svgp_gp_titsias_bwd", "km": "svgp_kernel_matrix_bwd_partials",
    "encb": "svgp_mnist_encoder_bwd", "encb_km": "svgp_mnist_encoder_bwd_km", "encb_km_sum": "svgp_mnist_encoder_bwd_km_sum",
    "red": "svgp_mnist_grad_reduce_all", "redp": "svgp_mnist_grad_reduce_part", "adam": "svgp_adam_tf1_finalize",
    "noadam": "svgp_elbo_finalize_noadam",
    "ar": "allreduce", "rs": "reduce_scatter", "ag": "allgather", "pack": "pack", "unpack": "unpack", "gb": "group_begin",
    "ge": "group_end", "point": "point_begin", "end": "point_end",
}


def expand(route):
    lines = []
    for tok in route.split():
        lane = "main"
        if tok[:3] in ("s0:", "s1:"):
            lane, tok = "side" + tok[1], tok[3:]
        if tok in ("fork0", "fork1", "join0", "join1"):
            lines.append(f"{tok[:4]} side{tok[4]}")
            continue
        head, *args = tok.split(":")
        lines.append(" ".join([lane, ABBR[head]] + args))
    return lines


# ---- the table -------------------------------------------------------------------------------------------------------------------
# m <= 64, one GPU.  Phase 1 ends with the reverse statistics unless they ride in phase 2's first launch (sfw).
P0, P0_TIT = "enc stats", "enc stats tstats"
LARGE_P0 = "enc fork1 stats s1:pieces:K"                                      # 64 < m < 512, phases back to back: K-only branch
LARGE_P1_K = "pieces:SIG join1 pieces:KL fork1 post_aji s1:tail s1:early dec_fwd dec_bwd stats_bwd"
LARGE_P1 = "defer fork1 post_aji s1:tail s1:early dec_fwd dec_bwd stats_bwd"
LATE = "late_a join1 fork1 s1:kbar channels join1 final"
LATE_INLINE = "late_a join1 late_b"
LARGE_TAIL = "pbf km encb red"
# the four exchange points of the channel-sharded form, the symmetric block as it is / tile-packed; {f}: the fork of point 2
X1 = "point:1 gb rs:S rs:v ge end:1"
X1P = "point:1 pack:S:all gb rs:S:packed rs:v ge unpack:S:window end:1"
X2 = "point:2 {f} gb ag:Si ag:t ag:u ge end:2"
X2P = "point:2 pack:Si:window {f} gb ag:Si:packed ag:t ag:u ge unpack:Si:others end:2"
X3 = "point:3 gb rs:A2 rs:ud rs:td ge end:3"
X3P = "point:3 pack:A2:all gb rs:A2:packed rs:ud rs:td ge unpack:A2:window end:3"
X4 = "point:4 gb ag:Ssym ag:vbar ag:KL ge end:4"
X4P = "point:4 pack:Ssym:window gb ag:Ssym:packed ag:vbar ag:KL ge unpack:Ssym:all end:4"
SH_ROWS = "post s1:bigf:TAIL s1:bigb:EARLY dec_fwd dec_bwd stats_bwd"
SH_LATE = "join1 bigb:LATE_A fork1 s1:bigb:KBAR bigb:CHANNELS join1 bigb:FINAL"
SH_TAIL = "post_bwd km encb red ar:gradC adam"


def _sharded(x1, x2, x3, x4, konly=True, fork=True, late=SH_LATE):
    head = "enc fork1 stats s1:bigf:K " + x1 + " bigf:SIG join1 bigf:KL" if konly else "enc stats " + x1 + " bigf:HEAD"
    rows = SH_ROWS if fork else "post bigf:TAIL dec_fwd dec_bwd stats_bwd"
    return " ".join([head, x2.format(f="fork1" if fork else ""), rows, x3, late if fork else "bigb:ALL", x4, SH_TAIL])


ROUTES = {
    # single-GPU step, m <= 64
    "step m<=32": "enc stats defer post dec_fused_aji sfw rows encb_km_sum red adam",
    "step m<=32 no adam": "enc stats defer post dec_fused_aji sfw rows encb_km_sum red noadam",
    "step 32<m<=64": "enc stats defer post_aji dec_fused sfw rows encb_km_sum red adam",
    "step m<=32 L>56": "enc stats defer post dec_fused_aji stats_bwd nfw rows encb_km_sum red adam",
    "step 32<m<=64 L>56": "enc stats defer post_aji dec_fused stats_bwd nfw rows encb_km_sum red adam",
    "step m<=64 titsias": "enc stats tstats defer post_aji tfwd dec_fused stats_bwd nfw pbf tbwd encb_km red adam",
    "step m<=32 DEC_SPLIT=0": "enc stats defer post_aji dec_fwd dec_bwd stats_bwd nf rows encb_km_sum red adam",
    "step m<=32 ENC_KM_MERGE=0": "enc stats defer post dec_fused_aji sfw pbf km encb red adam",
    "step m<=32 SUM_MERGE=0": "enc stats defer post dec_fused_aji sfw pbf encb_km red adam",
    "step m<=32 DEC_FUSE=0": "enc stats defer post dec_fwd_pre dec_bwd_pre_aji sfw rows encb_km_sum red adam",
    "step 32<m<=64 DEC_FUSE=0": "enc stats defer post_aji dec_fwd_pre dec_bwd_pre sfw rows encb_km_sum red adam",
    "step m<=32 SIDE_STREAMS=1": "enc stats defer post dec_fused_aji sfw pbf fork0 s0:km encb join0 red adam",
    "step m<=64 merges off": "enc stats defer post_aji dec_fwd dec_bwd stats_bwd nf pbf km encb red adam",
    # single-GPU step, m > 64
    "step 64<m<512": " ".join([LARGE_P0, LARGE_P1_K, LATE, LARGE_TAIL, "adam"]),
    "step m>=512": " ".join([P0, LARGE_P1, LATE, LARGE_TAIL, "adam"]),
    "step 64<m<512 KBAR_BRANCH=0": " ".join([LARGE_P0, LARGE_P1_K, LATE_INLINE, LARGE_TAIL, "adam"]),
    "step m>64 SIDE_STREAMS=0": "enc stats defer post_aji tail dec_fwd dec_bwd stats_bwd nf pbf km encb red adam",
    "step 64<m<512 SIDE_STREAMS=1": " ".join([LARGE_P0, LARGE_P1_K, LATE, "pbf fork0 s0:km encb join0 red adam"]),
    "step m>64 titsias": "enc stats tstats defer post_aji tail tfwd dec_fwd dec_bwd stats_bwd nf pbf tbwd km encb red adam",
    # stand-alone phases: each joins what it forks; no K-only branch (it needs back-to-back phases), no statistics rider
    "phase 0": P0,
    "phase 0 titsias": P0_TIT,
    "phase 1 m<=32": "defer post dec_fused_aji stats_bwd",
    "phase 1 m>64": LARGE_P1 + " join1",
    "phase 1 m>64 SIDE_STREAMS=0": "defer post_aji tail dec_fwd dec_bwd stats_bwd",
    "phase 2 m<=64": "nfw rows encb_km_sum red",
    "phase 2 m<=64 SIDE_STREAMS=1": "nfw pbf fork0 s0:km encb join0 red",
    "phase 2 m>64 early issued": " ".join([LATE, LARGE_TAIL]),
    "phase 2 m>64": "nf " + LARGE_TAIL,
    "phase 3": "adam",
    "phase 3 no adam": "noadam",
    "phase 4 m<=64": "nfw pbf km redp:1",
    "phase 4 m>64 early issued": LATE + " pbf km redp:1",
    "phase 4 m>64": "nf pbf km redp:1",
    "phase 5": "encb redp:2",
    # data parallel, an all-reduce behind each of the first three phases: no statistics rider; a branch may stay open across a phase
    "dp m<=32": "enc stats ar:statA defer post dec_fused_aji stats_bwd ar:statB nfw rows encb_km_sum red ar:gradC adam",
    "dp m<=32 split": "enc stats ar:statA defer post dec_fused_aji stats_bwd ar:statB nfw pbf km redp:1 fork1 s1:ar:gradC_hi "
                      "encb redp:2 ar:gradC_lo join1 adam",
    "dp m<=64 titsias": "enc stats tstats ar:statA defer post_aji tfwd dec_fused stats_bwd ar:statB nfw pbf tbwd encb_km red "
                        "ar:gradC adam",
    "dp m>64 titsias": "enc stats tstats ar:statA defer post_aji tail tfwd dec_fwd dec_bwd stats_bwd ar:statB nf pbf tbwd km encb "
                       "red ar:gradC adam",
    "dp 64<m<512 not sharded": " ".join([LARGE_P0, "ar:statA", LARGE_P1_K, "ar:statB", LATE, LARGE_TAIL, "ar:gradC adam"]),
    "dp 64<m<512 not sharded split": " ".join([LARGE_P0, "ar:statA", LARGE_P1_K, "ar:statB", LATE, "pbf km redp:1 fork1 "
                                               "s1:ar:gradC_hi encb redp:2 ar:gradC_lo join1 adam"]),
    # data parallel, channel-sharded
    "sharded 64<m<512": _sharded(X1, X2, X3, X4),
    "sharded 64<m<512 DP_PACK=1": _sharded(X1P, X2P, X3P, X4P),
    "sharded 64<m<512 KONLY_BRANCH=0": _sharded(X1, X2, X3, X4, konly=False),
    "sharded 64<m<512 KBAR_BRANCH=0": _sharded(X1, X2, X3, X4, late="join1 bigb:LATE"),
    "sharded m>64 SIDE_STREAMS=0": _sharded(X1, X2, X3, X4, konly=False, fork=False),
    "sharded m>=512": _sharded(X1P, X2P, X3P, X4P, konly=False),
    "sharded m>=512 DP_PACK=0": _sharded(X1, X2, X3, X4, konly=False),
}

# ---- the classes: (expected entry, form, phase, cfg fields, call arguments, environment) ------------------------------------------
def _c(key, form, m=32, L=16, env=None, phase=0, G=1, rank=0, adam=1, early=0, **cfg):
    return (key, form, phase, dict(m=m, L=L, **cfg), dict(nranks=G, rank=rank, adam=adam, early_issued=early), env or {})


def _off(*names):
    return {"SVGP_" + n: "0" for n in names}


CLASSES = [
    # shapes, single-GPU step, default switches
    _c("step m<=32", STEP, m=32), _c("step 32<m<=64", STEP, m=33), _c("step 32<m<=64", STEP, m=64),
    _c("step 64<m<512", STEP, m=65), _c("step 64<m<512", STEP, m=256), _c("step 64<m<512", STEP, m=511), _c("step m>=512", STEP, m=512),
    _c("step m<=32", STEP, L=56), _c("step m<=32 L>56", STEP, L=57), _c("step 32<m<=64 L>56", STEP, m=64, L=57),
    _c("step 64<m<512", STEP, m=256, L=57),
    _c("step m<=64 titsias", STEP, titsias=1), _c("step m>64 titsias", STEP, m=130, titsias=1),
    _c("step m<=32", STEP, kl_form=1), _c("step m<=32 no adam", STEP, adam=0),
    # switches, single-GPU step: each alone ...
    _c("step m<=32 DEC_SPLIT=0", STEP, env=_off("DEC_SPLIT")), _c("step m<=32 ENC_KM_MERGE=0", STEP, env=_off("ENC_KM_MERGE")),
    _c("step m<=32 SUM_MERGE=0", STEP, env=_off("SUM_MERGE")), _c("step m<=32 L>56", STEP, env=_off("STAT_MERGE")),
    _c("step 32<m<=64", STEP, env=_off("AJI_DEC")), _c("step m<=32 DEC_FUSE=0", STEP, env=_off("DEC_FUSE")),
    _c("step 32<m<=64 DEC_FUSE=0", STEP, m=64, env=_off("DEC_FUSE")),
    _c("step m<=32", STEP, env=_off("KONLY_BRANCH")), _c("step m<=32", STEP, env=_off("KBAR_BRANCH")),
    _c("step m<=32", STEP, env={"SVGP_DP_PACK": "1"}), _c("step m<=32", STEP, env=_off("DP_PACK")),
    _c("step m<=32", STEP, env=_off("SIDE_STREAMS")), _c("step m<=32 SIDE_STREAMS=1", STEP, env={"SVGP_SIDE_STREAMS": "1"}),
    _c("step m<=64 merges off", STEP, env=_off(*[n[5:] for n in MERGES])),
    _c("step m<=64 merges off", STEP, m=64, env=_off(*[n[5:] for n in MERGES])),
    # ... and the pairs in which one gates the other
    _c("step m<=32 DEC_SPLIT=0", STEP, env=_off("DEC_SPLIT", "AJI_DEC")), _c("step m<=32 DEC_SPLIT=0", STEP, env=_off("DEC_SPLIT", "STAT_MERGE")),
    _c("step m<=32 DEC_SPLIT=0", STEP, env=_off("DEC_SPLIT", "DEC_FUSE")),
    _c("step 32<m<=64 DEC_FUSE=0", STEP, env=_off("AJI_DEC", "DEC_FUSE")),
    _c("step m<=32 ENC_KM_MERGE=0", STEP, env=_off("ENC_KM_MERGE", "SUM_MERGE")),
    _c("step m<=32 SIDE_STREAMS=1", STEP, env={"SVGP_SIDE_STREAMS": "1", **_off("ENC_KM_MERGE")}),
    _c("step m<=32 SIDE_STREAMS=1", STEP, env={"SVGP_SIDE_STREAMS": "1", **_off("SUM_MERGE")}),
    # m > 64: the large-m switches; the m <= 64 merges do nothing there
    _c("step m>=512", STEP, m=256, env=_off("KONLY_BRANCH")), _c("step 64<m<512 KBAR_BRANCH=0", STEP, m=256, env=_off("KBAR_BRANCH")),
    _c("step m>64 SIDE_STREAMS=0", STEP, m=256, env=_off("SIDE_STREAMS")), _c("step m>64 SIDE_STREAMS=0", STEP, m=512, env=_off("SIDE_STREAMS")),
    _c("step 64<m<512 SIDE_STREAMS=1", STEP, m=256, env={"SVGP_SIDE_STREAMS": "1"}),
    _c("step 64<m<512", STEP, m=256, env=_off(*[n[5:] for n in MERGES])), _c("step 64<m<512", STEP, m=256, env={"SVGP_DP_PACK": "1"}),
    _c("step m>64 titsias", STEP, m=130, titsias=1, env=_off("SIDE_STREAMS")),
    # stand-alone phases
    _c("phase 0", PHASE, phase=0), _c("phase 0", PHASE, phase=0, m=256), _c("phase 0 titsias", PHASE, phase=0, titsias=1),
    _c("phase 1 m<=32", PHASE, phase=1), _c("phase 1 m<=32", PHASE, phase=1, env=_off("STAT_MERGE")),
    _c("phase 1 m>64", PHASE, phase=1, m=256), _c("phase 1 m>64", PHASE, phase=1, m=512),
    _c("phase 1 m>64 SIDE_STREAMS=0", PHASE, phase=1, m=256, env=_off("SIDE_STREAMS")),
    _c("phase 2 m<=64", PHASE, phase=2), _c("phase 2 m<=64", PHASE, phase=2, early=1),
    _c("phase 2 m<=64 SIDE_STREAMS=1", PHASE, phase=2, env={"SVGP_SIDE_STREAMS": "1"}),
    _c("phase 2 m>64 early issued", PHASE, phase=2, m=256, early=1), _c("phase 2 m>64", PHASE, phase=2, m=256, early=0),
    _c("phase 3", PHASE, phase=3), _c("phase 3", PHASE, phase=3, m=256), _c("phase 3 no adam", PHASE, phase=3, adam=0),
    _c("phase 4 m<=64", PHASE, phase=4), _c("phase 4 m>64 early issued", PHASE, phase=4, m=256, early=1),
    _c("phase 4 m>64", PHASE, phase=4, m=256), _c("phase 5", PHASE, phase=5), _c("phase 5", PHASE, phase=5, m=256),
    # data parallel: G = 3 does not divide L = 16, G = 2 does
    _c("dp m<=32", DP, G=3), _c("dp m<=32", DP, G=2, rank=1), _c("dp m<=32", DP, G=2, kl_form=1), _c("dp m<=32", DP, G=3, env=_off("STAT_MERGE")),
    _c("dp m<=32 split", DP, G=3, split_grad_exchange=1), _c("dp m<=32 split", DP, G=2, split_grad_exchange=1),
    _c("dp m<=64 titsias", DP, G=2, titsias=1), _c("dp m>64 titsias", DP, G=2, m=130, titsias=1),
    _c("dp 64<m<512 not sharded", DP, G=3, m=256), _c("dp 64<m<512 not sharded split", DP, G=3, m=256, split_grad_exchange=1),
    _c("sharded 64<m<512", DP, G=2, m=256), _c("sharded 64<m<512", DP, G=2, rank=1, m=65), _c("sharded 64<m<512", DP, G=2, m=511),
    _c("sharded 64<m<512", DP, G=2, m=256, split_grad_exchange=1), _c("sharded 64<m<512", DP, G=2, m=256, env=_off("DP_PACK")),
    _c("sharded 64<m<512 DP_PACK=1", DP, G=2, m=256, env={"SVGP_DP_PACK": "1"}),
    _c("sharded 64<m<512 KONLY_BRANCH=0", DP, G=2, m=256, env=_off("KONLY_BRANCH")),
    _c("sharded 64<m<512 KBAR_BRANCH=0", DP, G=2, m=256, env=_off("KBAR_BRANCH")),
    _c("sharded m>64 SIDE_STREAMS=0", DP, G=2, m=256, env=_off("SIDE_STREAMS")),
    _c("sharded m>=512", DP, G=2, m=512), _c("sharded m>=512 DP_PACK=0", DP, G=2, m=512, env=_off("DP_PACK")),
]


@pytest.fixture(scope="module", autouse=True)
def _library():
    if not os.path.exists(svgp_vae_amd.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _route(monkeypatch, form, phase, cfg, args, env, cap=8192):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    b = 64 if args["nranks"] == 1 or cfg.get("kl_form") else 32
    kw = dict(b=b, b_global=64, M=8, n_obj=400, N_train=4050.0, jitter=1e-6)
    kw.update(cfg)
    buf = C.create_string_buffer(cap)
    _lib.call("svgp_mnist_step_route", C.byref(_lib.MnistCfg(**kw)), form, phase, args["nranks"], args["rank"], args["adam"],
              args["early_issued"], buf, cap)
    return buf.value.decode().splitlines()


@pytest.mark.parametrize("case", CLASSES, ids=lambda c: f"{c[0]} | form {c[1]} phase {c[2]} {c[3]} {c[4]} {c[5]}".replace("SVGP_", ""))
def test_every_class_takes_its_route(monkeypatch, case):
    key, form, phase, cfg, args, env = case
    assert _route(monkeypatch, form, phase, cfg, args, env) == expand(ROUTES[key])


def test_every_table_entry_is_reached_and_every_switch_and_shape_is_covered():
    assert {c[0] for c in CLASSES} == set(ROUTES)
    ms = {c[3]["m"] for c in CLASSES}
    assert {32, 33, 64, 65, 511, 512} <= ms and {16, 56, 57} <= {c[3]["L"] for c in CLASSES}
    flipped = {frozenset(c[5].items()) for c in CLASSES}
    for name in MERGES + ["SVGP_KONLY_BRANCH", "SVGP_KBAR_BRANCH", "SVGP_DP_PACK", "SVGP_SIDE_STREAMS"]:
        assert frozenset({(name, "0")}) in flipped, name
    assert frozenset({("SVGP_DP_PACK", "1")}) in flipped and frozenset({("SVGP_SIDE_STREAMS", "1")}) in flipped
    assert {(c[1], c[2]) for c in CLASSES} >= {(PHASE, p) for p in range(6)} | {(STEP, 0), (DP, 0)}
    # every stage entry and every exchange word of the notation occurs in some route
    used = {ln.split()[1] for r in ROUTES.values() for ln in expand(r) if not ln.startswith(("fork", "join"))}
    assert used == set(ABBR.values())


STEP32 = ["svgp_mnist_encoder_kernel_matrix_fwd", "svgp_gp_stats_fwd", "svgp_gp_factor_fwd_defer_aji", "svgp_gp_posterior_fwd",
          "svgp_mnist_decoder_fwd_bwd_data_pre_aji", "svgp_gp_stats_factor_bwd_wgrad", "svgp_gp_posterior_bwd_rows",
          "svgp_mnist_encoder_bwd_km_sum", "svgp_mnist_grad_reduce_all", "svgp_adam_tf1_finalize"]
STEP256_HEAD = ["main svgp_mnist_encoder_kernel_matrix_fwd", "fork side1", "main svgp_gp_stats_fwd", "side1 svgp_gp_factor_fwd_pieces K",
                "main svgp_gp_factor_fwd_pieces SIG", "join side1", "main svgp_gp_factor_fwd_pieces KL"]
STEP256_REST = ["fork side1", "main svgp_gp_posterior_fwd_with_aji", "side1 svgp_gp_factor_fwd_aji_tail", "side1 svgp_gp_factor_bwd_early",
                "main svgp_mnist_decoder_fwd", "main svgp_mnist_decoder_bwd", "main svgp_gp_stats_bwd", "main svgp_gp_factor_bwd_late_a",
                "join side1", "fork side1", "side1 svgp_gp_factor_bwd_late_b_kbar", "main svgp_gp_factor_bwd_late_b_channels",
                "join side1", "main svgp_gp_factor_bwd_late_b_final", "main svgp_gp_posterior_bwd_with_final",
                "main svgp_kernel_matrix_bwd_partials", "main svgp_mnist_encoder_bwd", "main svgp_mnist_grad_reduce_all",
                "main svgp_adam_tf1_finalize"]


def _main(names):
    return ["main " + n for n in names]


def test_routes_spelled_out(monkeypatch):
    """Routes in full, as DESIGN.md 6.1 / 6.2 describe them: the ten launches of config 2 and their variants, the two-branch order of
    the large-m step, the three all-reduces."""
    def route(form=STEP, phase=0, env=None, G=1, early=0, **cfg):
        cfg.setdefault("m", 32), cfg.setdefault("L", 16)
        return _route(monkeypatch, form, phase, cfg, dict(nranks=G, rank=0, adam=1, early_issued=early), env or {})

    assert route() == _main(STEP32)
    r64 = list(STEP32)
    r64[3], r64[4] = "svgp_gp_posterior_fwd_with_aji", "svgp_mnist_decoder_fwd_bwd_data_pre"
    assert route(m=64) == _main(r64)
    assert route(L=57) == _main(STEP32[:5] + ["svgp_gp_stats_bwd", "svgp_gp_factor_bwd_nofinal_wgrad"] + STEP32[6:]) and len(route(L=57)) == 11
    assert route(DP, G=3) == _main(STEP32[:2]) + ["main allreduce statA"] + _main(STEP32[2:5] + ["svgp_gp_stats_bwd"]) + \
        ["main allreduce statB"] + _main(["svgp_gp_factor_bwd_nofinal_wgrad"] + STEP32[6:9]) + ["main allreduce gradC"] + _main(STEP32[9:])
    assert route(titsias=1) == _main([
        "svgp_mnist_encoder_kernel_matrix_fwd", "svgp_gp_stats_fwd", "svgp_gp_titsias_stats",
        "svgp_gp_factor_fwd_defer_aji", "svgp_gp_posterior_fwd_with_aji", "svgp_gp_titsias_fwd", "svgp_mnist_decoder_fwd_bwd_data_pre",
        "svgp_gp_stats_bwd",
        "svgp_gp_factor_bwd_nofinal_wgrad", "svgp_gp_posterior_bwd_with_final", "svgp_gp_titsias_bwd", "svgp_mnist_encoder_bwd_km",
        "svgp_mnist_grad_reduce_all", "svgp_adam_tf1_finalize"])
    assert route(env={n: "0" for n in MERGES}) == _main([
        "svgp_mnist_encoder_kernel_matrix_fwd", "svgp_gp_stats_fwd",
        "svgp_gp_factor_fwd_defer_aji", "svgp_gp_posterior_fwd_with_aji", "svgp_mnist_decoder_fwd", "svgp_mnist_decoder_bwd", "svgp_gp_stats_bwd",
        "svgp_gp_factor_bwd_nofinal", "svgp_gp_posterior_bwd_with_final", "svgp_kernel_matrix_bwd_partials", "svgp_mnist_encoder_bwd",
        "svgp_mnist_grad_reduce_all", "svgp_adam_tf1_finalize"])
    assert route(env={"SVGP_SIDE_STREAMS": "1"}) == _main(STEP32[:6] + ["svgp_gp_posterior_bwd_with_final"]) + \
        ["fork side0", "side0 svgp_kernel_matrix_bwd_partials", "main svgp_mnist_encoder_bwd", "join side0"] + _main(STEP32[8:])
    assert route(m=256) == STEP256_HEAD + STEP256_REST
    assert route(m=512) == ["main svgp_mnist_encoder_kernel_matrix_fwd", "main svgp_gp_stats_fwd", "main svgp_gp_factor_fwd_defer_aji"] + STEP256_REST
    off = route(m=256, env={"SVGP_SIDE_STREAMS": "0"})
    assert not [ln for ln in off if ln.startswith(("fork", "join", "side"))]
    assert off == _main(["svgp_mnist_encoder_kernel_matrix_fwd", "svgp_gp_stats_fwd",
                         "svgp_gp_factor_fwd_defer_aji", "svgp_gp_posterior_fwd_with_aji", "svgp_gp_factor_fwd_aji_tail",
                         "svgp_mnist_decoder_fwd", "svgp_mnist_decoder_bwd", "svgp_gp_stats_bwd", "svgp_gp_factor_bwd_nofinal",
                         "svgp_gp_posterior_bwd_with_final", "svgp_kernel_matrix_bwd_partials", "svgp_mnist_encoder_bwd",
                         "svgp_mnist_grad_reduce_all", "svgp_adam_tf1_finalize"])
    assert route(PHASE, 1, m=256)[-1] == "join side1"
    assert not [ln for ln in route(PHASE, 0, m=256) if ln.startswith("fork")]


def test_channel_sharded_route_spelled_out(monkeypatch):
    """m = 256, L = 16 on two ranks, tile-packed: the K-only branch forked before the forward statistics and issued behind them; at
    point 2 the fork between the packing of the rank's window and the collective, the unpack of the other ranks' windows behind the
    collective; TAIL and EARLY issued behind the row stage; the join behind point 3, in front of LATE_A."""
    got = _route(monkeypatch, DP, 0, dict(m=256, L=16), dict(nranks=2, rank=1, adam=1, early_issued=0), {"SVGP_DP_PACK": "1"})
    assert got == [
        "main svgp_mnist_encoder_kernel_matrix_fwd",
        "fork side1",
        "main svgp_gp_stats_fwd",
        "side1 svgp_big_factor_fwd K",
        "main point_begin 1", "main pack S all", "main group_begin", "main reduce_scatter S packed", "main reduce_scatter v",
        "main group_end", "main unpack S window", "main point_end 1",
        "main svgp_big_factor_fwd SIG", "join side1", "main svgp_big_factor_fwd KL",
        "main point_begin 2", "main pack Si window",
        "fork side1",
        "main group_begin", "main allgather Si packed", "main allgather t", "main allgather u", "main group_end",
        "main unpack Si others", "main point_end 2",
        "main svgp_gp_posterior_fwd",
        "side1 svgp_big_factor_fwd TAIL", "side1 svgp_big_factor_bwd EARLY",
        "main svgp_mnist_decoder_fwd", "main svgp_mnist_decoder_bwd",
        "main svgp_gp_stats_bwd",
        "main point_begin 3", "main pack A2 all", "main group_begin", "main reduce_scatter A2 packed", "main reduce_scatter ud",
        "main reduce_scatter td", "main group_end", "main unpack A2 window", "main point_end 3",
        "join side1",
        "main svgp_big_factor_bwd LATE_A",
        "fork side1",
        "side1 svgp_big_factor_bwd KBAR",
        "main svgp_big_factor_bwd CHANNELS",
        "join side1",
        "main svgp_big_factor_bwd FINAL",
        "main point_begin 4", "main pack Ssym window", "main group_begin", "main allgather Ssym packed", "main allgather vbar",
        "main allgather KL", "main group_end", "main unpack Ssym all", "main point_end 4",
        "main svgp_gp_posterior_bwd", "main svgp_kernel_matrix_bwd_partials", "main svgp_mnist_encoder_bwd", "main svgp_mnist_grad_reduce_all",
        "main allreduce gradC",
        "main svgp_adam_tf1_finalize"]


def test_channel_sharded_route_without_side_branches_spelled_out(monkeypatch):
    """The same step with SVGP_SIDE_STREAMS=0 (m = 256 < 512: blocks as they are on the wire): no fork, no join, nothing on a side
    lane; the whole head of the window factor stage in one call behind point 1, TAIL in line behind the row stage, the whole
    reverse factor stage in one call behind point 3."""
    got = _route(monkeypatch, DP, 0, dict(m=256, L=16), dict(nranks=2, rank=0, adam=1, early_issued=0), {"SVGP_SIDE_STREAMS": "0"})
    assert got == [
        "main svgp_mnist_encoder_kernel_matrix_fwd",
        "main svgp_gp_stats_fwd",
        "main point_begin 1", "main group_begin", "main reduce_scatter S", "main reduce_scatter v", "main group_end", "main point_end 1",
        "main svgp_big_factor_fwd HEAD",
        "main point_begin 2", "main group_begin", "main allgather Si", "main allgather t", "main allgather u", "main group_end",
        "main point_end 2",
        "main svgp_gp_posterior_fwd",
        "main svgp_big_factor_fwd TAIL",
        "main svgp_mnist_decoder_fwd", "main svgp_mnist_decoder_bwd",
        "main svgp_gp_stats_bwd",
        "main point_begin 3", "main group_begin", "main reduce_scatter A2", "main reduce_scatter ud", "main reduce_scatter td",
        "main group_end", "main point_end 3",
        "main svgp_big_factor_bwd ALL",
        "main point_begin 4", "main group_begin", "main allgather Ssym", "main allgather vbar", "main allgather KL", "main group_end",
        "main point_end 4",
        "main svgp_gp_posterior_bwd", "main svgp_kernel_matrix_bwd_partials", "main svgp_mnist_encoder_bwd", "main svgp_mnist_grad_reduce_all",
        "main allreduce gradC",
        "main svgp_adam_tf1_finalize"]


def test_bad_arguments_are_refused_with_a_message(monkeypatch):
    cfg = dict(m=32, L=16)
    with pytest.raises(svgp_vae_amd.SvgpError, match="phase 6 out of range 0..5"):
        _route(monkeypatch, PHASE, 6, cfg, dict(nranks=1, rank=0, adam=1, early_issued=0), {})
    with pytest.raises(svgp_vae_amd.SvgpError, match="rank 2 of 2"):
        _route(monkeypatch, DP, 0, cfg, dict(nranks=2, rank=2, adam=1, early_issued=0), {})
    with pytest.raises(svgp_vae_amd.SvgpError, match="form 3"):
        _route(monkeypatch, 3, 0, cfg, dict(nranks=1, rank=0, adam=1, early_issued=0), {})
    with pytest.raises(svgp_vae_amd.SvgpError, match="more than 64 bytes"):
        _route(monkeypatch, STEP, 0, cfg, dict(nranks=1, rank=0, adam=1, early_issued=0), {}, cap=64)
