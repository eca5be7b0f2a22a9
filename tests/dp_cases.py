"""The data-parallel forms of the MNIST step on ONE device: case table, problems, the float64 references, the rank-sum restatement,
the oracle's own one-ulp response, the virtual-rank runners and the comparison, shared by tests/test_gpu_dp_envelope.py (GPU) and
tests/test_dp_envelope_oracle_cpu.py (guard).

Virtual ranks are G engines on one device (rank r of G holds rows shard_rows(b, G, r)); what the collectives do between real ranks
is done by hand: the exchange blocks of the row-sharded schedules are summed across the engines, the points of the channel-sharded
schedule go through engine.virtual_exchange.  ONE step without the optimiser; EVERY rank is then compared with the oracle on the
GLOBAL batch -- scalars, the reduced gradients of every parameter, the forward fields.

Which field is complete where after a step (engine.ShardedExchange, csrc/gp_large.hip, csrc/step_plan.hpp):
  row fields (ROW_FIELDS: encoder outputs, Kn, knn, q, p_m, p_v, e, d, z, recon, and W = Kn Ki K for m > 64, which takes the place
      of M2 as in helpers._compare_step): the rank's rows [lo, hi) on every route;
  row-sharded routes (statA = S | v and statB = A2 | ud | td all-reduced, the factor stages replicated): K, Ki, ldK, S, v, Si, t,
      G, A, Aji, mu_hat, u, KL and M2 are complete on every rank;
  channel-sharded route (point 1 reduce-scatters S, v over the channels, the window factor stage svgp_big_factor_fwd writes Si, t,
      G, A, Aji, mu_hat, u, KL at its channels [l0, l0 + nl) only, point 2 all-gathers Si, t, u and point 4 KL): K, Ki, ldK, Si, t, u
      and KL are complete on every rank; S, v, G, A, Aji, mu_hat are compared on the owner's window only (WINDOW_FIELDS).

Bars, the project's own: Hensman cases helpers.FWD_TOL / SCALAR_TOL / GRAD_TOL (1e-9 / 1e-9 / 1e-7), Titsias cases those of
tests/titsias_cases.py against the literal b x b oracle.  The cases marked `ill` are held to max(bar, 20 x the oracle's own one-ulp
response) per quantity (the self_consistency rule of helpers._compare_step); at most the two m = 520 cases and the 5-row case may
be so marked.

What stays uncovered: STEP_FORM_DP (svgp_mnist_train_step_dp) with more than one rank needs more than one device.  On one GPU the
form is covered at one rank (ENTRY_CASES, a 1-rank RcclComm) and the rank arithmetic through the phase and stage entries (CASES);
the two are not covered in one run."""
import contextlib
import functools
import math
import os

import torch

from oracle import staged_gp as SG
from oracle import svgpvae_oracle as O
from tests import helpers as H
from tests import titsias_cases as TC

DT = torch.float64
N_TRAIN, C_MA, LAGRANGE, ALPHA, BETA, KAPPA2 = 4050.0, 0.02, 1.3, 0.9, 0.001, 0.02
SCALARS, GECO_SCALARS = TC.SCALARS, TC.GECO_SCALARS
ROW_FIELDS = ("qnet_mu", "qnet_var_raw", "qnet_var", "Kn", "knn", "q", "p_m", "p_v", "e", "d", "z", "recon", "W")
WINDOW_FIELDS = ("S", "v", "G", "A", "Aji", "mu_hat")          # (L, ...) fields only the channels' owner holds, channel-sharded route
TITSIAS_FIELDS = ("qnet_mu", "qnet_var", "p_m", "p_v", "z", "recon")
ROWS, ROWS_LARGE, CHANNELS, TITSIAS = "rows", "rows_large", "channels", "titsias"
SPLIT_PHASES = ((0, "statA"), (1, "statB"), (4, "gradC_tail"), (5, "gradC_head"), (3, None))
PLAIN_PHASES = ((0, "statA"), (1, "statB"), (2, "gradC"), (3, None))


def _case(route, G, b, m, L, M, geco, note, jitter=None, **kw):
    cs = dict(route=route, G=G, b=b, m=m, L=L, M=M, geco=geco, note=note,
              jitter=(1e-6 if m < 64 else 1e-4) if jitter is None else jitter, N_train=float(kw.pop("N_train", N_TRAIN)),
              normalize=kw.pop("normalize", False), with_table=kw.pop("with_table", True), clip_qs=kw.pop("clip_qs", True),
              titsias=route == TITSIAS, split_grad_exchange=kw.pop("split", False), single_stat_block=kw.pop("one_block", None),
              pack=kw.pop("pack", None), b_max=kw.pop("b_max", -(-b // G)), ill=kw.pop("ill", False), seed=kw.pop("seed", None))
    assert not kw, kw
    return cs


# name: route, G, global b, m, L, M, GECO, the form the case pins.  The problem is helpers.toy_problem(n_obj=60, seed=500 + index).
# N_train is 4050 and the jitter 1e-6 (m < 64) / 1e-4 unless the row says otherwise.  Rows that say otherwise failed the guard's (a)
# or (b) as first drawn up (tests/test_dp_envelope_oracle_cpu.py; the toy inducing points at m > 64 are close to rank-deficient, and
# c = N_train / b = 40 .. 60 amplifies that): they took N_train = 2 b, as tests/test_gpu_dp_virtual.py does, a larger jitter, the
# normalised object kernel or another seed -- never a wider bar -- until the response kept a factor of four below bar / 100 (it moves
# with the host's CPU and thread count).
CASES = {
    # row-sharded, m <= 64: the phases in lockstep, the exchange blocks summed by hand
    "m1": _case(ROWS, 2, 60, 1, 4, 3, True, "256 rows per workgroup"),
    "m2": _case(ROWS, 2, 60, 2, 3, 3, False, "128 rows per workgroup", clip_qs=False),
    "m7": _case(ROWS, 3, 60, 7, 5, 3, True, "36 rows per workgroup, three ranks", with_table=False),
    "m31": _case(ROWS, 3, 150, 31, 40, 8, False, "generic instance below kern<32>", normalize=True),
    "m32L17": _case(ROWS, 2, 150, 32, 17, 8, True, "kern<32>, odd L"),
    "m33": _case(ROWS, 2, 150, 33, 40, 8, False, "four-matrix form, the inverse in the row stage", clip_qs=False),
    "m64L64": _case(ROWS, 2, 200, 64, 64, 16, True, "LDS limit at the largest L", with_table=False),
    "m64L1": _case(ROWS, 4, 64, 64, 1, 16, False, "one channel, four ranks", normalize=True),
    "L56": _case(ROWS, 2, 256, 32, 56, 8, True, "last L at which the single-GPU step lets the reverse statistics ride", seed=701),
    "L57": _case(ROWS, 2, 256, 32, 57, 8, False, "first L past it"),
    "ragged8": _case(ROWS, 8, 210, 32, 16, 8, True, "ragged rows 27, 27, 26 x 6", seed=703),
    "rows5": _case(ROWS, 3, 5, 3, 3, 3, False, "ranks of 2, 2, 1 rows"),
    "cap127": _case(ROWS, 2, 254, 32, 16, 8, True, "capacity 127: one statistics partial per rank"),
    "cap128": _case(ROWS, 2, 256, 32, 16, 8, False, "capacity 128: four partials"),
    "cap129": _case(ROWS, 2, 257, 16, 16, 4, True, "capacity 129, the second rank one row below capacity", b_max=129, seed=711),
    "one_block": _case(ROWS, 2, 256, 32, 16, 8, False, "single_stat_block at the four-partial capacity", one_block=True, seed=713),
    "one_block_m31": _case(ROWS, 3, 150, 31, 17, 8, True, "single_stat_block, three ranks", one_block=True),
    "split_m31": _case(ROWS, 2, 150, 31, 17, 8, False, "split gradient exchange, phases 0, 1, 4, 5, 3", split=True, seed=712),
    "split_m64": _case(ROWS, 2, 200, 64, 64, 16, True, "split gradient exchange at the LDS limit", split=True),
    # row-sharded, m > 64, Hensman, L % G != 0: the replicated factor stages with rep_weight in svgp_big_factor_bwd
    "big72": _case(ROWS_LARGE, 2, 96, 72, 3, 16, False, "first large-m shape, L % 2 == 1", N_train=192, jitter=1e-2, normalize=True),
    "big65": _case(ROWS_LARGE, 2, 70, 65, 1, 16, True, "first global-memory m, one channel", N_train=140, jitter=1e-2, seed=702),
    "big72L22": _case(ROWS_LARGE, 3, 99, 72, 22, 16, False, "decoder reverse pass in two launches", N_train=198, jitter=1e-2, normalize=True,
                      with_table=False),
    "big130": _case(ROWS_LARGE, 3, 150, 130, 5, 24, True, "no multiple of the 64-wide tiles", N_train=300, jitter=1e-2, normalize=True),
    "big260": _case(ROWS_LARGE, 2, 80, 260, 3, 128, False, "largest m below the potrf + potri inverse", N_train=160, jitter=1e-3,
                    normalize=True),
    "big520": _case(ROWS_LARGE, 2, 64, 520, 3, 128, True, "potrf + potri inverse; ill-conditioned", jitter=1e-3, ill=True),
    "big72split": _case(ROWS_LARGE, 2, 96, 72, 3, 16, True, "split gradient exchange on the large-m path", N_train=192, jitter=1e-2,
                        normalize=True, split=True),
    # channel-sharded: sharded_stages + virtual_exchange
    "ch65": _case(CHANNELS, 2, 70, 65, 2, 16, False, "one channel per rank, packed", N_train=140, pack="1", clip_qs=False),
    "ch72": _case(CHANNELS, 4, 96, 72, 4, 16, True, "one channel per rank on four ranks", N_train=192, jitter=1e-2, normalize=True, pack="0"),
    "ch72pack": _case(CHANNELS, 4, 96, 72, 4, 16, False, "... packed", N_train=192, jitter=1e-2, normalize=True, pack="1"),
    "ch72L64": _case(CHANNELS, 2, 100, 72, 64, 16, True, "32 channels per rank, largest L", N_train=200, jitter=1e-2, normalize=True),
    "ch130": _case(CHANNELS, 3, 97, 130, 6, 24, False, "pack tile padding (130 = 4 x 32 + 2) and ragged rows", N_train=194, jitter=1e-2,
                   normalize=True, pack="1"),
    "ch260": _case(CHANNELS, 2, 80, 260, 2, 128, True, "largest m below the potrf + potri inverse", N_train=160, jitter=1e-3),
    "ch520": _case(CHANNELS, 2, 64, 520, 2, 128, False, "the default pack rule must be on; ill-conditioned", jitter=1e-3, ill=True),
    # Titsias, row-sharded
    "tit33": _case(TITSIAS, 3, 150, 33, 40, 8, True, "Titsias above the m = 32 instance, three ranks", jitter=1e-4),
    "tit130": _case(TITSIAS, 2, 150, 130, 3, 32, False, "Titsias on the global-memory path", jitter=1e-4),
}
ILL_ALLOWED = ("big520", "ch520", "rows5")


def _entry(b, m, L, M, geco, split=False, one_block=None, pack=None, **kw):
    note = f"DP entry, one rank, split {int(split)} one_block {one_block} pack {pack}"
    return _case(CHANNELS if m > 64 else ROWS, 1, b, m, L, M, geco, note, split=split, one_block=one_block, pack=pack, **kw)


# svgp_mnist_train_step_dp through a 1-rank communicator: (shape, split, one_block / pack).  One problem per shape (ENTRY_SHAPES).
ENTRY_SHAPES = {
    "e_m1": ((60, 1, 4, 3), dict(geco=True)), "e_m7": ((60, 7, 5, 3), dict(geco=False, with_table=False)),
    "e_m31": ((150, 31, 40, 8), dict(geco=True, normalize=True)), "e_L57": ((256, 32, 57, 8), dict(geco=False, seed=713)),
    "e_m33": ((150, 33, 40, 8), dict(geco=True, clip_qs=False)), "e_m64": ((200, 64, 64, 16), dict(geco=False)),
    "e_m72": ((100, 72, 64, 16), dict(geco=True, N_train=200, jitter=1e-2, normalize=True)), "e_m130": ((150, 130, 3, 24), dict(geco=False, N_train=300, jitter=1e-2, normalize=True)),
    "e_m260": ((80, 260, 2, 128), dict(geco=True, N_train=160, jitter=1e-3, normalize=True)),
}
ENTRY_ONE_BLOCK = ("e_m31", "e_L57")         # the m <= 64 shapes that also run with cfg.single_stat_block
ENTRY_CASES = {}
for _name, (_shape, _kw) in ENTRY_SHAPES.items():
    if _shape[1] > 64:                       # the wire-buffer workspace, blocks as they are / tile-packed
        for _pack in ("0", "1"):
            ENTRY_CASES[f"{_name}-pack{_pack}"] = _entry(*_shape, one_block=True, pack=_pack, **_kw)
    else:
        for _split in (False, True):
            for _one in (False, True) if _name in ENTRY_ONE_BLOCK else (False,):
                ENTRY_CASES[f"{_name}-split{int(_split)}-one{int(_one)}"] = _entry(*_shape, split=_split, one_block=_one, **_kw)
ALL = {**CASES, **ENTRY_CASES}


def seed_of(case):
    if ALL[case]["seed"] is not None:        # a problem whose first seed failed the guard's (a) or (b)
        return ALL[case]["seed"]
    if case in CASES:
        return 500 + list(CASES).index(case)
    return 600 + list(ENTRY_SHAPES).index(case.split("-")[0])


def shards(case):
    from svgp_vae_amd.engine import shard_rows
    cs = ALL[case]
    return [shard_rows(cs["b"], cs["G"], r) for r in range(cs["G"])]


def _pkey(case):
    cs = ALL[case]
    return (seed_of(case),) + tuple(cs[k] for k in ("b", "m", "L", "M", "jitter", "geco", "normalize", "with_table", "clip_qs",
                                                    "titsias", "N_train"))


@functools.lru_cache(maxsize=None)
def _problem(key):
    seed, b, m, L, M = key[:5]
    return H.toy_problem(b=b, m=m, L=L, M=M, n_obj=60, seed=seed, with_table=key[8])


def problem(case):
    """(params, images, aux, eps) of a case at its global batch; shared: callers must not write to it."""
    return _problem(_pkey(case))


def bars(case):
    return dict(scalar=TC.SCALAR_TOL, field=TC.FIELD_TOL, grad=TC.GRAD_TOL) if ALL[case]["titsias"] else \
        dict(scalar=H.SCALAR_TOL, field=H.FWD_TOL, grad=H.GRAD_TOL)


def bar(case, name):
    return bars(case)[name.split()[0]]


def _ulp_inputs(params, images):
    """The perturbation of helpers._compare_step: every parameter and the images times 1 +- 2^-52, signs from a fixed generator,
    the inducing points' id column kept."""
    gen = torch.Generator().manual_seed(17)
    ulp = lambda t: t * (1.0 + 2.0 ** -52 * (torch.randint(0, 2, t.shape, generator=gen).to(DT) * 2 - 1))
    p2 = {k: ulp(v) for k, v in params.items()}
    p2["inducing_index_points"][:, 0] = params["inducing_index_points"][:, 0]
    return p2, ulp(images)


def _oracle_kw(cs):
    return dict(beta=BETA, C_ma=torch.tensor(C_MA, dtype=DT), lagrange_mult=torch.tensor(LAGRANGE, dtype=DT), alpha=ALPHA,
                kappa=math.sqrt(KAPPA2), clipping_qs=cs["clip_qs"], GECO=cs["geco"], jitter=cs["jitter"], N_train=cs["N_train"], L=cs["L"],
                K_obj_normalize=cs["normalize"])


def _quantities(cs, out, grads, fields):
    q = {"scalar " + key: out[idx].detach().reshape(()) for key, idx in SCALARS + (GECO_SCALARS if cs["geco"] else ())}
    q.update({"field " + k: v.detach() for k, v in fields.items()})
    q.update({"grad " + k: v.detach() for k, v in grads.items()})
    return q


def _evaluate(case, params, images, aux, eps):
    """name -> tensor of every quantity the GPU comparison reads, from the oracle on the global batch: `scalar *` and `grad *` from
    svgpvae_oracle.loss_and_grads (Hensman: the efficient formulation, as helpers._compare_step; Titsias: the literal b x b one, as
    tests/titsias_cases.py), `field *` from helpers.oracle_stages (Titsias: from the oracle's 16-tuple)."""
    cs = ALL[case]
    b = cs["b"]
    if cs["titsias"]:
        out, grads = O.loss_and_grads(params, images, aux, eps, titsias=True, formulation="literal", **_oracle_kw(cs))
        fields = dict(qnet_mu=out[7], qnet_var=out[8], p_m=out[5], p_v=out[6], z=out[12], recon=out[9].reshape(b, 784))
        return _quantities(cs, out, grads, fields)
    out, grads = O.loss_and_grads(params, images, aux, eps, formulation="efficient", **_oracle_kw(cs))
    st = H.oracle_stages(params, images, aux, eps, N_train=cs["N_train"], jitter=cs["jitter"], clip_qs=cs["clip_qs"], geco=cs["geco"],
                         beta=BETA, K_obj_normalize=cs["normalize"], b_global=b)
    fields = {k: st[k].reshape(shp) for k, shp in H.FIELD_SHAPES(b, cs["m"], cs["L"]).items()}
    if cs["m"] > 64:                         # the large-m path does not form M2: its rows W = Kn Ki K are compared instead
        del fields["M2"]
        fields["W"] = st["Kn"] @ st["Ki"] @ st["K"]
    return _quantities(cs, out, grads, fields)


@functools.lru_cache(maxsize=None)
def _reference(key, case):
    return _evaluate(case, *_problem(key))


def reference(case):
    """The oracle's quantities on the global batch; computed once per problem and shared: callers must not write to it."""
    return _reference(_pkey(case), case if ALL[case]["titsias"] else _canonical(case))


def _canonical(case):
    """Cases that share a problem (the DP-entry variants of one shape) share one reference."""
    key = _pkey(case)
    return next(c for c in ALL if _pkey(c) == key)


def errors(got, want, rows=None, window=None):
    """name -> error of `got` against `want` in the measure of its bar, for every quantity `got` holds: scalars |got - want| /
    max(1, |want|), fields and gradients max-abs difference over the reference's max-abs.  rows = (lo, hi): row fields of `got`
    are the rank's rows; window = (l0, nl): WINDOW_FIELDS of `got` are the rank's channels."""
    e = {}
    for k, g in got.items():
        w = want[k]
        kind, name = k.split()
        if kind == "scalar":
            e[k] = abs(float(g) - float(w)) / max(1.0, abs(float(w)))
            continue
        if kind == "field" and rows is not None and name in ROW_FIELDS:
            w = w[rows[0]:rows[1]]
        if kind == "field" and window is not None and name in WINDOW_FIELDS:
            w = w[window[0]:window[0] + window[1]]
        assert tuple(g.shape) == tuple(w.shape), (k, g.shape, w.shape)
        e[k] = H.relerr(g, w)
    return e


def worst(errs):
    """{group: largest error} over scalars, fields and gradients."""
    return {g: max(v for k, v in errs.items() if k.startswith(g)) for g in ("scalar", "field", "grad")}


@functools.lru_cache(maxsize=None)
def _response(key, case):
    params, images, aux, eps = _problem(key)
    p2, img2 = _ulp_inputs(params, images)
    return errors(_evaluate(case, p2, img2, aux, eps), _reference(key, case))


def oracle_response(case):
    """The oracle evaluated again with its real inputs perturbed by one ulp: its change per quantity, as `errors` measures it."""
    return _response(_pkey(case), case if ALL[case]["titsias"] else _canonical(case))


def tolerances(case):
    """name -> bound of the GPU comparison: the fixed bar; for the cases marked ill max(bar, 20 x the oracle's own one-ulp
    response) per quantity."""
    ref = reference(case)
    if ALL[case]["ill"]:
        return {k: max(bar(case, k), 20 * v) for k, v in oracle_response(case).items()}
    return {k: bar(case, k) for k in ref}


# ---------------------------------------------------------------- the rank-sum restatement
def _restate(case, params, images, aux, eps, parts):
    """One step evaluated with the oracle's stage formulas (oracle/staged_gp.py, the pieces helpers.oracle_stages is made of) from
    statistics that are formed per shard of `parts` and added in rank order -- the only arithmetic that row sharding changes --,
    every later stage taken from the sum; gradients by autograd.  Same quantities as `_evaluate`."""
    cs = ALL[case]
    b, L, m, jitter = cs["b"], cs["L"], cs["m"], cs["jitter"]
    c = cs["N_train"] / float(b)
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    vae = O.MnistVAE(leaf, L)
    mu, var_raw = vae.encode(images)
    var = O.clip_by_value(var_raw, 1e-3, 10.0) if cs["clip_qs"] else var_raw
    K, Kn, knn = SG.kernel_matrix_fwd(aux, leaf["inducing_index_points"], leaf.get("object_vectors"), leaf["l_GP"],
                                      leaf["amplitude"], cs["normalize"])
    p = O.reciprocal_no_nan(var)

    def rank_sum(stat):
        tot = None
        for lo, hi in parts:
            part = stat(lo, hi)
            tot = part if tot is None else tuple(t + x for t, x in zip(tot, part))
        return tot

    S, v = rank_sum(lambda lo, hi: SG.gp_stats(Kn[lo:hi], p[lo:hi], (p * mu)[lo:hi])[:2])
    f = SG.gp_factor_fwd(K, S, v, jitter, c)
    ps = SG.gp_posterior_fwd(Kn, knn, mu, var, eps, f, c)
    if cs["titsias"]:
        S2, v2 = rank_sum(lambda lo, hi: SG.titsias_stats(Kn[lo:hi], mu[lo:hi], var[lo:hi], jitter))
        _, ld2, _, vt, rows = SG.titsias_fwd(K, S2, v2, mu, var, knn, ps["q"], jitter)
        inside_recon = -0.5 * (b * L * O.LOG_2PI + rows + ld2.sum() - L * f["ldK"] - vt.sum())
        inside_kl = torch.zeros((), dtype=DT)
        inside_elbo = inside_recon - inside_kl
    else:
        inside_recon, inside_kl = ps["L3"].sum(), f["KL"].sum()
        inside_elbo = inside_recon - (b / cs["N_train"]) * inside_kl
    ce_term = O.gauss_cross_entropy(ps["p_m"], ps["p_v"], mu, var).sum()
    kl_term = -ce_term + inside_elbo
    recon = vae.decode(ps["z"])
    C_ma, lagrange = torch.tensor(C_MA, dtype=DT), torch.tensor(LAGRANGE, dtype=DT)
    if cs["geco"]:                           # svgpvae_oracle.forward_pass_SVGPVAE, the GECO branch
        recon_loss = torch.sum(torch.mean((images - recon) ** 2, dim=(1, 2, 3)) - KAPPA2)
        C_ma = ALPHA * C_ma + (1 - ALPHA) * recon_loss / b
        elbo = -kl_term + lagrange * (recon_loss / b + (C_ma - recon_loss / b).detach())
        lagrange = lagrange * torch.exp(C_ma)
    else:
        recon_loss = torch.sum((images - recon) ** 2) / 784.0
        elbo = -recon_loss + (BETA / float(L)) * kl_term
    names = list(leaf)
    gs = torch.autograd.grad(elbo if cs["geco"] else -elbo, [leaf[k] for k in names], allow_unused=True)
    grads = {k: (torch.zeros_like(leaf[k]) if g is None else g) for k, g in zip(names, gs)}
    out = {0: elbo, 1: recon_loss, 2: kl_term, 3: inside_elbo, 4: ce_term, 10: inside_recon, 11: inside_kl, 13: C_ma, 14: lagrange}
    if cs["titsias"]:
        fields = dict(qnet_mu=mu, qnet_var=var, p_m=ps["p_m"], p_v=ps["p_v"], z=ps["z"], recon=recon.reshape(b, 784))
    else:
        fields = dict(qnet_mu=mu, qnet_var_raw=var_raw, qnet_var=var, K=K, Kn=Kn, knn=knn, S=S, v=v, Ki=f["Ki"],
                      ldK=f["ldK"].reshape(1), Si=f["Si"], t=f["t"], G=f["G"], A=f["A"], Aji=f["Aji"], mu_hat=f["mu"], u=f["u"],
                      KL=f["KL"], q=ps["q"], p_m=ps["p_m"], p_v=ps["p_v"], e=ps["e"], d=ps["d"], z=ps["z"], recon=recon.reshape(b, 784))
        if m > 64:
            fields["W"] = Kn @ f["Ki"] @ K
        else:
            fields["M2"] = f["Ki"][None] @ f["A"] @ f["Ki"][None]
    return _quantities(cs, out, grads, fields)


@functools.lru_cache(maxsize=None)
def restatement_gap(case):
    """The rank-sum restatement against the oracle on the whole batch, per quantity."""
    return errors(_restate(case, *problem(case), shards(case)), reference(case))


# ---------------------------------------------------------------- the engines
@contextlib.contextmanager
def pack_env(pack):
    """SVGP_DP_PACK for the duration of a comparison: "0" / "1", or None = unset (the library's rule: on from m = 512)."""
    old = os.environ.get("SVGP_DP_PACK")
    if pack is None:
        os.environ.pop("SVGP_DP_PACK", None)
    else:
        os.environ["SVGP_DP_PACK"] = pack
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SVGP_DP_PACK", None)
        else:
            os.environ["SVGP_DP_PACK"] = old


def engine(case, rank=0):
    """Rank `rank`'s MnistStepEngine of a case, capacity cs["b_max"] rows, the problem's parameters loaded, the GECO state set."""
    cs = ALL[case]
    kw = dict(geco=cs["geco"], clip_qs=cs["clip_qs"], N_train=cs["N_train"], jitter=cs["jitter"], beta=BETA, K_obj_normalize=cs["normalize"],
              kappa_squared=KAPPA2, titsias=cs["titsias"], split_grad_exchange=cs["split_grad_exchange"],
              single_stat_block=cs["single_stat_block"])
    eng = H.engine_for(problem(case)[0], cs["b_max"], rank=rank, world_size=cs["G"], **kw)
    eng.set_scalars(c_ma=C_MA, lagrange=LAGRANGE, alpha=ALPHA)
    return eng


def bind_rows(case, eng, lo, hi):
    _, images, aux, eps = problem(case)
    dev = eng.device
    eng.set_batch_size(hi - lo, ALL[case]["b"])
    eng.bind(images[lo:hi].contiguous().to(dev), aux[lo:hi].contiguous().to(dev), eps[lo:hi].contiguous().to(dev))


def lockstep(engines, phases, adam=False):
    """The row-sharded schedule with virtual ranks: every engine runs a phase, then the phase's exchange block is summed across
    the engines in rank order and written back to each -- what the all-reduce does between real ranks."""
    for k, name in phases:
        for e in engines:
            e.phase(k, adam)
        if name:
            for e in engines:
                e.synchronize()
            tot = sum(e.block(name) for e in engines)
            for e in engines:
                with torch.cuda.stream(e.stream):
                    e.block(name).copy_(tot)
                e.synchronize()
    for e in engines:
        e.synchronize()


def sharded_step(engines, packed, adam=False):
    """The channel-sharded schedule with virtual ranks: sharded_stages of every engine in lockstep, each exchange point through
    engine.virtual_exchange.  Five points; with the packed exchange points 1-4 carry the symmetric mark on their (L, m, m) member."""
    from svgp_vae_amd.engine import virtual_exchange
    gens = [e.sharded_stages(adam=adam) for e in engines]
    n_points = 0
    while True:
        ops = [next(g, None) for g in gens]
        if ops[0] is None:
            assert all(o is None for o in ops)
            break
        for e in engines:
            e.synchronize()
        assert all(len(o) == len(ops[0]) for o in ops)
        if n_points < 4:
            assert (ops[0][0].sym is not None) == packed, n_points
        virtual_exchange(ops)
        torch.cuda.synchronize()
        n_points += 1
    assert n_points == 5
    for e in engines:
        e.synchronize()


def rank_quantities(case, eng, window=None):
    """name -> CPU tensor of what rank `eng` holds after its step: scalars, reduced gradients, and the fields complete on it (the
    module docstring has the list); window = (l0, nl) on the channel-sharded route."""
    cs = ALL[case]
    b, m, L = eng.cfg.b, cs["m"], cs["L"]
    sc = eng.scalars()                        # raises SvgpError if a hand-off of the step timed out
    got = {"scalar " + key: torch.tensor(sc[key], dtype=DT) for key, _ in SCALARS + (GECO_SCALARS if cs["geco"] else ())}
    got.update({"grad " + k: v.cpu().clone() for k, v in eng.grads().items()})
    shapes = H.FIELD_SHAPES(b, m, L)
    names = TITSIAS_FIELDS if cs["titsias"] else [n for n in shapes if not (n == "M2" and m > 64)]
    for name in names:
        t = eng.ws_view(name, shapes[name]).cpu().clone()
        if window is not None and name in WINDOW_FIELDS:
            t = t[window[0]:window[0] + window[1]]
        got["field " + name] = t
    if m > 64 and not cs["titsias"]:
        got["field W"] = eng.ws[eng.wl.Kn + b * m:eng.wl.Kn + 2 * b * m].view(b, m).cpu().clone()
    return got


def assert_handoffs_clean(eng):
    fl = eng.ws_view("flags", (64,)).view(torch.int64)
    assert torch.count_nonzero(fl) == 0, fl.tolist()
    eng.scalars()                             # raises SvgpError("... hand-off ...") if a consumer gave up waiting


def judge(case, label, got, rows=None, window=None):
    """Prints every figure of `got` against the reference and returns the list of those past their bound."""
    tol, bad = tolerances(case), []
    for k, g in got.items():
        if not bool(torch.isfinite(g).all()):
            bad.append(f"{label} {k} is not finite")
    errs = errors(got, reference(case), rows, window)
    for k, e in errs.items():
        print(f"{label} {k}: {e:.2e} (bound {tol[k]:.1e})")
        if not e <= tol[k]:
            bad.append(f"{label} {k}: {e:.3e} > {tol[k]:.1e}")
    w = worst(errs)
    print(f"{label} WORST scalars {w['scalar']:.2e} fields {w['field']:.2e} gradients {w['grad']:.2e}")
    return bad


def compare_ranks(case):
    """ONE step without the optimiser of the case's G virtual ranks; every rank against the oracle on the global batch.  Returns the
    list of failures."""
    from svgp_vae_amd.engine import dp_pack_enabled
    cs = ALL[case]
    G, m = cs["G"], cs["m"]
    with pack_env(cs["pack"]):
        engines = []
        for r, (lo, hi) in enumerate(shards(case)):
            e = engine(case, r)
            bind_rows(case, e, lo, hi)
            assert e.channel_sharded() == (cs["route"] == CHANNELS)
            assert e.cfg.split_grad_exchange == int(cs["split_grad_exchange"])
            if cs["single_stat_block"] is not None:
                assert e.cfg.single_stat_block == int(cs["single_stat_block"])
            engines.append(e)
        if cs["route"] == CHANNELS:
            packed = dp_pack_enabled(m)
            assert packed == (cs["pack"] == "1" or (cs["pack"] is None and m >= 512))
            sharded_step(engines, packed)
        else:
            lockstep(engines, SPLIT_PHASES if cs["split_grad_exchange"] else PLAIN_PHASES)
    bad = []
    g0 = engines[0].grads()
    for r, ((lo, hi), e) in enumerate(zip(shards(case), engines)):
        window = (r * (cs["L"] // G), cs["L"] // G) if cs["route"] == CHANNELS else None
        bad += judge(case, f"{case} rank {r}", rank_quantities(case, e, window), (lo, hi), window)
        if e.wl.stat_parts != expected_stat_parts(case):
            bad.append(f"{case} rank {r}: {e.wl.stat_parts} statistics partials, expected {expected_stat_parts(case)}")
        for k, g in e.grads().items():        # replicas: same reduced inputs, same kernels
            if not torch.equal(g, g0[k]):
                bad.append(f"{case} rank {r} grad {k} is not bit-equal to rank 0's")
        assert_handoffs_clean(e)
    return bad


def expected_stat_parts(case):
    """Row partials of the statistics blocks: 4 where the per-rank capacity is at least 128, m <= 64 and the blocks are not asked
    to be single (cfg.single_stat_block), else 1."""
    cs = ALL[case]
    return 4 if cs["b_max"] >= 128 and cs["m"] <= 64 and not cs["single_stat_block"] else 1


def compare_entry(case, eng):
    """ONE step without the optimiser of `eng` (its communicator attached) on the case's whole batch against the oracle."""
    cs = ALL[case]
    with pack_env(cs["pack"]):
        bind_rows(case, eng, 0, cs["b"])
        eng.run(adam=False)
        eng.synchronize()
    window = (0, cs["L"]) if cs["route"] == CHANNELS else None
    bad = judge(case, case, rank_quantities(case, eng, window), (0, cs["b"]), window)
    assert_handoffs_clean(eng)
    return bad


def route_text(case, rank, forms=False):
    """The launch plan of STEP_FORM_DP for rank `rank` of the case (svgp_mnist_step_route[_forms]; no device needed)."""
    import ctypes as C
    from svgp_vae_amd import _lib
    cs = ALL[case]
    lo, hi = shards(case)[rank]
    one = cs["single_stat_block"]
    cfg = _lib.MnistCfg(b=hi - lo, b_global=cs["b"], b_cap=cs["b_max"], m=cs["m"], L=cs["L"], M=cs["M"],
                        n_obj=60 if cs["with_table"] else 0, normalize_obj=int(cs["normalize"]), clip_qs=int(cs["clip_qs"]),
                        geco=int(cs["geco"]), titsias=int(cs["titsias"]), train_ip=1, train_gp=1, train_ov=1,
                        single_stat_block=int((cs["G"] > 1 and cs["m"] > 64) if one is None else one),
                        split_grad_exchange=int(cs["split_grad_exchange"]), N_train=cs["N_train"], jitter=cs["jitter"],
                        kappa_squared=KAPPA2, alpha=ALPHA, rep_weight=1.0 if rank == 0 else 0.0)
    buf = C.create_string_buffer(8192)
    with pack_env(cs["pack"]):
        _lib.call("svgp_mnist_step_route_forms" if forms else "svgp_mnist_step_route", C.byref(cfg), 2, 0, cs["G"], rank, 0, 0, buf,
                  8192)
    return buf.value.decode()
