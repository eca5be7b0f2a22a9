"""The Titsias form of the MNIST step (cfg.titsias, csrc/gp_titsias.hip): shape-envelope case table, problems, the literal oracle,
the m x m restatement, the oracle's own one-ulp response, engine builder and comparison, shared by
tests/test_gpu_titsias_envelope.py, tests/test_gpu_titsias_stages.py (GPU) and tests/test_titsias_envelope_oracle_cpu.py (guard).

The bars are those of tests/test_gpu_titsias.py (float64 end to end): scalars 1e-8 relative to max(1, |want|), p_m / p_v / z /
recon 1e-8 of the tensor's max-abs, gradients 1e-6 of the tensor's max-abs."""
import functools
import math

import torch

from oracle import svgpvae_oracle as O
from tests import helpers as H

DT = torch.float64
SCALAR_TOL, FIELD_TOL, GRAD_TOL = 1e-8, 1e-8, 1e-6
N_TRAIN, C_MA, LAGRANGE, ALPHA, BETA, KAPPA2 = 4050.0, 0.02, 1.3, 0.9, 0.001, 0.02
SCALARS = (("elbo", 0), ("recon_loss", 1), ("kl_term", 2), ("inside_elbo", 3), ("ce_term", 4), ("inside_recon", 10),
           ("inside_kl", 11))
GECO_SCALARS = (("c_ma", 13), ("lagrange", 14))
FIELDS = (("p_m", 5), ("p_v", 6), ("z", 12), ("recon", 9))


def _case(b, m, L, M, jitter, geco, **kw):
    return dict(b=b, m=m, L=L, M=M, jitter=jitter, geco=geco, normalize=kw.pop("normalize", False),
                with_table=kw.pop("with_table", True), clip_qs=kw.pop("clip_qs", True), ill=kw.pop("ill", False), **kw)


# name: (b, m, L, M, jitter, GECO).  The problem is helpers.toy_problem(n_obj=60, seed=300 + the row's index).
CASES = {
    "L1": _case(60, 16, 1, 4, 1e-4, True),                            # (L - 1) m < 2 L: the reverse stage's W | cA | cB past L b m
    "m1": _case(60, 1, 4, 3, 1e-4, False, clip_qs=False),             # ... at one inducing point
    "m2": _case(60, 2, 3, 3, 1e-4, True, with_table=False),           # ... at two
    "m3L2": _case(60, 3, 2, 3, 1e-4, False, normalize=True),          # ... 6 + 4 > 6
    "m3L3": _case(60, 3, 3, 3, 1e-4, True),                           # first shape with L b m == b m + 2 b L
    "b128": _case(128, 32, 16, 8, 1e-4, False),                       # first capacity with four statistics partials, config-2 shape
    "b257": _case(257, 16, 16, 4, 1e-4, True, normalize=True),        # one row past the weight-gradient partial slots
    "j1e-6": _case(256, 32, 16, 8, 1e-6, False, with_table=False),    # the drivers' jitter
    "m33": _case(150, 33, 40, 8, 1e-4, True),                         # above the m = 32 kernel instance
    "m31": _case(150, 31, 40, 8, 1e-4, False, clip_qs=False),         # below it
    "m64L64": _case(200, 64, 64, 16, 1e-4, True),                     # LDS limit, largest L
    "m65": _case(70, 65, 5, 16, 1e-4, False, normalize=True),         # first global-memory m
    "m72L64": _case(100, 72, 64, 16, 1e-4, True),                     # global-memory path at the largest L
    "m72L22": _case(100, 72, 22, 16, 1e-4, False, with_table=False),  # decoder reverse pass in two launches
    "m130": _case(150, 130, 3, 32, 1e-4, True, clip_qs=False),        # no multiple of the 64-wide tiles
    # (m260 under the beta-ELBO objective: the literal oracle's one-ulp response of the inducing points' gradient is 1.004e-8, a
    # hair past bar / 100; under GECO, as the table was measured when it was drawn up, 1.5e-9 -- so GECO it is)
    "m260": _case(80, 260, 2, 128, 1e-3, True),                       # largest m below the potrf + potri inverse
    "m520": _case(64, 520, 2, 128, 1e-3, False, ill=True),            # potrf + potri inverse; ill-conditioned (see tolerances)
    # problems of the capacity tests
    "b127": _case(127, 32, 16, 8, 1e-4, True),                        # last capacity with one statistics partial
    "cap256": _case(256, 32, 16, 8, 1e-4, True),                      # stepped with its first CAPACITY_BATCHES rows
}
ENVELOPE_CASES = [c for c in CASES if c not in ("b127", "cap256")]
# (3 rows again after the full batch: partials that held rows must read as empty)
CAPACITY_CASE, CAPACITY_BATCHES = "cap256", (1, 3, 127, 255, 256, 3)
# 1 or 3 rows against 32 inducing points: held to 20x the oracle's own one-ulp response, as the Hensman suite holds them
# (tests/test_gpu_shape_envelope.py); every other batch takes the fixed bars
SELF_CONSISTENCY_ROWS = (1, 3)
STAGE_CASES = ("m3L3", "b128", "m64L64", "m72L22", "m130")
GRAPH_CASES = ("m64L64", "m72L22")


def expected_stat_parts(cs, b_max=None):
    """Row partials of the statistics blocks: 4 where the capacity is at least 128 and m <= 64, else 1."""
    return 4 if (cs["b"] if b_max is None else b_max) >= 128 and cs["m"] <= 64 else 1


@functools.lru_cache(maxsize=None)
def problem(case):
    """(params, images, aux, eps) of a case at its full batch; shared: callers must not write to it."""
    cs = CASES[case]
    return H.toy_problem(b=cs["b"], m=cs["m"], L=cs["L"], M=cs["M"], n_obj=60, seed=300 + list(CASES).index(case),
                         with_table=cs["with_table"])


def rows_of(case, rows=None):
    params, images, aux, eps = problem(case)
    b = CASES[case]["b"] if rows is None else rows
    return params, images[:b].contiguous(), aux[:b].contiguous(), eps[:b].contiguous()


def oracle(case, params, images, aux, eps, formulation="literal"):
    """(16-tuple, gradients) of the float64 oracle's Titsias step: the literal b x b branch, or ("mspace") the restatement."""
    cs = CASES[case]
    return O.loss_and_grads(params, images, aux, eps, beta=BETA, C_ma=torch.tensor(C_MA, dtype=DT),
                            lagrange_mult=torch.tensor(LAGRANGE, dtype=DT), alpha=ALPHA, kappa=math.sqrt(KAPPA2),
                            clipping_qs=cs["clip_qs"], GECO=cs["geco"], jitter=cs["jitter"], N_train=N_TRAIN, L=cs["L"],
                            K_obj_normalize=cs["normalize"], titsias=True, formulation=formulation)


@functools.lru_cache(maxsize=None)
def reference(case, rows=None):
    """The literal oracle's (16-tuple, gradients) for the first `rows` rows (default: all) of a case's problem; computed once
    per process and shared: callers must not write to it."""
    return oracle(case, *rows_of(case, rows))


def errors(case, out, grads, want, wgrads):
    """name -> error of (out, grads) against (want, wgrads) in the measure of its bar, for every quantity the GPU test compares:
    scalars |got - want| / max(1, |want|), fields and gradients max-abs difference over the reference's max-abs."""
    e = {}
    for key, idx in SCALARS + (GECO_SCALARS if CASES[case]["geco"] else ()):
        e["scalar " + key] = abs(float(out[idx]) - float(want[idx])) / max(1.0, abs(float(want[idx])))
    for key, idx in FIELDS:
        e["field " + key] = H.relerr(out[idx], want[idx])
    for k, w in wgrads.items():
        e["grad " + k] = H.relerr(grads[k], w)
    return e


def bar(name):
    return {"scalar": SCALAR_TOL, "field": FIELD_TOL, "grad": GRAD_TOL}[name.split()[0]]


def worst(errs):
    """{group: largest error} over scalars, fields and gradients."""
    return {g: max(v for k, v in errs.items() if k.startswith(g)) for g in ("scalar", "field", "grad")}


@functools.lru_cache(maxsize=None)
def oracle_response(case, rows=None):
    """The literal oracle evaluated again with its real inputs perturbed by one ulp (the perturbation of helpers._compare_step:
    every parameter and the images times 1 +- 2^-52, signs from a fixed generator, the inducing points' id column kept): its
    change per quantity, as `errors` measures it."""
    params, images, aux, eps = rows_of(case, rows)
    gen = torch.Generator().manual_seed(17)
    ulp = lambda t: t * (1.0 + 2.0 ** -52 * (torch.randint(0, 2, t.shape, generator=gen).to(DT) * 2 - 1))
    p2 = {k: ulp(v) for k, v in params.items()}
    p2["inducing_index_points"][:, 0] = params["inducing_index_points"][:, 0]
    out2, g2 = oracle(case, p2, ulp(images), aux, eps)
    return errors(case, out2, g2, *reference(case, rows))


@functools.lru_cache(maxsize=None)
def restatement_gap(case, rows=None):
    """The m x m restatement (oracle/staged_gp.py) against the literal oracle, per quantity."""
    return errors(case, *oracle(case, *rows_of(case, rows), formulation="mspace"), *reference(case, rows))


def tolerances(case, rows=None):
    """name -> bound of the GPU comparison: the fixed bar; for the one case marked ill and for the 1- and 3-row batches
    max(bar, 20 x the oracle's own one-ulp response) (the self_consistency rule of helpers._compare_step)."""
    resp = oracle_response(case, rows)
    if CASES[case]["ill"] or (rows is not None and rows in SELF_CONSISTENCY_ROWS):
        return {k: max(bar(k), 20 * v) for k, v in resp.items()}
    return {k: bar(k) for k in resp}


def engine(case, b_max=None, **kw):
    """A MnistStepEngine with cfg.titsias for a case, its problem's parameters loaded."""
    cs = CASES[case]
    return H.engine_for(problem(case)[0], cs["b"] if b_max is None else b_max, geco=cs["geco"], clip_qs=cs["clip_qs"],
                        N_train=N_TRAIN, jitter=cs["jitter"], beta=BETA, K_obj_normalize=cs["normalize"], kappa_squared=KAPPA2,
                        titsias=True, **kw)


def step(eng, images, aux, eps):
    """One step without the optimiser from the common scalars; returns (16-tuple slots the tests compare, gradients) on the CPU."""
    b, L = eps.shape
    if eng.cfg.b != b:
        eng.set_batch_size(b)
    eng.set_scalars(c_ma=C_MA, lagrange=LAGRANGE, alpha=ALPHA)
    H._run_once(eng, images, aux, eps)
    sc = eng.scalars()                 # raises SvgpError if a hand-off of the step timed out
    out = {idx: sc[key] for key, idx in SCALARS + GECO_SCALARS}
    for (key, idx), shp in zip(FIELDS, ((b, L), (b, L), (b, L), (b, 28, 28, 1))):
        out[idx] = eng.ws_view(key, (b, 784) if key == "recon" else shp).cpu().reshape(shp)
    return out, {k: v.cpu() for k, v in eng.grads().items()}


def compare(case, eng, rows=None, label=None):
    """One step of `eng` on the first `rows` rows of the case's problem against the literal oracle.  Prints every figure;
    returns (failures, {group: largest error})."""
    params, images, aux, eps = rows_of(case, rows)
    want, wgrads = reference(case, rows)
    out, grads = step(eng, images, aux, eps)
    tol, bad = tolerances(case, rows), []
    label = label or (case if rows is None else f"{case} rows {rows}")
    for k, g in grads.items():
        if not bool(torch.isfinite(g).all()):
            bad.append(f"{label} grad {k} is not finite")
    errs = errors(case, out, grads, want, wgrads)
    for k, e in errs.items():
        print(f"{label} {k}: {e:.2e} (bound {tol[k]:.1e})")
        if not e <= tol[k]:
            bad.append(f"{label} {k}: {e:.3e} > {tol[k]:.1e}")
    w = worst(errs)
    print(f"{label} WORST scalars {w['scalar']:.2e} fields {w['field']:.2e} gradients {w['grad']:.2e}")
    return bad, w
