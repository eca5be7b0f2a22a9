"""The Casale GP-VAE over the shape range check_cfg (csrc/casale.hip) accepts -- 1 <= Q <= 32, 1 <= M <= 128, H = M Q <= 2048,
1 <= L <= 64, any N, any batch range inside b_cap <= N -- at the shapes where the code changes form, against the float64 CPU
restatement (tests/casale_cases.py).  ENVELOPE_CASES says per entry which path it is there for; tests/test_casale_cpu.py holds
the guard that the oracle's own response to a one-ulp input change is at least 100 times below every bar used here.

1. the GP stage (`_GpStage.fwd` + `.bwd`) over the table, three batch ranges in a row on one NaN-filled workspace with a canary
   tail: the whole set, the last row alone (leftovers of the larger batch in VPb / zbbar must not leak), a ragged middle range;
2. the whole step past the 256 weight-gradient partial slots (N = 277 train rows, batch 256 + ragged tail) and at L = 64 / L = 1;
3. the row-wise kernels through the C ABI: both samples and their seed with variances exactly at the clip bounds, the plain-VAE
   glue and the closing scalars at b L = 1 / 255 / 257, the prediction variance at N, H around 64.

Bars as in tests/test_gpu_casale.py (tests/helpers.relerr, relative to the tensor's max-abs): scalars 1e-9, row and matrix
quantities 1e-8, gradients 1e-7; the element-wise kernels of part 3 are held to 1e-13 / 1e-12."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import casale_cases as CC
from tests.helpers import relerr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mnist_cfg2_inputs.npz")
FWD_NAMES = ("K_W", "L_W", "V", "G", "P", "U", "A")
CANARY, TAIL = -1.2345e300, 4096
_REF = {}


def _ref(key, fn):
    """References and cases are computed once and shared; nobody writes to them."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _case(name, normalize):
    return _ref(("case", name, normalize), lambda: CC.make_envelope_case(name, normalize))


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---------------------------------------------------------------------------------------------------------- 1. GP stage
def _poisoned_stage(case, train_gp=1, train_ov=1):
    """The stage of a case with b_cap = N on a workspace of NaNs followed by a canary tail."""
    from svgp_vae_amd.GPVAE_Casale_model import _GpStage, _row_index
    dev = torch.device("cuda:0")
    GP = CC.gp_object(case, ov_joint=True)
    angles, obj, ang = _row_index(case["aux"][:, 1:])
    st = _GpStage(GP, case["N"], angles, obj, ang, b_cap=case["N"], L=case["L"], device=dev, train_gp=train_gp, train_ov=train_ov)
    assert (st.Q, st.M, st.H) == (case["Q"], case["M"], case["H"])
    total = st.wl.total
    big = torch.full((total + TAIL,), float("nan"), dtype=torch.float64, device=dev)
    big[total:] = CANARY
    st.ws = big[:total]
    return st, big, GP._gp_vector(dev)


def _run(st, gp, case, batch, seed=1.0):
    """fwd + bwd of one batch range; every compared quantity as a CPU copy."""
    lo, hi = batch
    dev, b = st.dev, hi - lo
    Z, zb = CC.t64(case["Z"]).to(dev).contiguous(), CC.t64(case["zb"][batch]).to(dev).contiguous()
    s = _stream(dev)
    st.fwd(gp, Z.data_ptr(), zb.data_ptr(), lo, hi, s)
    st.bwd(gp, Z.data_ptr(), zb.data_ptr(), lo, hi, seed, s)
    torch.cuda.current_stream(dev).synchronize()
    out = {k: st.named(k, b).cpu().clone() for k in FWD_NAMES + ("Zbar", "zbbar", "terms")}
    g = st.ws[st.wl.grad_gp:st.wl.grad_gp + 3 + case["n_obj"] * case["M"]].cpu().clone()
    out.update(l_GP=g[0], amplitude=g[1], alpha=g[2], object_vectors=g[3:].view(case["n_obj"], case["M"]))
    return out


def _tail_intact(st, big):
    tail = big[st.wl.total:]
    return tail.numel() == TAIL and bool((tail == CANARY).all())


@pytest.mark.parametrize("name,normalize", CC.envelope_variants(), ids=lambda v: {False: "raw", True: "norm"}.get(v, v))
def test_gp_stage_over_the_envelope(name, normalize):
    case = _case(name, normalize)
    st, big, gp = _poisoned_stage(case)
    worst = {}
    for batch in case["batches"]:          # (0, N), then (N - 1, N) on the leftovers of the larger batch, then the middle
        ref = _ref(("gp", name, normalize, batch), lambda: CC.gp_stage_reference(case, batch))
        got = _run(st, gp, case, batch)
        assert _tail_intact(st, big), (name, batch)
        bad = []
        for k in FWD_NAMES:
            e = relerr(got[k], ref[k])
            worst[CC.FWD_TOL] = max(worst.get(CC.FWD_TOL, 0.0), e)
            if not e < CC.FWD_TOL:
                bad.append((k, e))
        e = relerr(got["terms"][:3], ref["terms"])
        e7 = abs(float(got["terms"][7]) - float(ref["GP_prior_term"])) / abs(float(ref["GP_prior_term"]))
        worst[CC.SCALAR_TOL] = max(worst.get(CC.SCALAR_TOL, 0.0), e, e7)
        if not (e < CC.SCALAR_TOL and e7 <= CC.SCALAR_TOL):
            bad.append(("terms", e, e7))
        for k in ("Zbar", "zbbar") + CC.GP_NAMES:
            e = relerr(got[k], ref[k])
            worst[CC.GRAD_TOL] = max(worst.get(CC.GRAD_TOL, 0.0), e)
            if not e < CC.GRAD_TOL:
                bad.append((k, e))
        assert not bad, (name, batch, bad)
        assert torch.count_nonzero(got["object_vectors"][case["unused"]]) == 0
        assert torch.count_nonzero(got["object_vectors"][case["ids"]]) > 0
    print(f"envelope {name}{' norm' if normalize else ''} N={case['N']} H={case['H']} L={case['L']}: worst error "
          + ", ".join(f"{e:.1e} (bar {bar:.0e})" for bar, e in sorted(worst.items())))


@pytest.mark.parametrize("train", [(0, 1), (1, 0)], ids=["ov", "gp"])
@pytest.mark.parametrize("name", ["M128", "Q32"])
def test_untrained_groups_are_exact_zeros_and_the_rest_keeps_its_bits(name, train):
    case = _case(name, True)
    batch = case["batches"][2]

    def run(train_gp, train_ov):
        st, big, gp = _poisoned_stage(case, train_gp, train_ov)
        out = _run(st, gp, case, batch)
        assert _tail_intact(st, big)
        return out

    base = _ref(("bits", name), lambda: run(1, 1))
    got = run(*train)
    train_gp, train_ov = train
    for k, v in got.items():
        if (k in ("l_GP", "amplitude", "alpha") and not train_gp) or (k == "object_vectors" and not train_ov):
            assert torch.count_nonzero(v) == 0 and torch.count_nonzero(base[k]) > 0, k
        else:
            assert torch.equal(v, base[k]), k


# ---------------------------------------------------------------------------------------------------------- 2. the whole step
N_BIG = 277


def _big_problem():
    """real_problem on 40 objects x 8 angles (~90 % kept), the sorted rows truncated to N_BIG: more than the 256 weight-gradient
    partial slots of the encoder workspace, no multiple of 4 (dead waves in the row kernels) or 64 (a short last chunk)."""
    def build():
        prob = dict(CC.real_problem(np.load(GOLDEN), n_objects=40, n_angles=8, keep=0.9))
        assert prob["N"] >= N_BIG
        prob.update(N=N_BIG, images=prob["images"][:N_BIG].contiguous(), aux=prob["aux"][:N_BIG].copy(),
                    eps_f=prob["eps_f"][:N_BIG].contiguous())
        return prob
    return _ref("big", build)


def _check_step(eng, prob, regime, lo, hi, eps_b, key, *, clip=True, ov_joint=True, beta=0.7):
    """The checks of test_gpu_casale.py::test_step_on_real_images for one step; returns the worst (scalar, forward, gradient)."""
    L = prob["L"]
    out, grads = _ref(key, lambda: CC.step_reference(regime, prob["params"], prob["images"], prob["aux"], lo, hi, prob["eps_f"],
                                                     eps_b, beta=beta, clip=clip, normalize=False, L=L, ov_joint=ov_joint))
    if regime != "VAE" and clip:
        CC.assert_clip_margin(out["var_all"], lo, hi)
    eng.step(regime, lo, hi, eps_full=prob["eps_f"], eps_batch=eps_b, adam=False)
    sc = eng.scalars()
    names = ("elbo", "recon_loss", "KL_term") if regime == "VAE" else ("elbo", "recon_loss", "GP_prior_term", "log_var")
    w = [0.0, 0.0, 0.0]
    for k in names:
        e = abs(sc[k] - float(out[k])) / abs(float(out[k]))
        w[0] = max(w[0], e)
        assert e < CC.SCALAR_TOL, (k, sc[k], float(out[k]))
    for k in ("qnet_mu", "qnet_var", "recon"):
        e = relerr(eng.ws_view(k), out[k])
        w[1] = max(w[1], e)
        assert e < CC.FWD_TOL, (k, e)
    g = eng.grads()
    listed = CC.regime_variables(regime, ov_joint)
    assert set(g) == set(grads)
    for k, want in grads.items():
        if k not in listed:
            assert torch.count_nonzero(g[k]) == 0, k
            continue
        e = relerr(g[k], want)
        w[2] = max(w[2], e)
        assert e < CC.GRAD_TOL, (k, e)
    assert sc["adam_t"] == 0.0
    return w


@pytest.mark.parametrize("regime", ["joint", "GP"])
def test_step_past_256_train_rows(regime):
    """Two steps on one engine: a full batch of 256, then the ragged tail of 21 rows.  The encoder runs forward and reverse
    on a workspace of b = N = 277 rows, 21 past SVGP_MAX_PART."""
    prob = _big_problem()
    N, L = prob["N"], prob["L"]
    assert N > 256 and N % 4 != 0 and N % 64 != 0
    assert len(np.unique(prob["aux"][:, 2])) == 8
    eng = CC.step_engine(prob, batch_size=256, beta=0.7, clip=True, ov_joint=True)
    assert eng._cfgN.b == N and eng.batch_size == 256
    rng = np.random.RandomState(6)
    for lo, hi in ((0, 256), (256, N)):
        eps_b = CC.t64(rng.randn(hi - lo, L))
        w = _check_step(eng, prob, regime, lo, hi, eps_b, ("bigstep", regime, lo))
        print(f"step N={N} {regime} [{lo}, {hi}): worst scalar {w[0]:.1e}, forward {w[1]:.1e}, gradient {w[2]:.1e}")


def test_vae_regime_step_at_256_rows():
    prob = _big_problem()
    eng = CC.step_engine(prob, batch_size=256, beta=0.7, clip=True, ov_joint=True)
    eps_b = CC.t64(np.random.RandomState(7).randn(256, prob["L"]))
    w = _check_step(eng, prob, "VAE", 0, 256, eps_b, ("bigstep", "VAE", 0))
    print(f"step N={prob['N']} VAE [0, 256): worst scalar {w[0]:.1e}, forward {w[1]:.1e}, gradient {w[2]:.1e}")


@pytest.mark.parametrize("L", [64, 1])
def test_step_at_the_channel_limits(L):
    """A-sized real-image problem with every lane / one lane per row in the row-wise kernels: a full batch and the ragged tail."""
    def build():
        prob = CC.real_problem(np.load(GOLDEN), L=L)
        if L == 1:      # real_problem pushes channel 0 below the lower clip bound; with one channel that would cut the
            prob["params"]["enc_d_b"][1:] += 7.5        # whole variance path, so the single channel is put back inside
        return prob
    prob = _ref(("realL", L), build)
    N = prob["N"]
    assert N >= 18 and prob["L"] == L
    eng = CC.step_engine(prob, batch_size=8, beta=0.7, clip=True, ov_joint=True)
    rng = np.random.RandomState(3)
    for lo, hi in ((4, 12), (16, N)):
        eps_b = CC.t64(rng.randn(hi - lo, L))
        w = _check_step(eng, prob, "joint", lo, hi, eps_b, ("stepL", L, lo))
        print(f"step L={L} joint [{lo}, {hi}): worst scalar {w[0]:.1e}, forward {w[1]:.1e}, gradient {w[2]:.1e}")


# ---------------------------------------------------------------------------------------------------------- 3. row-wise kernels
def _glue_cfg(N, L):
    from svgp_vae_amd import _lib
    cfg = _lib.CasaleCfg(N=N, n_obj=1, Q=1, M=1, L=L, b_cap=N, normalize_obj=0, train_gp=1, train_ov=1)
    wl = _lib.CasaleLayout()
    _lib.call("svgp_casale_layout_get", C.byref(cfg), C.byref(wl))
    return cfg, wl


BOUNDS = (1e-3, 10.0, 100.0)


def _sample_problem():
    """37 rows x 9 channels = 333 entries: two lv partials, the second one short.  The first, the last and a middle row hold
    var_raw exactly at 1e-3, 10 and 100 and one ulp on either side of each; the rest is log-uniform in [1e-4, 1e3]."""
    def build():
        N, L = 37, 9
        rng = np.random.RandomState(71)
        var = np.exp(rng.uniform(np.log(1e-4), np.log(1e3), (N, L)))
        edge = np.array([f(b) for b in BOUNDS for f in (lambda x: np.nextafter(x, 0.0), lambda x: x, lambda x: np.nextafter(x, np.inf))])
        assert len(edge) == L and all(b in edge for b in BOUNDS)
        for row, shift in ((0, 0), (N - 1, 4), (N // 2, 7)):
            var[row] = np.roll(edge, shift)
        return dict(N=N, L=L, mu=CC.t64(rng.randn(N, L)), var=CC.t64(var), eps_f=CC.t64(rng.randn(N, L)),
                    Zbar=CC.t64(rng.randn(N, L)), rng_seed=72)
    return _ref("sample", build)


def _sample_reference(p, clip, lo, hi, eps_b, zbbar, dec_zbar, c_lv):
    """float64 autograd of the two samples of elbo_casale; torch.clamp passes the gradient at its bounds, like tf.clip_by_value."""
    mu, var = p["mu"].clone().requires_grad_(True), p["var"].clone().requires_grad_(True)
    Z = mu + p["eps_f"] * torch.sqrt(torch.clamp(var, 1e-3, 10.0) if clip else var)
    v2 = torch.clamp(var[lo:hi], 1e-3, 100.0) if clip else var[lo:hi]
    zb = mu[lo:hi] + eps_b * torch.sqrt(v2)
    lv = torch.sum(torch.log(v2))
    ybar, s2bar = torch.autograd.grad(torch.sum(p["Zbar"] * Z) + torch.sum((dec_zbar + zbbar) * zb) + c_lv * lv, [mu, var])
    return dict(Z=Z.detach(), zb=zb.detach(), qvar_b=v2.detach(), lv=lv.detach(), ybar=ybar, s2bar=s2bar)


@pytest.mark.parametrize("clip", [1, 0], ids=["clip", "noclip"])
@pytest.mark.parametrize("rng_", ["first", "last", "all"])
def test_samples_and_seeds_at_the_clip_bounds(rng_, clip):
    from svgp_vae_amd import _lib
    p = _sample_problem()
    N, L = p["N"], p["L"]
    lo, hi = dict(first=(0, 5), last=(N - 4, N), all=(0, N))[rng_]
    b = hi - lo
    cfg, wl = _glue_cfg(N, L)
    assert wl.n_lv >= 2 and (N * L) % 256 != 0
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(p["rng_seed"] + lo)
    eps_b, zbbar, dec_zbar = (CC.t64(rng.randn(b, L)) for _ in range(3))
    c_lv = -0.5 * 0.7 / L
    ref = _ref(("sample", rng_, clip), lambda: _sample_reference(p, clip, lo, hi, eps_b, zbbar, dec_zbar, c_lv))
    d = lambda t: t.to(dev).contiguous()
    mu, var, eps_f, eps_bd, dec = d(p["mu"]), d(p["var"]), d(p["eps_f"]), d(eps_b), d(dec_zbar)
    ws = torch.full((wl.total,), float("nan"), dtype=torch.float64, device=dev)
    z_dec = torch.full((b, L), float("nan"), dtype=torch.float64, device=dev)
    s = _stream(dev)
    _lib.call("svgp_casale_sample", C.byref(cfg), clip, lo, hi, mu.data_ptr(), var.data_ptr(), eps_f.data_ptr(), eps_bd.data_ptr(),
              z_dec.data_ptr(), ws.data_ptr(), s)
    view = lambda name, n: ws[getattr(wl, name):getattr(wl, name) + n]
    got = dict(Z=view("Z", N * L).view(N, L), zb=view("zb", b * L).view(b, L), qvar_b=view("qvar_b", b * L).view(b, L))
    for k, v in got.items():
        e = relerr(v, ref[k])
        assert e <= 1e-13, (k, e)
    assert torch.equal(z_dec, got["zb"])
    assert torch.equal(got["qvar_b"].cpu(), ref["qvar_b"])                      # a clip is a selection: bit for bit
    lv = float(view("lv_part", wl.n_lv).sum())
    e = abs(lv - float(ref["lv"])) / abs(float(ref["lv"]))
    print(f"sample {rng_} clip={clip} sum(lv_part) {e:.1e}")
    assert e <= 1e-13, (lv, float(ref["lv"]))
    # the seed of (mu, var_raw) over all N rows
    view("Zbar", N * L).copy_(d(p["Zbar"]).view(-1))
    view("zbbar", b * L).copy_(d(zbbar).view(-1))
    ybar, s2bar = (torch.full((N, L), float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
    seeds = lambda eps_f_, eps_b_, dec_, c: _lib.call(
        "svgp_casale_seeds", C.byref(cfg), clip, lo, hi, var.data_ptr(), eps_f_.data_ptr(), eps_b_.data_ptr(), dec_.data_ptr(), c,
        ybar.data_ptr(), s2bar.data_ptr(), ws.data_ptr(), s)
    seeds(eps_f, eps_bd, dec, c_lv)
    for k, v in (("ybar", ybar), ("s2bar", s2bar)):
        e = relerr(v, ref[k])
        print(f"seeds {rng_} clip={clip} {k} {e:.1e}")
        assert e <= 1e-12, (k, e)
    # the clip masks on their own, bounds included: Zbar = eps_f = 1 and nothing from the batch leaves 1 / (2 sqrt(v)) exactly
    # where [1e-3, 10] passes; dec_zbar = eps_b = 1 with Zbar = 0 does the same for [1e-3, 100] on the batch rows
    vr = p["var"]
    in_b = torch.zeros(N, L, dtype=torch.bool)
    in_b[lo:hi] = True
    pass10 = (vr >= 1e-3) & (vr <= 10.0) if clip else torch.ones_like(in_b)
    pass100 = ((vr >= 1e-3) & (vr <= 100.0) if clip else torch.ones_like(in_b)) & in_b
    if clip:
        assert 0 < int(pass10.sum()) < int(((vr >= 1e-3) & (vr <= 100.0)).sum()) < N * L
        for bound, m in ((1e-3, pass10), (10.0, pass10), (100.0, pass100)):
            at = (vr == bound) & in_b
            assert at.any() and m[at].all()                                     # the bound itself passes
    ones_f, ones_b, zero_b = torch.ones_like(eps_f), torch.ones_like(eps_bd), torch.zeros_like(dec)
    view("Zbar", N * L).fill_(1.0)
    view("zbbar", b * L).zero_()
    seeds(ones_f, ones_b, zero_b, 0.0)
    assert torch.equal(s2bar.cpu() != 0, pass10)
    view("Zbar", N * L).zero_()
    seeds(ones_f, ones_b, ones_b, 0.0)
    assert torch.equal(s2bar.cpu() != 0, pass100)


@pytest.mark.parametrize("b,L", [(1, 1), (85, 3), (257, 1)], ids=["bL1", "bL255", "bL257"])
def test_vae_glue_and_closing_scalars(b, L):
    """svgp_casale_vae_sample / _vae_seeds / _finalize (both modes) against their closed forms with one element, one short of a
    workgroup and one past it.  Bars: the element-wise results are three or four correctly rounded operations, held to 1e-14 of
    the tensor's max-abs; the sums (KL, whose terms are >= 0, and log_var) are held to 1e-13 relative to the float64 reference's
    value, the bar of sum(lv_part) in test_samples_and_seeds_at_the_clip_bounds: at most 257 terms, and the magnitudes of the
    log terms add up to less than 3 times |sum log var| with these inputs, so any summation order stays within
    3 * 257 * 2^-53 = 9e-14 of it."""
    from svgp_vae_amd import _lib
    cfg, wl = _glue_cfg(b, L)
    n = b * L
    n_part = -(-n // 256)
    assert wl.n_lv == n_part
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(80 + b)
    mu, eps, dec = (CC.t64(rng.randn(b, L)) for _ in range(3))
    var = CC.t64(np.exp(rng.uniform(np.log(1e-3), np.log(50.0), (b, L))))
    d = lambda t: t.to(dev).contiguous()
    mu_d, var_d, eps_d, dec_d = d(mu), d(var), d(eps), d(dec)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    ws, z, ybar, s2bar = nan(wl.total), nan(b, L), nan(b, L), nan(b, L)
    s = _stream(dev)
    _lib.call("svgp_casale_vae_sample", C.byref(cfg), b, mu_d.data_ptr(), var_d.data_ptr(), eps_d.data_ptr(), z.data_ptr(),
              ws.data_ptr(), s)
    assert relerr(z, mu + eps * torch.sqrt(var)) <= 1e-14
    kl_terms = 0.5 * (var + mu * mu - 1.0 - torch.log(var))
    assert float(kl_terms.min()) >= 0
    KL = float(ws[wl.lv_part:wl.lv_part + n_part].sum())
    assert abs(KL - float(kl_terms.sum())) <= 1e-13 * float(kl_terms.sum())
    scale = 0.5 / 0.01 ** 2 * 784.0
    _lib.call("svgp_casale_vae_seeds", C.byref(cfg), b, scale, mu_d.data_ptr(), var_d.data_ptr(), eps_d.data_ptr(),
              dec_d.data_ptr(), ybar.data_ptr(), s2bar.data_ptr(), s)
    assert relerr(ybar, scale * dec + mu) <= 1e-14
    assert relerr(s2bar, scale * dec * eps / (2 * torch.sqrt(var)) + 0.5 * (1 - 1 / var)) <= 1e-14
    # closing scalars, plain-VAE mode: KL from the partials above
    sq, beta, sigma = 123.456, 0.7, 0.01
    sums = torch.tensor([0.0, 0.0, sq, 0.0], dtype=torch.float64, device=dev)
    out, state = nan(8), torch.zeros(_lib.STATE_LEN, dtype=torch.float64, device=dev)
    fin = lambda mode, adam: _lib.call("svgp_casale_finalize", C.byref(cfg), mode, b, beta, sigma, sums.data_ptr(), adam,
                                       ws.data_ptr(), out.data_ptr(), state.data_ptr(), s)
    fin(1, 1)
    o = out.cpu()
    assert abs(float(o[0]) - (-(0.5 / sigma ** 2) * sq - KL)) <= 1e-14 * (0.5 / sigma ** 2) * sq
    assert float(o[1]) == sq / 784.0 and float(o[4]) == KL and torch.count_nonzero(o[[2, 3, 5, 6, 7]]) == 0
    assert float(state[_lib.STATE["ADAM_T"]]) == 1.0
    # Casale mode: log_var partials of svgp_casale_sample over the whole set as the batch, terms[7] as the GP prior term
    zdec = nan(b, L)
    _lib.call("svgp_casale_sample", C.byref(cfg), 0, 0, b, mu_d.data_ptr(), var_d.data_ptr(), eps_d.data_ptr(), eps_d.data_ptr(),
              zdec.data_ptr(), ws.data_ptr(), s)
    assert torch.equal(zdec, z)
    t7 = -4.321
    ws[wl.terms + 7] = t7
    fin(0, 0)
    o = out.cpu()
    lv = float(o[3])
    lv_ref = float(torch.log(var).sum())
    assert float(torch.log(var).abs().sum()) < 3 * abs(lv_ref)
    e =abs(lv - lv_ref) / abs(lv_ref)
    print(f"finalize b={b} L={L} log_var {e:.1e}")
    assert e <= 1e-13, (lv, lv_ref)
    want =sq / 784.0 - (beta / L) * (t7 + 0.5 * lv)
    assert abs(float(o[0]) - want) <= 1e-14 * (sq / 784.0 + (beta / L) * (abs(t7) + 0.5 * abs(lv)))
    assert float(o[1]) == sq / 784.0 and float(o[2]) == t7 and torch.count_nonzero(o[4:]) == 0
    st = state.cpu()
    assert float(st[_lib.STATE["ADAM_T"]]) == 1.0 and torch.count_nonzero(st) == 1          # did_adam = 0: no further count


@pytest.mark.parametrize("H", [1, 64, 65])
@pytest.mark.parametrize("N", [63, 65])
@pytest.mark.parametrize("T", [1, 5])
def test_predict_var_at_the_wave_edges(T, N, H):
    """var_i = k_ii - (|k_i|^2 - r_i . (P r_i)) / alpha with one lane short of, and one past, a pass of the wave over N and H.
    Bar: two sums of at most 65 terms each, 65 * 2^-53 = 7e-15 of the magnitudes that enter; 1e-13 of them."""
    from svgp_vae_amd import _lib
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(1000 * T + 10 * N + H)
    Ktn, ktt, R, RP = CC.t64(rng.randn(T, N)), CC.t64(rng.rand(T) + 40.0), CC.t64(rng.randn(T, H)), CC.t64(rng.randn(T, H))
    alpha = 0.15
    d = lambda t: t.to(dev).contiguous()
    a = [d(x) for x in (Ktn, ktt, R, RP, CC.t64([alpha]))]
    var = torch.full((T + 3,), CANARY, dtype=torch.float64, device=dev)
    _lib.call("svgp_casale_predict_var", T, N, H, *[x.data_ptr() for x in a], var.data_ptr(), _stream(dev))
    torch.cuda.synchronize()
    want = ktt - ((Ktn * Ktn).sum(1) - (R * RP).sum(1)) / alpha
    scale = ktt.abs() + ((Ktn * Ktn).sum(1) + (R * RP).abs().sum(1)) / alpha
    assert bool(((var[:T].cpu() - want).abs() <= 1e-13 * scale).all())
    assert bool((var[T:] == CANARY).all())
