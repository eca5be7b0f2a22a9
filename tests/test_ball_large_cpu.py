"""CPU-side checks of the moving-ball large engine (csrc/ball_large.hip, ball.BallLargeStepEngine): the ABI, every refusal with
its message and before any launch, the workspace size query, the engine choice, the reverse algebra the large-m factor stage
follows for the ball's KL form, the efficient step oracle of tests/ball_large_cases.py against the literal one, and the oracle's
own one-ulp response at every case of the table (the guard of tests/test_ball_envelope_oracle_cpu.py)."""
import ctypes as C
import os
import re

import pytest
import torch

import svgp_vae_amd
from oracle import ball_oracle as BO
from oracle import staged_gp as SG
from oracle import svgpvae_oracle as O
from svgp_vae_amd import _lib
from svgp_vae_amd._lib import BallLargeCfg, WsLayout
from tests import ball_cases as BC
from tests import ball_large_cases as LC
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = torch.float64
NEW_SYMBOLS = ("svgp_ball_large_ws_layout_get", "svgp_ball_large_workspace_elems", "svgp_ball_large_gp_fwd",
               "svgp_ball_large_gp_bwd", "svgp_ball_large_elbo_assemble")
FAKE = 4096                                                     # never dereferenced: every case fails validation first
ONE_ULP = 1.0 + 2.0 ** -52


def _cfg(T=130, B=3, m=65, titsias=0, kl_form=1, clip_pv=2, jitter=1e-6):
    return BallLargeCfg(T=T, B=B, m=m, titsias=titsias, kl_form=kl_form, clip_pv=clip_pv, jitter=jitter)


def test_header_declares_and_library_exports_the_large_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svgpvae_hip.h")).read(), flags=re.S)
    lib = svgp_vae_amd.load_library()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", src), f"{n} not declared in include/svgpvae_hip.h"
        assert hasattr(lib, n), f"{n} not exported"
        assert n in _lib.SIGNATURES or n in _lib.NON_STATUS
    assert lib.svgp_struct_sizeof(10) == C.sizeof(BallLargeCfg)
    ceiling = int(re.search(r"#define\s+SVGP_BALL_LARGE_MAX_VIDEOS\s+(\d+)", src).group(1))
    assert ceiling == _lib.BALL_LARGE_MAX_VIDEOS >= 256


def _layout(q):
    _lib.call("svgp_ball_large_ws_layout_get", C.byref(q), C.byref(WsLayout()))


def _fwd(q):
    _lib.call("svgp_ball_large_gp_fwd", C.byref(q), FAKE, FAKE, FAKE, None, FAKE, FAKE, None)


def _bwd(q):
    _lib.call("svgp_ball_large_gp_bwd", C.byref(q), FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None)


def _asm(q):
    _lib.call("svgp_ball_large_elbo_assemble", C.byref(q), FAKE, FAKE, FAKE, FAKE, FAKE, None)


@pytest.mark.parametrize("run", [_layout, _fwd, _bwd, _asm])
def test_bad_configurations_are_refused_with_their_message(run):
    lib = svgp_vae_amd.load_library()
    with pytest.raises(svgp_vae_amd.SvgpError, match="m=2049"):
        run(_cfg(m=2049))
    with pytest.raises(svgp_vae_amd.SvgpError, match=f"B={_lib.BALL_LARGE_MAX_VIDEOS + 1} videos"):
        run(_cfg(B=_lib.BALL_LARGE_MAX_VIDEOS + 1))
    with pytest.raises(svgp_vae_amd.SvgpError, match="kl_form=0"):
        run(_cfg(kl_form=0))
    with pytest.raises(svgp_vae_amd.SvgpError, match="kl_form=2"):
        run(_cfg(kl_form=2))
    with pytest.raises(svgp_vae_amd.SvgpError, match="clip_pv=1"):
        run(_cfg(clip_pv=1))
    for bad in (dict(m=0), dict(B=0), dict(T=0)):
        with pytest.raises(svgp_vae_amd.SvgpError, match="bad shape"):
            run(_cfg(**bad))
    with pytest.raises(svgp_vae_amd.SvgpError, match="titsias=2"):
        run(_cfg(titsias=2))
    # SVGP_ERR_UNSUPPORTED for the two ceilings, before any pointer is looked at
    assert lib.svgp_ball_large_gp_fwd(C.byref(_cfg(m=2049)), None, None, None, None, None, None, None) == -2
    assert lib.svgp_ball_large_gp_bwd(C.byref(_cfg(B=257)), None, None, None, None, None, None, None, None) == -2


def test_null_pointers_are_refused_before_any_launch():
    q = _cfg()
    with pytest.raises(svgp_vae_amd.SvgpError, match="cfg is NULL"):
        _lib.call("svgp_ball_large_gp_fwd", None, FAKE, FAKE, FAKE, None, FAKE, FAKE, None)
    with pytest.raises(svgp_vae_amd.SvgpError, match="out is NULL"):
        _lib.call("svgp_ball_large_ws_layout_get", C.byref(q), None)
    for k in (0, 1, 2, 4, 5):                                       # times, ip, ls, ws, state (eps may be NULL: Philox)
        args = [FAKE, FAKE, FAKE, None, FAKE, FAKE]
        args[k] = None
        with pytest.raises(svgp_vae_amd.SvgpError, match="NULL device pointer"):
            _lib.call("svgp_ball_large_gp_fwd", C.byref(q), *args, None)
    for k in range(7):                                              # times, ip, ls, ws, state, d_ip, d_ls
        args = [FAKE] * 7
        args[k] = None
        with pytest.raises(svgp_vae_amd.SvgpError, match="NULL device pointer"):
            _lib.call("svgp_ball_large_gp_bwd", C.byref(q), *args, None)
    for k in range(5):
        args = [FAKE] * 5
        args[k] = None
        with pytest.raises(svgp_vae_amd.SvgpError, match="NULL device pointer"):
            _lib.call("svgp_ball_large_elbo_assemble", C.byref(q), *args, None)


def test_workspace_grows_with_m_and_batch_and_matches_the_layout():
    lib = svgp_vae_amd.load_library()
    ws = lambda **kw: int(lib.svgp_ball_large_workspace_elems(C.byref(_cfg(**kw))))
    sizes = [ws(m=m) for m in (1, 8, 64, 65, 129, 512, 513, 2048)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    sizes = [ws(B=B) for B in (1, 3, 64, 65, 256)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    assert ws(T=260) > ws(T=130)
    assert ws(titsias=1) > ws(titsias=0)
    B, m = 65, 96
    assert ws(B=B, m=m) >= 12 * B * m * m                           # the (batch, m, m) blocks dominate
    wl = WsLayout()
    _lib.call("svgp_ball_large_ws_layout_get", C.byref(_cfg(B=B, m=m)), C.byref(wl))
    assert wl.total == ws(B=B, m=m)
    assert wl.enc_a1 == wl.enc_a2 == wl.enc_a3                      # no fields of the MNIST networks
    assert wl.KL - wl.M2 == 0 and wl.q - wl.KL >= 2 * B             # large-m form; [KL | tr(Ki A A)]
    for bad in (dict(m=2049), dict(B=257), dict(kl_form=0), dict(clip_pv=0), dict(T=0)):
        assert ws(**bad) == 0


def test_existing_entry_points_keep_their_refusals():
    cfg = _lib.MnistCfg(b=30, b_global=30, m=80, L=35, M=1, n_obj=0, N_train=30.0, jitter=1e-6, kl_form=1, clip_pv=2)
    with pytest.raises(svgp_vae_amd.SvgpError, match="moving-ball SVGP"):
        _lib.call("svgp_mnist_ws_layout_get", C.byref(cfg), C.byref(WsLayout()))
    cfg = _lib.MnistCfg(b=30, b_global=30, m=8, L=65, M=1, n_obj=0, N_train=30.0, jitter=1e-6, kl_form=1, clip_pv=2)
    with pytest.raises(svgp_vae_amd.SvgpError, match="more than 64 latent channels"):
        _lib.call("svgp_mnist_ws_layout_get", C.byref(cfg), C.byref(WsLayout()))


def test_engine_choice_and_engine_refusals():
    from svgp_vae_amd import ball
    assert ball.sparse_engine_class(64, 64) is ball.BallStepEngine
    assert ball.sparse_engine_class(65, 8) is ball.BallLargeStepEngine
    assert ball.sparse_engine_class(8, 65) is ball.BallLargeStepEngine
    mk = lambda n, m: ball.SVGP(False, m, False, 1, 30, 2.0, False, n, 1e-6, 1, 30, 2.0)
    with pytest.raises(svgp_vae_amd.SvgpError, match="m=2049"):
        ball.BallLargeStepEngine(mk("x", 2049), mk("y", 2049), batch=4, tmax=30, px=8, py=8, hidden=8)
    with pytest.raises(svgp_vae_amd.SvgpError, match="B=300 videos"):
        ball.BallLargeStepEngine(mk("x", 80), mk("y", 80), batch=300, tmax=30, px=8, py=8, hidden=8)
    if not torch.cuda.is_available():
        with pytest.raises(svgp_vae_amd.SvgpError, match="no CPU execution path"):
            ball.BallLargeStepEngine(mk("x", 80), mk("y", 80), batch=4, tmax=30, px=8, py=8, hidden=8)


# ---------------------------------------------------------------------------------------------------------
# The reverse factor stage of gp_large.hip ("W form", oracle/staged_gp.py gp_factor_bwd_w) with the ball's KL form, as the
# kernels compute it (k_ball_dmat, k_ball_asum and the plain vector chain): D_l = Ki - Aji_l + L (Ki A_l + A_l Ki) in the place
# of Ki - Aji_l, sum_l (A_l + L A_l A_l) in the place of sum_l A_l, ubar = ud, mubar = Ki ubar.  Held to autograd here, so that a
# GPU mismatch points at the kernels and not at the algebra.
# ---------------------------------------------------------------------------------------------------------
def _factor_bwd_w_ball(K, v, f, A2, SW, ud, td, loc, gT, c, N_train, b_global):
    L, m = v.shape
    g3, gK = gT, -gT * (b_global / N_train)
    Ki, Si, A, Aji, mu, t, G = (f[k] for k in ('Ki', 'Si', 'A', 'Aji', 'mu', 't', 'G'))
    M = Ki[None] @ A
    D = Ki[None] - Aji + L * (M + M.transpose(1, 2))
    Hm = G @ D
    HG = Hm @ G.transpose(1, 2)
    ubar = ud
    mubar = ubar @ Ki.T
    tbar = td + c * (mubar @ K.T)
    tv = torch.einsum('li,lj->lij', tbar, v)
    X = A2 - 0.5 * g3 * SW + 0.5 * (tv + tv.transpose(1, 2))
    vbar = torch.einsum('lij,lj->li', Si, tbar)
    Sg0 = -(Si @ X @ Si)
    Ssym = c * (Sg0 + Sg0.transpose(1, 2)) - c * gK * HG
    Zs = Hm.sum(0)
    Kb_win = 0.5 * gK * (Zs + Zs.T) + c * torch.einsum('li,lj->ij', mubar, t) + (Sg0 - 0.5 * gK * HG).sum(0)
    Kib_win = 0.5 * gK * (A + L * (A @ A)).sum(0) + torch.einsum('li,lj->ij', ubar, mu)
    Kib_loc = loc['Qs'] + loc['Pbar'] @ K
    Kbar = (Kb_win - Ki @ Kib_win @ Ki + (0.5 * gK * L) * Ki) + (Ki @ loc['Pbar'] - Ki @ Kib_loc @ Ki)
    return dict(Kbar=Kbar, vbar=vbar, Ssym=Ssym)


def test_w_form_reverse_pass_with_the_ball_kl_form_matches_autograd():
    g = torch.Generator().manual_seed(2)
    L, T, m = 4, 10, 5
    x = torch.arange(T, dtype=DT) + 1.0
    y, s2 = torch.randn(T, L, dtype=DT, generator=g), torch.rand(T, L, dtype=DT, generator=g) * 2 + 0.05
    z = torch.linspace(1.0, float(T), m, dtype=DT) + 0.1 * torch.randn(m, dtype=DT, generator=g)
    ls = torch.tensor(1.7, dtype=DT)
    K, Kn, knn = BO.se_matrix(z[:, None], z[:, None], ls), BO.se_matrix(x[:, None], z[:, None], ls), torch.ones(T, dtype=DT)
    eps, zbar = torch.randn(T, L, dtype=DT, generator=g), torch.randn(T, L, dtype=DT, generator=g)
    N, j, gT, c = float(T), 1e-6, -0.41, 1.0
    lv = [t.clone().requires_grad_() for t in (K, Kn, knn, y, s2)]
    p_m, p_v, L3, KL = O.gp_block_efficient(*lv, j, N, kl_form=1)
    ce = O.gauss_cross_entropy(p_m, p_v, lv[3], lv[4]).sum()
    loss = gT * (-ce + L3.sum() - KL.sum()) + (zbar * (p_m + eps * torch.sqrt(p_v))).sum()
    gs = torch.autograd.grad(loss, lv)
    p = O.reciprocal_no_nan(s2)
    S, v, _ = SG.gp_stats(Kn, p, p * y)
    f = SG.gp_factor_fwd(K, S, v, j, c, 1)
    ps = SG.gp_posterior_fwd_w(Kn, knn, y, s2, eps, f, c, K)
    g_pv, g_pm, mvbar = SG.gp_posterior_bwd_weights(y, s2, eps, ps, zbar, gT, c)
    A2, ud, td = SG.gp_stats(Kn, g_pv, mvbar, c * g_pm)
    loc = SG.gp_rows_local_w(Kn, ps, g_pv, gT, K, f['Ki'])
    fb = _factor_bwd_w_ball(K, v, f, A2, SG.gp_sw_rows(ps), ud, td, loc, gT, c, N, N)
    man = (fb['Kbar'],) + SG.gp_posterior_bwd_rows_w(Kn, knn, y, s2, ps, f, fb, loc, g_pv, g_pm, mvbar, gT, c, K)
    for name, a, b_ in zip(("K", "Kn", "knn", "y", "s2"), gs, man):
        if name == "K":                                             # the kernel-matrix reverse pass reads Kbar + Kbar^T only
            a, b_ = a + a.T, b_ + b_.T
        assert float((a - b_).abs().max() / a.abs().max()) < 1e-9, name


# ---------------------------------------------------------------------------------------------------------
# the step oracle
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["m65", "m65_tit"])
def test_efficient_oracle_equals_the_literal_one(case):
    cs = LC.LARGE_CASES[case]
    p, vid, eps, out, grads = LC.large_reference(case)
    lit, _, lgrads = BC.sparse_oracle(cs, p, vid, eps)
    for i, n in enumerate(LC.OUT_NAMES):
        want = lit[i] if torch.is_tensor(lit[i]) else torch.full((cs["batch"],), float(lit[i]), dtype=DT)
        e = H.relerr(out[i], want)
        print(f"{case} {n}: {e:.2e}")
        assert e < 1e-10, (n, e)
    for k in BO.PARAM_ORDER:
        e = H.relerr(grads[k], lgrads[k])
        print(f"{case} grad {k}: {e:.2e}")
        assert e < 1e-8, (k, e)


@pytest.mark.parametrize("case", list(LC.LARGE_CASES))
def test_large_case_oracle_response_is_far_below_the_tolerances(case):
    cs = LC.LARGE_CASES[case]
    p, vid, eps, out, grads = LC.large_reference(case)
    out2, _, grads2 = LC.large_oracle(cs, {k: v * ONE_ULP for k, v in p.items()}, vid, eps)
    for o in out:
        assert torch.isfinite(o).all()
    e_out = max(H.relerr(o2, o) for o, o2 in zip(out, out2))
    e_elbo = abs(float(out2[0].mean()) - float(out[0].mean())) / abs(float(out[0].mean()))
    e_grad = max(H.relerr(grads2[k], grads[k]) for k in grads)
    print(f"{case}: oracle response outputs {e_out:.2e}, mean elbo {e_elbo:.2e}, gradients {e_grad:.2e}")
    assert e_out <= BC.OUT_TOL / 100, (case, e_out)
    assert e_elbo <= BC.ELBO_TOL / 100, (case, e_elbo)
    assert e_grad <= BC.GRAD_TOL / 100, (case, e_grad)
