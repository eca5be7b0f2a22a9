"""Case table and step oracle of the moving-ball large engine (svgp_vae_amd.ball.BallLargeStepEngine: more than 64 inducing
points or more than 64 videos per batch), shared by tests/test_ball_large_cpu.py and tests/test_gpu_ball_large.py.

The literal oracle (oracle/ball_oracle.py) forms a (batch, tmax, m, m) tensor -- 6 GB at batch 65, m 96 -- so the expected values
come from a composition of oracle pieces that are each pinned elsewhere: mlp_inference -> svgpvae_oracle.gp_block_efficient(...,
kl_form=1) per latent coordinate (titsias_block_efficient for the Titsias L_2) -> mlp_decoder, gradients from autograd.  The
per-video KL is recovered from the per-channel pieces as in tests/test_ball_oracle.py (the reference adds one batch-wide scalar
to every video).  tests/test_ball_large_cpu.py holds this composition to the literal oracle at the smallest case.

Frames 8 x 8, hidden 16, jitter 1e-6, beta 0.8, clipping_qs, inputs from ball_cases._problem.  The Titsias ELBO is more sensitive
to the conditioning of K_mm, so two of its cases use a shorter length scale (cond(K_mm + jI) about 5 instead of about 65); a case
whose oracle fails the one-ulp guard of tests/test_ball_large_cpu.py gets another lt or tmax, never a wider tolerance.
"""
import functools

import torch

from oracle import ball_oracle as BO
from oracle import svgpvae_oracle as O
from oracle.ball_oracle import mlp_decoder, mlp_inference, se_matrix
from tests import ball_cases as BC

DT = torch.float64

_SHAPES = {
    # case: (batch, tmax, m, lt Hensman, lt Titsias)
    "m65": (3, 130, 65, 2.0, 2.0),          # first size past the LDS path
    "B65_m66": (65, 132, 66, 2.0, 2.0),     # first batch past 64 channels; the batch-wide KL scalar over 65 videos
    "m129": (2, 258, 129, 2.0, 2.0),        # one past a 128-wide block step
    "m257": (2, 260, 257, 1.0, 0.7),        # one past 256
    "m513": (2, 520, 513, 1.0, 0.7),        # Cholesky branch of the SPD inverse (m >= 512), D matrices materialised
    "m8_B65": (65, 40, 8, 4.0, 4.0),        # m <= 64 on the large-m kernels (more than 64 videos); tmax >= 3 m: SW from S_l
}
LARGE_CASES = {}
for _name, (_B, _T, _m, _lh, _lt) in _SHAPES.items():
    LARGE_CASES[_name] = dict(batch=_B, tmax=_T, m=_m, titsias=False, lt=_lh)
    LARGE_CASES[_name + "_tit"] = dict(batch=_B, tmax=_T, m=_m, titsias=True, lt=_lt)

OUT_NAMES = ("elbo", "recon", "KL_term", "inside_elbo", "ce_term", "full_p_mu", "full_p_var", "qnet_mu", "qnet_var",
             "pred_vid", "l_x", "l_y", "inside_recon", "inside_kl", "ip_x", "ip_y", "cov_mean_x", "cov_mean_y")


def large_problem(case):
    cs = LARGE_CASES[case]
    return BC._problem(cs["batch"], cs["tmax"], BC.ENV_PX, BC.ENV_HIDDEN, cs["m"], seed=60 + list(LARGE_CASES).index(case),
                       lt=cs["lt"])


def efficient_loss_and_grads(params, vid, eps, *, beta, titsias, jitter, clipping_qs=True):
    """BO.loss_and_grads without (batch, tmax, m, m) temporaries: (the 18 outputs of build_SVGPVAE_elbo_graph, loss, grads)."""
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    B, T, px, py = vid.shape
    t = torch.arange(T, dtype=DT) + 1.0
    mu, var = mlp_inference(leaf, vid)
    if clipping_qs:
        var = torch.clamp(var, 1e-6, 1e3)
    pm, pv, cov, rec, kl = [], [], [], 0.0, torch.zeros(B, dtype=DT)
    for c, cn in enumerate("xy"):
        z, l = leaf[f"ip_{cn}"], leaf[f"l_{cn}"]
        K, Kn, knn = se_matrix(z[:, None], z[:, None], l), se_matrix(t[:, None], z[:, None], l), torch.ones(T, dtype=DT)
        y, s2 = mu[:, :, c].T, var[:, :, c].T
        p_m, p_v, L3, KL, aux = O.gp_block_efficient(K, Kn, knn, y, s2, jitter, float(T), want_aux=True, kl_form=1)
        if titsias:
            rec = rec + O.titsias_block_efficient(K, Kn, knn, y, s2, jitter)
        else:
            klq = torch.einsum('ij,ljk,lki->l', aux["Ki"], aux["A_hat"], aux["A_hat"])
            rec, kl = rec + L3, kl + KL - 0.5 * B * klq + 0.5 * klq.sum()
        pm.append(p_m.T); pv.append(p_v.T)
        Knn = se_matrix(t[:, None], t[:, None], l)
        cov.append(Knn - Kn @ aux["Ki"] @ Kn.T + Kn @ aux["Si"].mean(0) @ Kn.T)
    fm, fv = torch.stack(pm, 2), torch.stack(pv, 2)
    ce = -O.gauss_cross_entropy(fm, fv, mu, var).sum((1, 2))
    zz = fm + eps * torch.sqrt(torch.clamp(fv, 1e-4, 1000))
    logits = mlp_decoder(leaf, zz, px, py)
    recon = -torch.nn.functional.binary_cross_entropy_with_logits(logits, vid, reduction="none").sum((1, 2, 3))
    inside = rec - kl
    klt = ce + inside
    elbo = recon + beta * klt
    loss = -elbo.mean()
    gs = torch.autograd.grad(loss, [leaf[k] for k in BO.PARAM_ORDER], allow_unused=True)
    grads = {k: (torch.zeros_like(leaf[k]) if g is None else g) for k, g in zip(BO.PARAM_ORDER, gs)}
    out = (elbo, recon, klt, inside, ce, fm, fv, mu, var, torch.sigmoid(logits), leaf["l_x"], leaf["l_y"], rec, kl,
           leaf["ip_x"], leaf["ip_y"], cov[0], cov[1])
    return tuple(o.detach() for o in out), loss.detach(), grads


def large_oracle(cs, p, vid, eps):
    return efficient_loss_and_grads(p, vid, eps, beta=BC.SPARSE_BETA, titsias=cs["titsias"], jitter=BC.SPARSE_JITTER,
                                    clipping_qs=True)


@functools.lru_cache(maxsize=None)
def large_reference(case):
    """(params, videos, eps, oracle outputs, oracle gradients) of a LARGE_CASES entry; computed once per process and shared:
    callers must not write to it."""
    p, vid, eps = large_problem(case)
    out, _, grads = large_oracle(LARGE_CASES[case], p, vid, eps)
    return p, vid, eps, out, grads


def large_engine(p, cs, **kw):
    """The engine ball.sparse_engine_class picks for the case, on the case's parameters."""
    from svgp_vae_amd import ball
    B, T, m = cs["batch"], cs["tmax"], cs["m"]
    fixed_ip, fixed_gp = kw.pop("fixed_ip", False), kw.pop("fixed_gp", False)
    mk = lambda n: ball.SVGP(cs["titsias"], m, fixed_ip, 1, T, 2.0, fixed_gp, n, BC.SPARSE_JITTER, 1, T, 2.0)
    sx, sy = mk("x"), mk("y")
    flat = {k: (v.reshape(-1) if k.startswith(("encB", "decB", "l_")) else v) for k, v in p.items()}
    kw.setdefault("beta", BC.SPARSE_BETA)
    return ball.sparse_engine_class(m, B)(sx, sy, batch=B, tmax=T, px=BC.ENV_PX, py=BC.ENV_PX, hidden=BC.ENV_HIDDEN,
                                          clip_qs=True, params=flat, **kw)
