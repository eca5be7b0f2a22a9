"""Plain VAE / conditional VAE on rotated MNIST: float64 CPU restatement of the reference, the case table and the problem
builders of the CVAE tests.  Test infrastructure only.

Written from forward_pass_standard_VAE_rotated_mnist (SVGPVAE_model.py:718-782), mnistVAE / mnistCVAE (VAE_utils.py:99-162,
165-258), KL_term_standard_normal_prior (:261-272), predict_CVAE (SVGPVAE_model.py:785-820) and the step of
MNIST_experiment.py:188-208 (the loss is -elbo, TF1 Adam).  Gradients come from autograd.

Bars (tests/helpers.relerr: relative to the tensor's max-abs), those of tests/casale_cases.py: scalars 1e-9, stored fields
1e-8, gradients 1e-7, trajectory elbo and parameters 1e-8.  The restatement evaluated with the batch rows in reverse order moves by
less than 1e-12 (tests/test_cvae_cases_cpu.py), so the bars are not spent on the reference's own summation order.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import svgpvae_oracle as O

DT = torch.float64
SCALAR_TOL, FWD_TOL, GRAD_TOL, TRAJ_TOL = 1e-9, 1e-8, 1e-7, 1e-8
FUSED_LIMIT = 64            # largest L of the fused step (svgp_cvae_lds_bytes): the library's ceiling, so there is no split form

VAE_NAMES = [n for n, _ in O.mnist_vae_param_shapes(1)]


def param_shapes(L, cvae):
    out = []
    for name, shp in O.mnist_vae_param_shapes(L):
        if cvae:
            shp = dict(enc_c1_w=(3, 3, 3, 8), enc_d_w=(34, 2 * L), dec_d_w=(L + 2, 128), dec_c1_w=(3, 3, 10, 8)).get(name, shp)
        out.append((name, shp))
    return out


def glorot_params(L, cvae, seed):
    rng = np.random.RandomState(seed)
    p = {}
    for name, shp in param_shapes(L, cvae):
        if name.endswith("_b"):
            p[name] = 0.1 * rng.randn(*shp)              # non-zero: the bias gradients carry signal
        else:
            rf = shp[0] * shp[1] if len(shp) == 4 else 1
            fan_in, fan_out = (rf * shp[2], rf * shp[3]) if len(shp) == 4 else shp
            lim = math.sqrt(6.0 / (fan_in + fan_out))
            p[name] = rng.uniform(-lim, lim, size=shp)
    return p


def t64(x):
    return torch.as_tensor(np.asarray(x), dtype=DT)


# The smallest shapes where csrc/cvae.hip can go wrong.  Every case runs for both variants.
#   b1_L1     degenerate loops
#   b2_L16    the reference's default L
#   b257_L4   one workgroup walks two images: partials accumulate across images, the next image is staged
#   b40_cap64 ragged batch in a larger workspace: offsets fixed by b_cap
#   L64_b3    the fused limit and the ceiling (L = 65 is refused: there is no split form); every L-sized LDS row full
#   L63_b2    one below the limit: a row count that is no multiple of the 8- and 16-lane groups of the dense products
#   angles    {0, -0.3, 7.0, pi/2} in one batch: constant planes, border of the same-padded first up-convolution, per-row angle
#   clip      clip_qs with shifted encoder biases: exp(.) below 1e-3, inside, above 10
CASES = dict(
    b1_L1=dict(b=1, L=1, seed=51),
    b2_L16=dict(b=2, L=16, seed=52),
    b257_L4=dict(b=257, L=4, seed=53),
    b40_cap64=dict(b=40, b_cap=64, L=5, seed=54),
    L64_b3=dict(b=3, L=64, seed=55),
    L63_b2=dict(b=2, L=63, seed=56),
    angles=dict(b=4, L=3, seed=57, angles=(0.0, -0.3, 7.0, math.pi / 2)),
    clip=dict(b=6, L=4, seed=58, clip=True),
)


def make_case(name, cvae):
    c = dict(CASES[name])
    rng = np.random.RandomState(c["seed"] + (1000 if cvae else 0))
    b, L = c["b"], c["L"]
    p = glorot_params(L, cvae, c["seed"])
    if c.get("clip"):
        p["enc_d_b"][L:] += np.array([-9.0, 0.3, 4.5, -0.2])[np.arange(L) % 4]
    images = np.clip(0.142 + 0.316 * rng.randn(b, 28, 28, 1), -0.2, 1.2)
    ang = np.asarray(c["angles"]) if "angles" in c else rng.uniform(0, 2 * math.pi, b)
    aux = np.stack([rng.randint(0, 5, b).astype(np.float64), ang], 1)
    c.update(name=name, cvae=bool(cvae), b_cap=c.get("b_cap", b), clip=bool(c.get("clip", False)), sigma=0.01,
             params={k: t64(v) for k, v in p.items()}, images=t64(images), aux=t64(aux), eps=t64(rng.randn(b, L)))
    return c


# ------------------------------------------------------------------------------------------------------------ the networks
def encode(p, images, angles, L, cvae):
    """mnistVAE.encode (VAE_utils.py:143-152) / mnistCVAE.encode (:218-233) with the input planes of SVGPVAE_model.py:737-740."""
    x = images
    if cvae:
        b = images.shape[0]
        sin_ = torch.sin(angles).reshape(b, 1, 1, 1).expand(b, 28, 28, 1)
        cos_ = torch.cos(angles).reshape(b, 1, 1, 1).expand(b, 28, 28, 1)
        x = torch.cat([images, sin_, cos_], 3)
    h = F.elu(O._conv2d_nhwc(x, p["enc_c1_w"], p["enc_c1_b"], 2, 'valid'))
    h = F.elu(O._conv2d_nhwc(h, p["enc_c2_w"], p["enc_c2_b"], 2, 'valid'))
    h = F.elu(O._conv2d_nhwc(h, p["enc_c3_w"], p["enc_c3_b"], 2, 'valid'))
    h = h.reshape(h.shape[0], -1)
    if cvae:
        h = torch.cat([h, torch.sin(angles)[:, None], torch.cos(angles)[:, None]], 1)
    enc = h @ p["enc_d_w"] + p["enc_d_b"]
    return enc[:, :L], torch.exp(enc[:, L:])


def decode(p, z, angles, cvae):
    """mnistVAE.decode (VAE_utils.py:154-162) / mnistCVAE.decode (:235-258)."""
    b = z.shape[0]
    if cvae:
        z = torch.cat([z, torch.sin(angles)[:, None], torch.cos(angles)[:, None]], 1)
    h = (z @ p["dec_d_w"] + p["dec_d_b"]).reshape(b, 4, 4, 8)
    if cvae:
        h = torch.cat([h, torch.sin(angles).reshape(b, 1, 1, 1).expand(b, 4, 4, 1),
                       torch.cos(angles).reshape(b, 1, 1, 1).expand(b, 4, 4, 1)], 3)
    h = F.elu(O._conv2d_nhwc(O._upsample2_nhwc(h), p["dec_c1_w"], p["dec_c1_b"], 1, 'same'))
    h = F.elu(O._conv2d_nhwc(O._upsample2_nhwc(h), p["dec_c2_w"], p["dec_c2_b"], 1, 'valid'))
    h = F.elu(O._conv2d_nhwc(O._upsample2_nhwc(h), p["dec_c3_w"], p["dec_c3_b"], 1, 'same'))
    return h


def forward(p, images, aux, eps, *, L, cvae, clip=False, sigma=0.01):
    """forward_pass_standard_VAE_rotated_mnist (SVGPVAE_model.py:718-782); returns (-elbo, dict of the 7-tuple)."""
    ang = aux[:, 1]
    mu, var = encode(p, images, ang, L, cvae)
    if clip:
        var = O.clip_by_value(var, 1e-3, 10.0)
    z = mu + eps * torch.sqrt(var)
    recon = decode(p, z, ang, cvae)
    sq = torch.sum((images - recon) ** 2)
    KL = O.KL_term_standard_normal_prior(mu, var)
    elbo = -(0.5 / sigma ** 2) * sq - KL
    return -elbo, dict(recon_loss=sq / 784.0, KL_term=KL, elbo=elbo, recon=recon, qnet_mu=mu, qnet_var=var, z=z)


def step_reference(params, images, aux, eps, *, L, cvae, clip=False, sigma=0.01):
    p = {k: t64(v).clone().requires_grad_(True) for k, v in params.items()}
    obj, out = forward(p, images, aux, eps, L=L, cvae=cvae, clip=clip, sigma=sigma)
    names = list(p)
    g = torch.autograd.grad(obj, [p[k] for k in names])
    return {k: v.detach() for k, v in out.items()}, dict(zip(names, g))


def case_reference(c):
    return step_reference(c["params"], c["images"], c["aux"], c["eps"], L=c["L"], cvae=c["cvae"], clip=c["clip"], sigma=c["sigma"])


def train_trajectory(params, batches, *, L, cvae, lr, clip=False, sigma=0.01):
    """batches: list of (images, aux, eps).  TF1 Adam on -elbo, one step per batch.  Returns (params, elbos, m, v)."""
    p = {k: t64(v).clone() for k, v in params.items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(x) for k, x in p.items()}
    elbos = []
    for t, (images, aux, eps) in enumerate(batches, start=1):
        out, g = step_reference(p, images, aux, eps, L=L, cvae=cvae, clip=clip, sigma=sigma)
        elbos.append(float(out["elbo"]))
        O.adam_tf1_step(p, g, m, v, t, lr)
    return p, elbos, m, v


def predict_reference(p, images_train, images_test, aux_train, aux_test, eps, *, L):
    """predict_CVAE (SVGPVAE_model.py:785-820): no clipping, group means over equal ids (empty group: NaN), decoded at the test
    row's angle, mean squared error over all test pixels."""
    mu, var = encode(p, images_train, aux_train[:, 1], L, True)
    z = mu + eps * torch.sqrt(var)
    means = []
    for t in range(aux_test.shape[0]):
        mask = aux_train[:, 0] == aux_test[t, 0]
        means.append(z[mask].sum(0) / mask.sum().to(DT))          # rows in ascending order; 0 / 0 = NaN like reduce_mean of nothing
    zt = torch.stack(means, 0)
    recon = decode(p, zt, aux_test[:, 1], True)
    return recon, torch.mean((images_test - recon) ** 2)


def assert_clip_margin(var_raw, rel=1e-6):
    v = var_raw.detach()
    for bound in (1e-3, 10.0):
        assert float(((v - bound).abs() / bound).min()) > rel, bound
