"""--bias_analysis / --save_latents of the rotated-MNIST driver (MNIST_experiment.py:172-187, 325-363, 531-541; supplement C.4)
from the engine up: the device-side sum of the per-step mean vectors, the whole-train-set pass, the latent samples, and the
driver's bias line against a loop over the oracle written out here."""
import glob
import json
import math
import pickle

import numpy as np
import pytest
import torch

from oracle import svgpvae_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu
DT = torch.float64
N = 640                      # rows of the golden split: batches 256 / 256 / 128


# ---------------------------------------------------------------------------------------------------------
# engine: accumulation behind the step
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,L,b,titsias", [(32, 16, 64, False), (72, 3, 40, False), (32, 16, 64, True)],
                         ids=["m32", "m72-large-m-path", "m32-titsias"])
def test_engine_sums_the_mean_vectors_of_three_steps(m, L, b, titsias):
    """Three optimiser steps with mean_vectors_accumulate() behind each: the accumulator holds x1 + x2 + x3, added in that order on
    the host from clones of ws[mu_hat] taken after each step, to the bit, and the count 3.  A second engine that never accumulates
    ends with the same theta, to the bit.  mean_vectors_bias then agrees with the host function on the same three vectors: the
    terms are the same float64 numbers, the two sums of m (and of L) terms each obey the sum rule 2^-52 (n + 8) sum |term|."""
    from svgp_vae_amd.utils import compute_bias_variance_mean_estimators
    params = H.toy_problem(b=b, m=m, L=L, M=4, n_obj=20, seed=0)[0]
    batches = [H.toy_problem(b=b, m=m, L=L, M=4, n_obj=20, seed=s)[1:] for s in (1, 2, 3)]
    kw = dict(geco=True, N_train=400.0, jitter=1e-4 if titsias else 1e-6, titsias=titsias)
    eng, plain = H.engine_for(params, b, **kw), H.engine_for(params, b, **kw)
    with pytest.raises(ValueError):
        eng.mean_vectors_accumulate()                       # before mean_vectors_begin()
    eng.mean_vectors_begin()
    with pytest.raises(ValueError, match="no step"):
        eng.mean_vectors_bias(torch.zeros(L, m, dtype=DT))
    xs = []
    for images, aux, eps in batches:
        for e in (eng, plain):
            e.bind(images.to(e.device), aux.to(e.device), eps.to(e.device))
            e.run(adam=True)
            if e is eng:
                e.mean_vectors_accumulate()
            e.synchronize()
        xs.append(eng.ws_view("mu_hat", (L, m)).clone().cpu())
    assert not torch.equal(xs[0], xs[1]) and not torch.equal(xs[1], xs[2])
    acc = eng._mv_acc.cpu()
    assert torch.equal(acc[:L * m], (xs[0] + xs[1] + xs[2]).reshape(-1))
    assert float(acc[L * m]) == 3.0
    assert torch.equal(eng.theta.cpu(), plain.theta.cpu())
    assert eng.scalars()["adam_t"] == 3.0
    full = xs[1] * 1.01
    bias, per = eng.mean_vectors_bias(full)
    want = float(compute_bias_variance_mean_estimators(xs, full))
    scale = float(np.mean([np.abs((xs[0] + xs[1] + xs[2])[l].numpy() / 3 - full[l].numpy()).sum() for l in range(L)]))
    print(f"engine bias {bias!r} host {want!r}")
    assert per.shape == (L,) and abs(float(per.mean()) - bias) <= 2 * 2.0 ** -52 * (L + 8) * scale
    assert abs(bias - want) <= 2 * 2.0 ** -52 * (m + 8 + L + 8) * scale
    eng.mean_vectors_begin()                                # the next epoch starts from zero
    eng.synchronize()
    assert float(eng._mv_acc.abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------------
# the whole-train-set pass and the latent samples on the 640-row golden split, fresh parameters
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def split(golden):
    """Parameters, images, aux, eps of the 640 rows, and the oracle's encodings of all rows (with the clip), computed once."""
    params, images, aux, eps = H.golden_problem(golden, slice(0, N))
    ovae, osv = O.make_models(params, False, 1e-6, float(N), 16)
    mu, var = ovae.encode(images)
    return params, images, aux, eps, osv, mu, O.clip_by_value(var, 1e-3, 10.0)


def test_mean_vectors_full_matches_the_oracle(split):
    """ovae.encode over all rows, the clip, and osv.mean_vector_bias_analysis per channel with N_train = 640 (c = 1): the project's
    bound for these vectors (tests/test_gpu_api.py, test_forward_pass_bias_analysis).  Training state is only read."""
    params, images, aux, eps, osv, mu, var = split
    eng = H.engine_for(params, N, geco=True, clip_qs=True, N_train=float(N))
    eng.set_batch_size(256)
    before = [t.clone() for t in (eng.theta, eng.adam_m, eng.adam_v, eng.state)]
    got = eng.mean_vectors_full(images, aux)
    assert got.shape == (16, 32)
    for l in range(16):
        err = H.relerr(got[l], osv.mean_vector_bias_analysis(aux, mu[:, l], var[:, l]))
        assert err < 1e-8, (l, err)
    for a, b_ in zip(before, (eng.theta, eng.adam_m, eng.adam_v, eng.state)):
        assert torch.equal(a, b_)
    assert (eng.cfg.b, eng.cfg.b_global) == (256, 256)
    with pytest.raises(ValueError, match="capacity"):
        H.engine_for(params, 256, geco=True, N_train=float(N)).mean_vectors_full(images, aux)


def _models(params):
    from svgp_vae_amd.SVGPVAE_model import mnistSVGP
    from svgp_vae_amd.VAE_utils import mnistVAE
    VAE = mnistVAE(L=16)
    VAE.params = {k: params[k].clone() for k in VAE.params}
    SVGP_ = mnistSVGP(titsias=False, fixed_inducing_points=False, initial_inducing_points=params["inducing_index_points"].numpy(),
                      fixed_gp_params=False, object_vectors_init=params["object_vectors"].numpy(), name='main', jitter=1e-6,
                      N_train=N, L=16, K_obj_normalize=False)
    return VAE, SVGP_


def test_latent_samples_match_the_oracle(split):
    """p_m + eps sqrt(p_v) from approximate_posterior_params(aux, aux, mu_l, var_l) per channel (utils.py:995-1006): the bound of
    the 16-tuple members (tests/test_gpu_api.py, test_forward_pass_SVGPVAE_sixteen_tuple)."""
    from svgp_vae_amd.SVGPVAE_model import batching_encode_SVGPVAE_full
    from svgp_vae_amd.utils import latent_samples_SVGPVAE
    params, images, aux, eps, osv, mu, var = split
    VAE, SVGP_ = _models(params)
    gmu, gvar = batching_encode_SVGPVAE_full(images, VAE, clipping_qs=True)
    assert H.relerr(gmu, mu) < 1e-12 and H.relerr(gvar, var) < 1e-12
    got = latent_samples_SVGPVAE(images, aux, VAE, SVGP_, clipping_qs=True, epsilon=eps)
    want = []
    for l in range(16):
        p_m, p_v, _, _ = osv.approximate_posterior_params(aux, aux, mu[:, l], var[:, l])
        want.append(p_m + eps[:, l] * torch.sqrt(p_v))
    err = H.relerr(got, torch.stack(want, 1))
    print(f"latent samples rel err {err:.3e}")
    assert got.shape == (N, 16) and got.is_cuda and err < 1e-8
    a = latent_samples_SVGPVAE(images, aux, VAE, SVGP_, clipping_qs=True)
    b_ = latent_samples_SVGPVAE(images, aux, VAE, SVGP_, clipping_qs=True)
    assert a.shape == (N, 16) and torch.isfinite(a).all() and torch.isfinite(b_).all() and not torch.equal(a, b_)


# ---------------------------------------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------------------------------------
SPANS = [(0, 256), (256, 512), (512, N)]
EPS_OF = lambda epoch, i, b, L: np.random.RandomState(1000 * epoch + i + 7).randn(b, L)
# |driver bias - oracle bias| <= TOL * S, S = mean_l sum_j |full_lj| (the scale of the subtracted vectors; the bias itself is a
# difference and may be small).  TOL is to be ten times the largest |diff| / S measured on the MI355X over the three cases and both
# epochs, rounded up to a power of ten (the margin: the oracle's LU inverse against the device's elimination at other seeds).
# NOT MEASURED YET: 1e-6 is a placeholder, the project's bound for the parameters after the same six updates
# (tests/test_gpu_api.py, test_cli_driver_epoch_trajectory_matches_oracle), of which the mean vectors are a smooth function.  The
# test prints every figure before it asserts; NOTEBOOK.md ("Bias analysis and latents") says what to do with them.
TOL = 1e-6


def _data_dir(gin, tmp_path):
    d = str(tmp_path) + "/"
    pickle.dump({"images": gin["images"][:N], "aux_data": gin["aux"][:N]}, open(d + "train_data3.p", "wb"))
    for name, sl in (("eval_data3.p", slice(0, 64)), ("test_data3.p", slice(64, 128))):
        pickle.dump({"images": gin["images"][sl], "aux_data": gin["aux"][sl]}, open(d + name, "wb"))
    pickle.dump(gin["object_vectors"], open(d + "pca_ov_init3.p", "wb"))
    return d


def _argv(d, elbo, extra):
    return ["--elbo", elbo, "--mnist_data_path", d, "--train_file", d + "train_data3.p", "--ip_joint", "--GP_joint", "--ov_joint",
            "--clip_qs", "--PCA", "--opt_regime", "joint-2", "--eval_every", "100", "--lr", "0.002", "--seed", "3"] + extra


def _oracle_bias_run(gin, GECO, titsias):
    """The train_trajectory state machine (MNIST_experiment.py:313-355) with the bias analysis of :325-363 around it: the mean
    vectors of every step at the parameters BEFORE its update, the whole-set vectors at the parameters the epoch ends with."""
    from svgp_vae_amd.utils import compute_bias_variance_mean_estimators, generate_init_inducing_points
    params = {k: torch.tensor(v, dtype=DT) for k, v in O.glorot_uniform_init(16, seed=3).items()}
    ip = generate_init_inducing_points(None, n=2, PCA=True, M=8, aux_data=np.asarray(gin["aux"][:N]))   # (pinned bit for bit by
    params["inducing_index_points"] = torch.tensor(ip, dtype=DT)                  # test_cli_driver_epoch_trajectory_matches_oracle)
    params["l_GP"], params["amplitude"] = torch.tensor(1.0, dtype=DT), torch.tensor(1.0, dtype=DT)
    params["object_vectors"] = torch.tensor(gin["object_vectors"], dtype=DT)
    img, aux = torch.tensor(gin["images"][:N], dtype=DT), torch.tensor(gin["aux"][:N], dtype=DT)
    m_state = {k: torch.zeros_like(v) for k, v in params.items()}
    v_state = {k: torch.zeros_like(v) for k, v in params.items()}
    C_ma, lagr, first, t = torch.zeros((), dtype=DT), torch.ones((), dtype=DT), True, 0
    kappa, kw = math.sqrt(0.020), dict(clipping_qs=True, GECO=GECO)
    steps, biases, scales = [], [], []
    for epoch in range(2):
        mean_vectors_arr = []
        for i, (lo, hi) in enumerate(SPANS):
            t += 1
            eps = torch.tensor(EPS_OF(epoch, i, hi - lo, 16), dtype=DT)
            alpha = 0.0 if (GECO and first) else 0.99
            out, grads = O.loss_and_grads(params, img[lo:hi], aux[lo:hi], eps, beta=0.001, C_ma=C_ma, lagrange_mult=lagr, alpha=alpha,
                                          kappa=kappa, jitter=1e-6, N_train=float(N), L=16, formulation="efficient", titsias=titsias,
                                          **kw)
            ovae, osv = O.make_models(params, titsias, 1e-6, float(N), 16)
            fwd = O.forward_pass_SVGPVAE((img[lo:hi], aux[lo:hi]), 0.001, ovae, osv, C_ma, lagr, alpha, kappa, epsilon=eps,
                                         formulation="efficient", bias_analysis=True, **kw)
            mean_vectors_arr.append([v.numpy().copy() for v in fwd[15]])
            O.adam_tf1_step(params, grads, m_state, v_state, t, 0.002)
            if GECO:
                C_ma, lagr = out[13], out[14]
            first = False
            steps.append(dict(elbo=float(out[0]), recon_loss=float(out[1]), C_ma=float(out[13]), lagrange_mult=float(out[14])))
        ovae, osv = O.make_models(params, titsias, 1e-6, float(N), 16)
        mu, var = ovae.encode(img)
        var = O.clip_by_value(var, 1e-3, 10.0)
        full = [osv.mean_vector_bias_analysis(aux, mu[:, l], var[:, l]).numpy() for l in range(16)]
        biases.append(float(compute_bias_variance_mean_estimators(mean_vectors_arr, full)))
        scales.append(float(np.mean([np.abs(f).sum() for f in full])))
    return steps, biases, scales


@pytest.mark.parametrize("elbo,GECO", [("SVGPVAE_Hensman", True), ("SVGPVAE_Hensman", False), ("SVGPVAE_Titsias", True)])
def test_cli_driver_prints_the_bias_of_every_epoch(golden, tmp_path, capsys, elbo, GECO):
    """The setup of test_cli_driver_epoch_trajectory_matches_oracle (640 rows, batches 256 / 256 / 128, two epochs, the same
    epsilon_fn) with --bias_analysis: one bias per epoch within TOL * S of the oracle loop, and the per-step log within that
    test's 1e-8."""
    from svgp_vae_amd import MNIST_experiment as E
    gin, _ = golden
    d = _data_dir(gin, tmp_path)
    args = E.build_parser().parse_args(_argv(d, elbo, ["--bias_analysis", "--log_json", d + "log.json"] + (["--GECO"] if GECO else [])))
    args.epsilon_fn = EPS_OF
    log = E.run_experiment_rotated_mnist_SVGPVAE(args)
    printed = capsys.readouterr().out
    assert json.load(open(d + "log.json"))["bias"] == [[epoch, bias] for epoch, bias in log["bias"]]
    steps, biases, scales = _oracle_bias_run(gin, GECO, "Titsias" in elbo)
    assert [s["rows"] for s in log["steps"]] == [256, 256, 128] * 2
    assert len(log["bias"]) == 2 and [e for e, _ in log["bias"]] == [0, 1]
    for epoch, bias in log["bias"]:
        assert f"Bias for epoch {epoch}: {bias}" in printed
    worst = 0.0
    for (epoch, got), want, S in zip(log["bias"], biases, scales):
        print(f"{elbo} GECO={GECO} epoch {epoch}: bias {got!r} oracle {want!r} S {S!r} |diff| / S {abs(got - want) / S:.3e}")
        worst = max(worst, abs(got - want) / S)
    step_worst = max(abs(got[k] - want[k]) / max(1.0, abs(want[k])) for got, want in zip(log["steps"], steps)
                     for k in ("elbo", "recon_loss", "C_ma", "lagrange_mult"))
    print(f"{elbo} GECO={GECO}: worst |bias diff| / S {worst:.3e} (TOL {TOL:.0e}); worst per-step log error {step_worst:.3e}")
    assert worst <= TOL
    for t, (got, want) in enumerate(zip(log["steps"], steps)):
        for k in ("elbo", "recon_loss", "C_ma", "lagrange_mult"):
            assert abs(got[k] - want[k]) <= 1e-8 * max(1.0, abs(want[k])), (t, k, got[k], want[k])
    assert log["_engine"].scalars()["adam_t"] == 6.0


def test_cli_driver_without_the_flags_logs_no_bias(golden, tmp_path):
    from svgp_vae_amd import MNIST_experiment as E
    gin, _ = golden
    args = E.build_parser().parse_args(_argv(_data_dir(gin, tmp_path), "SVGPVAE_Hensman", ["--GECO", "--opt_regime", "joint-1"]))
    args.epsilon_fn = EPS_OF
    log = E.run_experiment_rotated_mnist_SVGPVAE(args)
    assert "bias" not in log and "_latents" not in log
    assert getattr(log["_engine"], "_mv_acc", None) is None          # the accumulator is never allocated, no launch is added


def test_cli_driver_saves_the_latents(golden, tmp_path):
    """--save_latents without --save is refused; with --save --epsilon_seed 7 the pickle holds the (640, 16) array of
    log["_latents"], and an identical second run reproduces it to the bit."""
    from svgp_vae_amd import MNIST_experiment as E
    gin, _ = golden
    d = _data_dir(gin, tmp_path)
    with pytest.raises(ValueError, match="--save"):
        E.run_experiment_rotated_mnist_SVGPVAE(E.build_parser().parse_args(_argv(d, "SVGPVAE_Hensman", ["--GECO", "--save_latents"])))
    runs = []
    for k in range(2):
        base = d + f"run{k}"
        argv = _argv(d, "SVGPVAE_Hensman", ["--GECO", "--opt_regime", "joint-1", "--save", "--save_latents", "--epsilon_seed", "7", "--base_dir", base,
                                            "--log_json", base + ".json"])
        log = E.run_experiment_rotated_mnist_SVGPVAE(E.build_parser().parse_args(argv))
        files = glob.glob(base + "/debug_MNIST/*/latents_train_full.p")
        assert len(files) == 1
        z = pickle.load(open(files[0], "rb"))
        assert isinstance(z, np.ndarray) and z.shape == (N, 16) and z.dtype == np.float64 and np.isfinite(z).all()
        assert np.array_equal(z, log["_latents"].cpu().numpy())
        runs.append(z)
    assert np.array_equal(runs[0], runs[1])
    assert "_latents" not in json.load(open(base + ".json")) and "bias" not in json.load(open(base + ".json"))
