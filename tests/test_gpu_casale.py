"""Casale GP-VAE on the GPU against the float64 CPU restatement (tests/casale_cases.py): the GP stage, the whole step in its
three regimes on real images, an Adam trajectory over the regimes, prediction and the refusals.

Bars (tests/helpers.relerr, relative to the tensor's max-abs): scalars 1e-9, row and matrix quantities 1e-8, gradients 1e-7,
trajectory ELBO and parameters 1e-8."""
import os

import numpy as np
import pytest
import torch

import svgp_vae_amd
from tests import casale_cases as CC
from tests.helpers import relerr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mnist_cfg2_inputs.npz")
_REF = {}


def _ref(key, fn):
    """References are computed once and shared."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------- 1. GP stage
@pytest.mark.parametrize("train", [(1, 1), (0, 1), (1, 0), (0, 0)], ids=["gp+ov", "ov", "gp", "fixed"])
@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "norm"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_gp_stage(name, normalize, train):
    from svgp_vae_amd.GPVAE_Casale_model import casale_gp_stage
    train_gp, train_ov = train
    case = CC.make_case(name, normalize=normalize)
    for batch in case["batches"]:
        lo, hi = batch
        ref = _ref(("gp", name, normalize, batch), lambda: CC.gp_stage_reference(case, batch))
        GP = CC.gp_object(case, ov_joint=bool(train_ov), fixed_gp=not train_gp)
        st = casale_gp_stage(GP, case["aux"][:, 1:], CC.t64(case["Z"]), CC.t64(case["zb"][batch]), lo, hi)
        b = hi - lo
        for k in ("K_W", "L_W", "V", "G", "P", "U", "A"):
            e = relerr(st.named(k, b), ref[k])
            print(f"{name} {k} {e:.2e}")
            assert e < CC.FWD_TOL, (k, e)
        terms = st.named("terms", b).cpu()
        assert relerr(terms[:3], ref["terms"]) < CC.SCALAR_TOL
        assert abs(float(terms[7]) - float(ref["GP_prior_term"])) <= CC.SCALAR_TOL * abs(float(ref["GP_prior_term"]))
        g = st.ws[st.wl.grad_gp:st.wl.grad_gp + 3 + case["n_obj"] * case["M"]].cpu()
        got = dict(Zbar=st.named("Zbar", b), zbbar=st.named("zbbar", b), l_GP=g[0], amplitude=g[1], alpha=g[2],
                   object_vectors=g[3:].view(case["n_obj"], case["M"]))
        for k, v in got.items():
            want = ref[k]
            if (k in ("l_GP", "amplitude", "alpha") and not train_gp) or (k == "object_vectors" and not train_ov):
                assert torch.count_nonzero(v) == 0, k
                continue
            e = relerr(v, want)
            print(f"{name} grad {k} {e:.2e}")
            assert e < CC.GRAD_TOL, (k, e)


# ---------------------------------------------------------------------------------------------------------- 2. the whole step
def _real(normalize=False):
    return _ref(("real", normalize), lambda: CC.real_problem(np.load(GOLDEN), normalize=normalize))


@pytest.mark.parametrize("ov_joint", [True, False], ids=["ovj", "ovfix"])
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("regime", ["joint", "GP", "VAE"])
def test_step_on_real_images(regime, clip, ov_joint):
    prob = _real()
    N, L, beta = prob["N"], prob["L"], 0.7
    assert N >= 18
    eng = CC.step_engine(prob, batch_size=8, beta=beta, clip=clip, ov_joint=ov_joint)
    rng = np.random.RandomState(3)
    for lo, hi in ((4, 12), (16, N)):                       # a full batch and the ragged tail
        eps_b = CC.t64(rng.randn(hi - lo, L))
        out, grads = _ref(("step", regime, clip, ov_joint, lo), lambda: CC.step_reference(
            regime, prob["params"], prob["images"], prob["aux"], lo, hi, prob["eps_f"], eps_b, beta=beta, clip=clip,
            normalize=False, L=L, ov_joint=ov_joint))
        if regime != "VAE" and clip:
            CC.assert_clip_margin(out["var_all"], lo, hi)
        eng.step(regime, lo, hi, eps_full=prob["eps_f"], eps_batch=eps_b, adam=False)
        sc = eng.scalars()
        names = ("elbo", "recon_loss", "KL_term") if regime == "VAE" else ("elbo", "recon_loss", "GP_prior_term", "log_var")
        for k in names:
            e = abs(sc[k] - float(out[k])) / abs(float(out[k]))
            print(f"{regime} {k} {e:.2e}")
            assert e < CC.SCALAR_TOL, (k, sc[k], float(out[k]))
        for k in ("qnet_mu", "qnet_var", "recon"):
            assert relerr(eng.ws_view(k), out[k]) < CC.FWD_TOL, k
        g = eng.grads()
        listed = CC.regime_variables(regime, ov_joint)
        assert set(g) == set(grads)
        for k, want in grads.items():
            if k not in listed:
                assert torch.count_nonzero(g[k]) == 0, k
                continue
            e = relerr(g[k], want)
            print(f"{regime} grad {k} {e:.2e}")
            assert e < CC.GRAD_TOL, (k, e)
        assert sc["adam_t"] == 0.0


# ---------------------------------------------------------------------------------------------------------- 3. trajectory
def test_adam_trajectory_over_the_regimes():
    """VAE, GP, joint, joint on B-sized data (real images, L 16, normalised object kernel): parameters and ELBO series;
    moments of untouched variables are bit-equal across a step that skips them; one shared step count."""
    prob = _ref("traj", lambda: CC.real_problem(np.load(GOLDEN), n_objects=12, n_angles=8, M=5, L=16, seed=9, normalize=True))
    N, L, beta = prob["N"], prob["L"], 0.7
    rng = np.random.RandomState(4)
    sched = []
    for regime, (lo, hi) in zip(("VAE", "GP", "joint", "joint"), ((0, 32), (32, 64), (40, 72), (N - 20, N))):
        sched.append((regime, lo, hi, CC.t64(rng.randn(N, L)), CC.t64(rng.randn(hi - lo, L))))
    p_ref, elbos, _, _ = CC.train_trajectory(prob["params"], prob["images"], prob["aux"], sched, beta=beta, clip=True,
                                             normalize=True, L=L, ov_joint=True)
    eng = CC.step_engine(prob, batch_size=32, beta=beta, clip=True, ov_joint=True)
    n_vae = eng.n_vae
    got = []
    for regime, lo, hi, eps_f, eps_b in sched:
        m0, v0 = eng.adam_m.clone(), eng.adam_v.clone()
        eng.step(regime, lo, hi, eps_full=eps_f, eps_batch=eps_b, adam=True)
        got.append(eng.scalars()["elbo"])
        skipped = slice(n_vae, None) if regime == "VAE" else (slice(0, n_vae) if regime == "GP" else slice(0, 0))
        assert torch.equal(eng.adam_m[skipped], m0[skipped]) and torch.equal(eng.adam_v[skipped], v0[skipped])
    for a, b in zip(got, elbos):
        print(f"elbo {a:.12g} ref {b:.12g}")
        assert abs(a - b) <= CC.TRAJ_TOL * abs(b)
    assert eng.scalars()["adam_t"] == 4.0
    for k, want in p_ref.items():
        e = relerr(eng.params[k], want)
        print(f"param {k} {e:.2e}")
        assert e < CC.TRAJ_TOL, (k, e)


# ---------------------------------------------------------------------------------------------------------- 4. prediction
@pytest.mark.parametrize("ov_joint", [True, False], ids=["ovj", "ovfix"])
def test_values_api_and_prediction(ov_joint):
    from svgp_vae_amd.GPVAE_Casale_model import encode, forward_pass_Casale, predict_test_set_Casale
    from svgp_vae_amd.VAE_utils import mnistVAE
    prob = _real()
    N, L, M, p = prob["N"], prob["L"], prob["M"], prob["params"]
    dev = torch.device("cuda:0")
    vae = mnistVAE(L=L)
    vae.params = {k: p[k].clone() for k in vae.params}
    GP = CC.gp_object(prob, ov_joint=ov_joint, values=p)
    from svgp_vae_amd.GPVAE_Casale_model import _angles_mask
    mask = _angles_mask(prob["aux"][:, 1:])
    V = GP.V_matrix(prob["aux"], mask)
    V_ref = CC.V_literal(p["object_vectors"], prob["aux"], mask, p["l_GP"], p["amplitude"], False)
    assert relerr(V, V_ref) < CC.FWD_TOL
    Z = encode(prob["images"].to(dev), vae, clipping_qs=True, epsilon=prob["eps_f"])
    mu, var = CC.O.MnistVAE(p, L).encode(prob["images"])
    Z_ref = mu + prob["eps_f"] * torch.sqrt(torch.clamp(var, 1e-3, 10))
    assert relerr(Z, Z_ref) < CC.FWD_TOL
    a, B, c = GP.taylor_coeff(Z, V)
    a_ref, B_ref, c_ref = CC.taylor_coeff_literal(Z_ref, V_ref, p["alpha"])
    for got, want in ((a, a_ref), (B, B_ref), (c, c_ref)):
        assert got.shape == want.shape and relerr(got, want) < CC.FWD_TOL
    # the 7-tuple from the materialised coefficients
    lo, hi, beta = 4, 12, 0.7
    rng = np.random.RandomState(8)
    eps_b = CC.t64(rng.randn(hi - lo, L))
    tup = forward_pass_Casale((prob["images"][lo:hi].to(dev), CC.t64(prob["aux"][lo:hi])), vae, a, B, c, V, beta, GP,
                              clipping_qs=True, epsilon=eps_b)
    out, _ = CC.step_reference("GP", p, prob["images"], prob["aux"], lo, hi, prob["eps_f"], eps_b, beta=beta, clip=True,
                               normalize=False, L=L, ov_joint=ov_joint, formulation="literal", mask=mask)
    for got, k in zip(tup[:4], ("elbo", "recon_loss", "GP_prior_term", "log_var")):
        assert abs(float(got) - float(out[k])) <= CC.SCALAR_TOL * abs(float(out[k])), k
    for got, k in zip(tup[4:], ("qnet_mu", "qnet_var", "recon")):
        assert relerr(got, out[k]) < CC.FWD_TOL, k
    # conditional generation at held-out angles of the train objects
    T = 7
    ids = rng.randint(0, 6, T).astype(np.float64)
    test_aux = CC.t64(np.concatenate([np.stack([ids, rng.uniform(0, 6.28, T)], 1), p["object_vectors"].numpy()[ids.astype(int)]], 1))
    train_aux = CC.t64(np.concatenate([prob["aux"], p["object_vectors"].numpy()[prob["aux"][:, 1].astype(int)]], 1))
    test_images = prob["images"][:T]
    eps_t = CC.t64(rng.randn(T, L))
    for take_mean in (True, False):
        rec, loss = predict_test_set_Casale(test_images.to(dev), test_aux, train_aux, vae, GP, V, Z, take_mean=take_mean,
                                            epsilon=eps_t)
        rec_ref, loss_ref, _, var_ref = CC.predict_reference(test_images, test_aux, train_aux, p, V_ref, Z_ref, L=L,
                                                             normalize=False, ov_joint=ov_joint, take_mean=take_mean,
                                                             epsilon=eps_t)
        if var_ref is not None:
            assert float(var_ref.min()) > 0
        assert relerr(rec, rec_ref) < CC.FWD_TOL
        assert abs(float(loss) - float(loss_ref)) <= CC.SCALAR_TOL * abs(float(loss_ref))


# ---------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_raise_before_any_launch():
    from svgp_vae_amd.GPVAE_Casale_model import CasaleStepEngine, casale_gp_stage, casaleGP
    from svgp_vae_amd.VAE_utils import mnistVAE
    rng = np.random.RandomState(0)

    def problem(P, Q, M):
        aux = np.array([[p, 0.1 * q] for p in range(P) for q in range(Q)], dtype=np.float64)
        return casaleGP(False, rng.randn(P, M), False, True), aux

    GP, aux = problem(2, 33, 2)
    with pytest.raises(svgp_vae_amd.SvgpError, match="Q <= 32"):
        casale_gp_stage(GP, aux, torch.zeros(len(aux), 2), torch.zeros(4, 2), 0, 4)
    GP, aux = problem(1, 17, 121)                                # H = 2057
    with pytest.raises(svgp_vae_amd.SvgpError, match="H <= 2048"):
        casale_gp_stage(GP, aux, torch.zeros(len(aux), 2), torch.zeros(4, 2), 0, 4)
    GP, aux = problem(3, 4, 2)
    with pytest.raises(svgp_vae_amd.SvgpError, match="batch range"):
        casale_gp_stage(GP, aux, torch.zeros(12, 2), torch.zeros(4, 2), 9, 13)
    full = np.concatenate([np.arange(12.0)[:, None], aux], 1)
    with pytest.raises(svgp_vae_amd.SvgpError, match="single GPU"):
        CasaleStepEngine(mnistVAE(L=2), GP, np.zeros((12, 28, 28, 1)), full, batch_size=4, world_size=2)
    eng = CasaleStepEngine(mnistVAE(L=2), GP, np.zeros((12, 28, 28, 1)), full, batch_size=4)
    with pytest.raises(svgp_vae_amd.SvgpError, match="batch range"):
        eng.step("joint", 10, 13)
    with pytest.raises(svgp_vae_amd.SvgpError, match="batch range"):
        eng.step("joint", 0, 5)


# ---------------------------------------------------------------------------------------------------------- 5. driver
def test_driver_follows_the_reference_trajectory(tmp_path):
    """--elbo GPVAE_Casale --opt_regime VAE-1 GP-1 joint-2 on a 96-row train pickle (2 batches, the second ragged): the
    per-step ELBO series equals train_trajectory; test_metrics.txt has one line per evaluation."""
    import pickle

    from svgp_vae_amd import MNIST_experiment
    from svgp_vae_amd.GPVAE_Casale_model import sort_train_data
    from svgp_vae_amd.VAE_utils import mnistVAE
    g = np.load(GOLDEN)
    rng = np.random.RandomState(21)
    rows = rng.permutation(len(g["aux"]))
    tr, te = rows[:96], rows[96:108]
    data = str(tmp_path) + "/"
    pickle.dump(dict(images=g["images"][tr], aux_data=g["aux"][tr]), open(data + "train96.p", "wb"))
    pickle.dump(dict(images=g["images"][te], aux_data=g["aux"][te]), open(data + "test_data3.p", "wb"))
    L, seed = 4, 0
    log = MNIST_experiment.main(["--elbo", "GPVAE_Casale", "--opt_regime", "VAE-1", "GP-1", "joint-2", "--epsilon_seed", "0",
                                 "--save", "--ov_joint", "--GP_joint", "--clip_qs", "--L", str(L), "--batch_size", "64",
                                 "--train_file", data + "train96.p", "--mnist_data_path", data, "--base_dir", data,
                                 "--eval_every", "2", "--seed", str(seed)])
    # the same initial values and schedule on the CPU
    np.random.seed(seed)
    ov = np.random.normal(0, 1.5, 400 * 8).reshape(400, 8)
    params = {k: v.clone() for k, v in mnistVAE(L=L, seed=seed).params.items()}
    params.update(l_GP=CC.t64(1.0), amplitude=CC.t64(1.0), alpha=CC.t64(0.1), object_vectors=CC.t64(ov))
    train = sort_train_data(dict(images=g["images"][tr], aux_data=g["aux"][tr]))
    sched = []
    for epoch, regime in enumerate(("VAE", "GP", "joint", "joint")):
        for i, (lo, hi) in enumerate(((0, 64), (64, 96))):
            sched.append((regime, lo, hi, CC.t64(np.random.RandomState(1000 * epoch + i).randn(96, L)),
                          CC.t64(np.random.RandomState(500000 + 1000 * epoch + i).randn(hi - lo, L))))
    _, elbos, _, _ = CC.train_trajectory(params, CC.t64(train["images"]), train["aux_data"][:, :3], sched, beta=0.001,
                                         clip=True, normalize=False, L=L, ov_joint=True)
    assert len(log["step_elbo"]) == 8
    for a, b in zip(log["step_elbo"], elbos):
        print(f"driver elbo {a:.12g} ref {b:.12g}")
        assert abs(a - b) <= CC.TRAJ_TOL * abs(b)
    lines = open(log["chkpnt_dir"] + "pics/test_metrics.txt").read().split()
    assert [ln.split(",")[0] for ln in lines] == ["2", "4"]
    assert [float(ln.split(",")[1]) for ln in lines] == [round(c, 4) for _, c in log["cgen_mse"]]
    assert os.path.exists(log["chkpnt_dir"] + "cgen_images.p")
    with pytest.raises(NotImplementedError):
        MNIST_experiment.main(["--elbo", "GPVAE_Casale_batch"])


# ---------------------------------------------------------------------------------------------------------- reference-executed fixture
@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "norm"])
def test_against_the_reference_executed_fixture(normalize):
    """V, a, B, c, the 7-tuple, every gradient of elbo and the prediction (mean and sampled) against what the reference's
    own code computes (tests/golden/ref_casale_small.npz)."""
    from svgp_vae_amd.GPVAE_Casale_model import (CasaleStepEngine, encode, forward_pass_Casale, predict_test_set_Casale)
    from svgp_vae_amd.VAE_utils import mnistVAE
    fx = np.load(os.path.join(os.path.dirname(GOLDEN), "ref_casale_small.npz"))
    tag = "norm" if normalize else "raw"
    prob = CC.fixture_problem(np.load(GOLDEN), normalize)
    p, L, lo, hi, beta = prob["params"], prob["L"], prob["lo"], prob["hi"], prob["beta"]
    dev = torch.device("cuda:0")
    vae = mnistVAE(L=L)
    vae.params = {k: p[k].clone() for k in vae.params}
    GP = CC.gp_object(prob["case"], ov_joint=True, normalize=normalize)
    V = GP.V_matrix(prob["aux"], prob["case"]["mask"])
    assert relerr(V, fx[f"{tag}.V"]) < CC.FWD_TOL
    Z = encode(prob["images"].to(dev), vae, clipping_qs=True, epsilon=prob["eps_f"])
    assert relerr(Z, fx[f"{tag}.Z"]) < CC.FWD_TOL
    a, B, c = GP.taylor_coeff(Z, V)
    for got, k in ((a, "a"), (B, "B"), (c, "c")):
        assert got.shape == fx[f"{tag}.{k}"].shape and relerr(got, fx[f"{tag}.{k}"]) < CC.FWD_TOL, k
    tup = forward_pass_Casale((prob["images"][lo:hi].to(dev), CC.t64(prob["aux"][lo:hi])), vae, a, B, c, V, beta, GP,
                              clipping_qs=True, epsilon=prob["eps_b"])
    for got, k in zip(tup, ("elbo", "recon_loss", "GP_prior_term", "log_var", "qnet_mu", "qnet_var", "recon_images")):
        want = fx[f"{tag}.fwd.{k}"]
        assert relerr(got, want) < (CC.SCALAR_TOL if want.ndim == 0 else CC.FWD_TOL), k
    for take_mean in (True, False):
        rec, loss = predict_test_set_Casale(prob["test_images"].to(dev), prob["test_aux"], CC.t64(prob["aux"]), vae, GP, V, Z,
                                            take_mean=take_mean, epsilon=prob["eps_t"])
        kind = "mean" if take_mean else "sample"
        e_rec, e_loss = relerr(rec, fx[f"{tag}.predict.{kind}.recon"]), relerr(loss, fx[f"{tag}.predict.{kind}.loss"])
        print(f"fixture predict {kind} recon {e_rec:.2e} loss {e_loss:.2e}")
        assert e_rec < CC.FWD_TOL and e_loss < CC.SCALAR_TOL, kind
    # the training step: scalars and every gradient of elbo
    eng = CasaleStepEngine(vae, GP, prob["images"], prob["aux"][:, :3], batch_size=hi - lo, beta=beta, clipping_qs=True)
    eng.step("joint", lo, hi, eps_full=prob["eps_f"], eps_batch=prob["eps_b"], adam=False)
    sc = eng.scalars()
    for k in ("elbo", "recon_loss", "GP_prior_term", "log_var"):
        assert abs(sc[k] - float(fx[f"{tag}.fwd.{k}"])) <= CC.SCALAR_TOL * abs(float(fx[f"{tag}.fwd.{k}"])), k
    for k, g in eng.grads().items():
        e = relerr(g, fx[f"{tag}.grad.{k}"])
        print(f"fixture grad {k} {e:.2e}")
        assert e < CC.GRAD_TOL, (k, e)
