"""Casale posterior cache and conditional generation on the GPU against the literal float64 oracle
(tests/casale_generate_cases.py has the cases, the query rows, the references and the bars; tests/test_casale_generate_cpu.py the
guard that makes the bars meaningful).  Bar: casale_cases.FWD_TOL = 1e-8 with helpers.relerr; bit-equality where stated."""
import ctypes as C
import glob
import os
import pickle

import numpy as np
import pytest
import torch

from tests import casale_cases as CC
from tests import casale_generate_cases as CG
from tests.helpers import relerr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mnist_cfg2_inputs.npz")
DT = torch.float64
CANARY = -7.25e11
SPLIT_ROUTE = ["k_casale_generate_rows", "svgp_dgemm_batched", "svgp_dgemm_batched", "k_casale_generate_rowsum",
               "k_casale_generate"]
_CACHES = {}


def package_vae(p, L):
    from svgp_vae_amd.VAE_utils import mnistVAE
    vae = mnistVAE(L=L)
    vae.params = {k: p[k].clone() for k in vae.params}
    return vae


def build(variant):
    from svgp_vae_amd.generate import CasalePosteriorCache
    pr = CG.problem(variant)
    case = pr["case"]
    GP = CC.gp_object(case, ov_joint=True, normalize=pr["normalize"])
    return CasalePosteriorCache.from_latents(package_vae(pr["p"], pr["L"]), GP, case["aux"], CC.t64(case["Z"]))


def cache_of(variant):
    if variant not in _CACHES:
        _CACHES[variant] = build(variant)
    return _CACHES[variant]


def raw_generate(cache, aux, eps, gather, moments=True):
    """One svgp_casale_generate call of b = len(aux) rows with canaries behind every output.  Returns (images, mean, var)."""
    from svgp_vae_amd import _lib
    sh, dev = cache.shape, cache.device
    b, L = aux.shape[0], sh["L"]
    n_work = int(_lib.load_library().svgp_casale_generate_workspace_elems(C.byref(cache.cfg), b))
    buf = lambda n: torch.full((n + 64,), CANARY, dtype=DT, device=dev)
    work = buf(n_work) if n_work else None
    img, mean, var = buf(b * 784), buf(b * L), buf(b)
    d_aux = aux.to(dev).contiguous()
    d_eps = None if eps is None else eps.to(dev).contiguous()
    torch.cuda.synchronize()
    _lib.call("svgp_casale_generate", C.byref(cache.cfg), b, cache.theta.data_ptr(), cache.data.data_ptr(), d_aux.data_ptr(),
              int(gather), None if d_eps is None else d_eps.data_ptr(), img.data_ptr(), mean.data_ptr() if moments else None,
              var.data_ptr() if moments else None, None if work is None else work.data_ptr(), cache.stream.cuda_stream)
    cache.stream.synchronize()
    for t, n in ((img, b * 784), (mean, b * L), (var, b)) + (((work, n_work),) if n_work else ()):
        assert bool((t[n:] == CANARY).all()), "a canary behind an output was overwritten"
    if not moments:
        assert bool((mean == CANARY).all()) and bool((var == CANARY).all())
    return img[:b * 784].view(b, 28, 28, 1).cpu(), mean[:b * L].view(b, L).cpu(), var[:b].cpu()


# ---------------------------------------------------------------------------------------------- 1. the cache
@pytest.mark.parametrize("variant", list(CG.VARIANTS))
def test_cache_fields_match_float64_numpy(variant):
    pr, cf = CG.problem(variant), CG.cache_form(variant)
    cache, again = cache_of(variant), build(variant)
    assert torch.equal(cache.field("angles").cpu(), CC.t64(pr["case"]["angles"]))
    errs = {k: relerr(cache.field(k), cf[k]) for k in ("L_W", "U", "P")}
    print(f"{variant}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < CC.FWD_TOL for v in errs.values()), (variant, errs)
    P = cache.field("P")
    assert torch.equal(P, P.t()), "P is not symmetric bit for bit"
    assert torch.equal(cache.data, again.data), "two builds from the same latent rows differ"
    assert torch.equal(cache.theta[cache.wl.n_enc:cache.wl.n_vae].cpu(),
                       torch.cat([pr["p"][k].reshape(-1) for k in pr["p"] if k.startswith("dec_")]))


# ---------------------------------------------------------------------------------------------- 2. generation
@pytest.mark.parametrize("variant", list(CG.VARIANTS))
def test_generate_matches_the_literal_oracle(variant):
    from svgp_vae_amd import generate as G
    pr, ref = CG.problem(variant), CG.reference(variant)
    qaux, eps, cache = pr["qaux"], pr["eps"], cache_of(variant)
    assert G.route(cache) == (["k_casale_generate"] if pr["H"] <= 256 else SPLIT_ROUTE)
    img, mean, var = raw_generate(cache, qaux, eps, 1)
    errs = dict(mean=relerr(mean, ref["mean"]), var=relerr(var, ref["var"]), images=relerr(img, ref["images"]))
    print(f"{variant}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < CC.FWD_TOL for v in errs.values()), (variant, errs)
    # eps = NULL: the decode of the posterior mean; the moments are the same bits
    img0, mean0, var0 = raw_generate(cache, qaux, None, 1)
    e0 = relerr(img0, ref["images_mean"])
    print(f"{variant}: eps NULL images {e0:.2e}")
    assert e0 < CC.FWD_TOL and torch.equal(mean0, mean) and torch.equal(var0, var)
    # mean_out / var_out = NULL: the images keep their bits
    img1, _, _ = raw_generate(cache, qaux, eps, 1, moments=False)
    assert torch.equal(img1, img)
    # b = 1, and b = 300 (more images than one grid pass of workgroups, more rows than one pass of the split route): every copy
    # of a row gives the row's bits
    i1, m1, v1 = raw_generate(cache, qaux[:1], eps[:1], 1)
    assert torch.equal(i1, img[:1]) and torch.equal(m1, mean[:1]) and torch.equal(v1, var[:1])
    idx = torch.arange(300) % CG.N_QUERY
    ib, mb, vb = raw_generate(cache, qaux[idx], eps[idx], 1)
    assert torch.equal(ib, img[idx]) and torch.equal(mb, mean[idx]) and torch.equal(vb, var[idx])
    # a gathered row whose id is outside the table: NaN images and moments, no read outside it; the neighbours keep their bits
    bad = qaux.clone()
    bad[1, 0], bad[3, 0], bad[5, 0] = pr["n_obj"], -1.0, 1e15
    ibad, mbad, vbad = raw_generate(cache, bad, eps, 1)
    for r in range(CG.N_QUERY):
        if r in (1, 3, 5):
            assert torch.isnan(ibad[r]).all() and torch.isnan(mbad[r]).all() and torch.isnan(vbad[r]), r
        else:
            assert torch.equal(ibad[r], img[r]) and torch.equal(mbad[r], mean[r]) and torch.equal(vbad[r], var[r]), r
    # gather = 0 with the table's vector in the row (ids that are never looked up)
    own = qaux.clone()
    own[:, 0] = 1e15
    ig, mg, vg = raw_generate(cache, own, eps, 0)
    eg = dict(mean=relerr(mg, mean), var=relerr(vg, var), images=relerr(ig, img))
    print(f"{variant}: gather 0 against gather 1 " + "  ".join(f"{k} {v:.2e}" for k, v in eg.items()))
    assert all(v < CC.FWD_TOL for v in eg.values()), (variant, eg)
    # the Python entry: same bits as the raw call, moments of the stated shapes
    gi, gm, gv = G.generate(cache, qaux, eps=eps, return_moments=True)
    assert gm.shape == (CG.N_QUERY, pr["L"]) and gv.shape == (CG.N_QUERY,)
    assert torch.equal(gi.cpu(), img) and torch.equal(gm.cpu(), mean) and torch.equal(gv.cpu(), var)
    assert torch.equal(G.generate(cache, qaux).cpu(), img0)


def test_cache_save_load_round_trip(tmp_path):
    from svgp_vae_amd import generate as G
    cache, pr = cache_of("B-norm"), CG.problem("B-norm")
    path = str(tmp_path / "cache.pt")
    cache.save(path)
    back = G.CasalePosteriorCache.load(path)
    assert back.shape == cache.shape and torch.equal(back.data, cache.data) and torch.equal(back.theta, cache.theta)
    assert torch.equal(G.generate(back, pr["qaux"], eps=pr["eps"]), G.generate(cache, pr["qaux"], eps=pr["eps"]))
    with pytest.raises(ValueError, match="not a posterior cache file"):
        G.PosteriorCache.load(path)


# ---------------------------------------------------------------------------------------------- 3. chunked build
def test_build_in_chunks_equals_build_in_one_chunk():
    """The encoder kernel works one image per workgroup pass and nothing in it depends on the other rows of a call, so the
    chunking changes no bit of Z, and with it none of the cache: bit-equality is asserted, not the 1e-12 fallback."""
    from svgp_vae_amd.generate import CasalePosteriorCache
    prob = CC.real_problem(np.load(GOLDEN))
    N, L, p = prob["N"], prob["L"], prob["params"]
    assert N >= 18 and N % 5 != 0
    vae = package_vae(p, L)
    GP = CC.gp_object(prob, ov_joint=True, values=p)
    kw = dict(clip_qs=True, eps_full=prob["eps_f"])
    one = CasalePosteriorCache.build(vae, GP, prob["images"], prob["aux"], chunk=N, **kw)
    five = CasalePosteriorCache.build(vae, GP, prob["images"], prob["aux"], chunk=5, **kw)
    assert torch.equal(one.Z, five.Z) and torch.equal(one.data, five.data)
    mu, var = CC.O.MnistVAE(p, L).encode(prob["images"])
    CC.assert_clip_margin(var, 0, N)
    e = relerr(five.Z, mu + prob["eps_f"] * torch.sqrt(torch.clamp(var, 1e-3, 10)))
    print(f"Z of the chunked build against the oracle {e:.2e}")
    assert e < CC.FWD_TOL
    mean = CasalePosteriorCache.build(vae, GP, prob["images"], prob["aux"], chunk=5, clip_qs=True, latent="mean")
    assert relerr(mean.Z, mu) < CC.FWD_TOL and not torch.equal(mean.field("U"), five.field("U"))
    assert torch.equal(mean.field("P"), five.field("P"))           # P does not depend on the latent rows
    with pytest.raises(ValueError, match="latent"):
        CasalePosteriorCache.build(vae, GP, prob["images"], prob["aux"], latent="mode")


# ---------------------------------------------------------------------------------------------- 4. reference-executed fixture
@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "norm"])
def test_against_the_reference_executed_fixture(normalize):
    """generate(eps=None) on the fixture's test rows against the images the reference's own predict_test_set_Casale(take_mean=True)
    produced (tests/golden/ref_casale_small.npz)."""
    from svgp_vae_amd.generate import CasalePosteriorCache, generate
    from svgp_vae_amd.GPVAE_Casale_model import encode
    fx = np.load(os.path.join(os.path.dirname(GOLDEN), "ref_casale_small.npz"))
    tag = "norm" if normalize else "raw"
    prob = CC.fixture_problem(np.load(GOLDEN), normalize)
    vae = package_vae(prob["params"], prob["L"])
    GP = CC.gp_object(prob["case"], ov_joint=True, normalize=normalize)
    Z = encode(prob["images"].to("cuda:0"), vae, clipping_qs=True, epsilon=prob["eps_f"])
    cache = CasalePosteriorCache.from_latents(vae, GP, prob["aux"][:, :3], Z)
    e = relerr(generate(cache, prob["test_aux"]), fx[f"{tag}.predict.mean.recon"])
    print(f"fixture {tag}: images of the mean {e:.2e}")
    assert e < CC.FWD_TOL


# ---------------------------------------------------------------------------------------------- 5. engine
@pytest.mark.parametrize("ov_joint", [True, False], ids=["ovj", "ovfix"])
def test_engine_cache_agrees_with_the_engines_predict(ov_joint):
    from svgp_vae_amd.generate import generate
    prob = CC.real_problem(np.load(GOLDEN))
    N, L, p = prob["N"], prob["L"], prob["params"]
    eng = CC.step_engine(prob, batch_size=8, beta=0.7, clip=True, ov_joint=ov_joint)
    rng = np.random.RandomState(12)
    for lo, hi in ((4, 12), (16, N)):
        eng.step("joint", lo, hi, eps_full=CC.t64(rng.randn(N, L)), eps_batch=CC.t64(rng.randn(hi - lo, L)), adam=True)
    eng.synchronize()
    assert not torch.equal(eng.params["dec_d_w"].cpu(), p["dec_d_w"])           # the live parameters, not the initial ones
    T = 7
    ids = rng.randint(0, 6, T).astype(np.float64)
    ov = eng.params["object_vectors"].cpu().numpy()
    test_aux = CC.t64(np.concatenate([np.stack([ids, rng.uniform(0, 6.28, T)], 1), ov[ids.astype(int)]], 1))
    e_f = CC.t64(rng.randn(N, L))
    want, _ = eng.predict(prob["images"][:T].to(eng.dev), test_aux, take_mean=True, eps_full=e_f)
    cache = eng.posterior_cache(eps_full=e_f)
    assert cache.shape["ov_joint"] == int(ov_joint) and torch.equal(cache.theta, eng.theta)
    got = generate(cache, test_aux)                                  # gather defaults to the model's ov_joint
    e = relerr(got, want)
    print(f"ov_joint {ov_joint}: engine cache against engine predict {e:.2e}")
    assert e < CC.FWD_TOL
    assert relerr(generate(cache, test_aux, gather=not ov_joint), want) < CC.FWD_TOL     # the rows carry the table's vectors


# ---------------------------------------------------------------------------------------------- 6. driver and command line
def test_generate_cli_from_a_casale_driver_checkpoint(tmp_path):
    from svgp_vae_amd import MNIST_experiment
    from svgp_vae_amd import generate as G
    from svgp_vae_amd.GPVAE_Casale_model import _angles_mask, encode, predict_test_set_Casale
    g = np.load(GOLDEN)
    rng = np.random.RandomState(21)
    rows = rng.permutation(len(g["aux"]))
    tr, te = rows[:96], rows[96:108]
    data = str(tmp_path) + "/"
    pickle.dump(dict(images=g["images"][tr], aux_data=g["aux"][tr]), open(data + "train96.p", "wb"))
    pickle.dump(dict(images=g["images"][te], aux_data=g["aux"][te]), open(data + "test_data3.p", "wb"))
    L = 4
    log = MNIST_experiment.main(["--elbo", "GPVAE_Casale", "--opt_regime", "VAE-1", "GP-1", "joint-2", "--epsilon_seed", "0",
                                 "--save", "--save_model_weights", "--ov_joint", "--GP_joint", "--clip_qs", "--L", str(L),
                                 "--batch_size", "64", "--train_file", data + "train96.p", "--mnist_data_path", data,
                                 "--base_dir", data, "--eval_every", "2", "--seed", "0"])
    run = log["chkpnt_dir"]
    assert sorted(os.path.basename(f) for f in glob.glob(run + "model_*.pt")) == ["model_4.pt", "model_8.pt"]
    ck = run + "model_8.pt"
    # query rows: train objects at other angles, the table's row in the columns (not read: the run has --ov_joint)
    train = pickle.load(open(data + "train96.p", "rb"))
    vae, GP, a, train = G.casale_models_from_run(ck, train)
    assert a["elbo"] == "GPVAE_Casale" and GP.object_vectors.shape == (400, 8) and GP.ov_joint
    assert np.array_equal(train["aux_data"][:, 0], np.arange(96)) and np.all(np.diff(train["aux_data"][:, 1]) >= 0)
    ids = train["aux_data"][rng.randint(0, 96, 6), 1]
    q = np.concatenate([np.stack([ids, rng.uniform(0, 6.28, 6)], 1), GP.object_vectors[ids.astype(int)]], 1)
    np.save(data + "q.npy", q)
    out = data + "images.npy"
    G.main(["--checkpoint", ck, "--aux_file", data + "q.npy", "--latent_seed", "3", "--out", out])
    got = np.load(out)
    assert got.shape == (6, 28, 28, 1) and np.isfinite(got).all()
    # predict_test_set_Casale(take_mean=True) with the checkpoint's parameters and the same latent rows
    dev = torch.device("cuda:0")
    Z = encode(CC.t64(train["images"]).to(dev), vae, clipping_qs=True, epsilon=np.random.RandomState(3).randn(96, L))
    V = GP.V_matrix(train["aux_data"][:, :3], _angles_mask(train["aux_data"][:, 1:]))
    want, _ = predict_test_set_Casale(torch.zeros(6, 28, 28, 1, dtype=DT, device=dev), q, train["aux_data"][:, :3], vae, GP, V, Z,
                                      take_mean=True)
    e = relerr(got, want)
    print(f"command line against predict_test_set_Casale {e:.2e}")
    assert e < CC.FWD_TOL
    G.main(["--checkpoint", ck, "--ids", "0", "1", "--n_angles", "4", "--latent", "mean", "--out", out])
    sweep = np.load(out)
    assert sweep.shape == (8, 28, 28, 1) and np.isfinite(sweep).all() and float(np.abs(sweep[0] - sweep[1]).max()) > 0
    # a run whose args.json says SVGPVAE still goes down the SVGPVAE path: its loader answers for this theta
    import json
    args = json.load(open(run + "args.json"))
    args["elbo"] = "SVGPVAE_Hensman"
    os.makedirs(data + "other/")
    json.dump(args, open(data + "other/args.json", "wt"))
    torch.save(torch.load(ck), data + "other/model_8.pt")
    with pytest.raises(ValueError, match="fits no number of inducing points"):
        G.main(["--checkpoint", data + "other/model_8.pt", "--ids", "0", "--out", out])
