"""Posterior cache, one-launch conditional generation, the generate CLI and --restore on the GPU, against the float64 oracle
(tests/generate_cases.py has the cases, the reference and the bars; tests/test_generate_cpu.py the guard that makes the bars
meaningful)."""
import ctypes as C
import glob
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import generate_cases as GC
from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = torch.float64
CANARY = -7.25e11
_MODELS, _CACHES = {}, {}


def models(case):
    """(vae, svgp) of the package at the case's parameters (one pair per case: the existing predict path binds an engine to it)."""
    if case not in _MODELS:
        from svgp_vae_amd.SVGPVAE_model import mnistSVGP
        from svgp_vae_amd.VAE_utils import mnistVAE
        cs, params = GC.CASES[case], GC.problem(case)[0]
        vae = mnistVAE(L=cs["L"])
        vae.params = {k: params[k].clone() for k in vae.params}
        ov = params["object_vectors"].numpy() if cs["table"] else None
        svgp = mnistSVGP(False, False, params["inducing_index_points"].numpy(), False, ov, "main", GC.JITTER, float(cs["rows"]), cs["L"])
        svgp.l_GP, svgp.amplitude = params["l_GP"].clone(), params["amplitude"].clone()
        _MODELS[case] = (vae, svgp)
    return _MODELS[case]


def build(case, chunk):
    from svgp_vae_amd.generate import PosteriorCache
    _, img, aux, _, _ = GC.problem(case)
    vae, svgp = models(case)
    return PosteriorCache.build(vae, svgp, img, aux, chunk=chunk, clip_qs=True)


def cache_of(case):
    if case not in _CACHES:
        _CACHES[case] = build(case, GC.CASES[case]["rows"])
    return _CACHES[case]


def raw_generate(cache, aux, eps, gather, moments=True):
    """One svgp_mnist_generate call of b = len(aux) rows with canaries behind every output.  Returns (images, p_m, p_v)."""
    from svgp_vae_amd import _lib
    from svgp_vae_amd.generate import _cfg
    sh, dev = cache.shape, cache.device
    b, L = aux.shape[0], sh["L"]
    cfg = _cfg(sh, b, b)
    n_work = int(_lib.load_library().svgp_mnist_generate_workspace_elems(C.byref(cfg)))
    work = torch.empty(n_work, dtype=DT, device=dev) if n_work else None
    buf = lambda n: torch.full((n + 64,), CANARY, dtype=DT, device=dev)
    img, pm, pv = buf(b * 784), buf(b * L), buf(b * L)
    d_aux = aux.to(dev).contiguous()
    d_eps = None if eps is None else eps.to(dev).contiguous()
    torch.cuda.synchronize()
    _lib.call("svgp_mnist_generate", C.byref(cfg), cache.theta.data_ptr(), cache.data.data_ptr(), d_aux.data_ptr(), int(gather),
              None if d_eps is None else d_eps.data_ptr(), img.data_ptr(), pm.data_ptr() if moments else None,
              pv.data_ptr() if moments else None, None if work is None else work.data_ptr(), cache.stream.cuda_stream)
    cache.stream.synchronize()
    for t, n in ((img, b * 784), (pm, b * L), (pv, b * L)):
        assert bool((t[n:] == CANARY).all()), "a canary behind an output was overwritten"
    if not moments:
        assert bool((pm == CANARY).all()) and bool((pv == CANARY).all())
    return img[:b * 784].view(b, 28, 28, 1).cpu(), pm[:b * L].view(b, L).cpu(), pv[:b * L].view(b, L).cpu()


@pytest.mark.parametrize("case", list(GC.CASES))
def test_cache_matches_the_oracle_in_one_chunk_and_in_ragged_chunks(case):
    cs, ref = GC.CASES[case], GC.reference(case)
    one, ragged, again = cache_of(case), build(case, 16), build(case, 16)
    assert cs["rows"] % 16 in (5, 6)
    for name, c in (("one chunk", one), ("chunks of 16", ragged)):
        ew, eX = H.relerr(c.field("w"), ref["w"]), H.relerr(c.field("X"), ref["X"])
        print(f"{case} {name}: w {ew:.2e}  X {eX:.2e}")
        assert ew < GC.TOL and eX < GC.TOL, (case, name, ew, eX)
        X = c.field("X")
        assert torch.equal(X, X.transpose(1, 2)), "X is not symmetric bit for bit"
        assert float(c.field("acc_rows")[0]) == cs["rows"]
    e = max(H.relerr(ragged.field(k), one.field(k)) for k in ("w", "X"))
    print(f"{case}: chunks of 16 against one chunk {e:.2e}")
    assert e < GC.PATH_TOL
    assert torch.equal(ragged.data, again.data), "two builds with the same chunking differ"


@pytest.mark.parametrize("case", list(GC.CASES))
def test_generate_matches_the_oracle(case):
    cs, ref = GC.CASES[case], GC.reference(case)
    _, _, _, qaux, eps = GC.problem(case)
    cache, gather = cache_of(case), cs["table"]
    img, pm, pv = raw_generate(cache, qaux, eps, gather)
    errs = dict(p_m=H.relerr(pm, ref["p_m"]), p_v=H.relerr(pv, ref["p_v"]), images=H.relerr(img, ref["images"]))
    print(f"{case}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < GC.TOL for v in errs.values()), (case, errs)
    # eps = NULL: the decode of the posterior mean; the moments are the same bits
    img0, pm0, pv0 = raw_generate(cache, qaux, None, gather)
    e0 = H.relerr(img0, ref["images_mean"])
    print(f"{case}: eps NULL images {e0:.2e}")
    assert e0 < GC.TOL and torch.equal(pm0, pm) and torch.equal(pv0, pv)
    # p_m_out / p_v_out = NULL: the images keep their bits
    img1, _, _ = raw_generate(cache, qaux, eps, gather, moments=False)
    assert torch.equal(img1, img)
    # b = 1, and b = 300 (more images than one grid pass of workgroups): every copy of a row gives the row's bits
    i1, m1, v1 = raw_generate(cache, qaux[:1], eps[:1], gather)
    assert torch.equal(i1, img[:1]) and torch.equal(m1, pm[:1]) and torch.equal(v1, pv[:1])
    idx = torch.arange(300) % cs["q"]
    ib, mb, vb = raw_generate(cache, qaux[idx], eps[idx], gather)
    assert torch.equal(ib, img[idx]) and torch.equal(mb, pm[idx]) and torch.equal(vb, pv[idx])


@pytest.mark.parametrize("case", ["B", "D", "E"])
def test_an_id_outside_the_table_gives_nan_rows_and_no_read_outside_it(case):
    """The C entry point on its own (no host check): a gathered row whose id is n_obj, -1 or far outside gets NaN images and
    moments on both routes (B, D: the fused launch; E: the GEMM route); the other rows keep their bits."""
    cs = GC.CASES[case]
    _, _, _, qaux, eps = GC.problem(case)
    cache = cache_of(case)
    img, pm, pv = raw_generate(cache, qaux, eps, True)
    bad = qaux.clone()
    bad[1, 0], bad[3, 0], bad[4, 0] = cs["n_obj"], -1.0, 1e15
    ib, mb, vb = raw_generate(cache, bad, eps, True)
    for r in range(cs["q"]):
        if r in (1, 3, 4):
            assert torch.isnan(ib[r]).all() and torch.isnan(mb[r]).all() and torch.isnan(vb[r]).all(), r
        else:
            assert torch.equal(ib[r], img[r]) and torch.equal(mb[r], pm[r]) and torch.equal(vb[r], pv[r]), r


@pytest.mark.parametrize("case", ["C", "E"])
def test_generate_agrees_with_the_existing_predict_path_and_leaves_the_state_alone(case):
    from svgp_vae_amd.generate import generate
    from svgp_vae_amd.SVGPVAE_model import bacthing_predict_SVGPVAE_rotated_mnist, batching_encode_SVGPVAE
    cs = GC.CASES[case]
    _, img, aux, qaux, eps = GC.problem(case)
    vae, svgp = models(case)
    cache = cache_of(case)
    mu, var, _ = batching_encode_SVGPVAE((img, aux), vae, clipping_qs=True)
    recon, _ = bacthing_predict_SVGPVAE_rotated_mnist((torch.zeros(cs["q"], 28, 28, 1, dtype=DT), qaux), vae, svgp, mu, var, aux,
                                                      epsilon=eps)
    eng = svgp._rt.eng
    eng.synchronize()
    state = eng.state.clone()
    got, p_m, p_v = generate(cache, qaux, eps=eps, return_moments=True)
    eng.synchronize()
    assert torch.equal(eng.state, state)
    e = dict(images=H.relerr(got, recon), p_m=H.relerr(p_m, eng.ws_view("p_m", (cs["q"], cs["L"]))),
             p_v=H.relerr(p_v, eng.ws_view("p_v", (cs["q"], cs["L"]))))
    print(f"{case}: against bacthing_predict_SVGPVAE_rotated_mnist " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert all(v < GC.PATH_TOL for v in e.values()), (case, e)


@pytest.mark.parametrize("case", ["B", "F", "E"])
def test_generate_in_capacity_batches_equals_row_wise_calls(case):
    """2.5 capacity batches of rows: m <= 64 (B, F) is one launch for all of them, E goes through calls of GEN_ROWS rows."""
    from svgp_vae_amd import generate as G
    cs = GC.CASES[case]
    _, _, _, qaux, eps = GC.problem(case)
    cache = cache_of(case)
    n = 2 * G.GEN_ROWS + G.GEN_ROWS // 2
    idx = torch.arange(n) % cs["q"]
    aux, ep = qaux[idx].clone(), eps[idx].clone()
    aux[:, 1] += torch.arange(n, dtype=DT) * 0.01                  # every row its own angle
    img, pm, pv = G.generate(cache, aux, eps=ep, gather=cs["table"], return_moments=True)
    assert img.shape == (n, 28, 28, 1) and pm.shape == pv.shape == (n, cs["L"])
    for r in range(n):
        i1, m1, v1 = G.generate(cache, aux[r:r + 1], eps=ep[r:r + 1], gather=cs["table"], return_moments=True)
        assert torch.equal(i1[0], img[r]) and torch.equal(m1[0], pm[r]) and torch.equal(v1[0], pv[r]), r
    assert torch.equal(G.generate(cache, aux[:3], gather=cs["table"]), G.generate(cache, aux, gather=cs["table"])[:3])
    if cs["table"]:
        bad = aux[:2].clone()
        bad[1, 0] = cs["n_obj"]
        with pytest.raises(ValueError):
            G.generate(cache, bad)
    else:
        with pytest.raises(ValueError):
            G.generate(cache, aux[:2], gather=True)


def test_cache_save_load_round_trip(tmp_path):
    from svgp_vae_amd import generate as G
    cache = cache_of("C")
    path = str(tmp_path / "cache.pt")
    cache.save(path)
    back = G.PosteriorCache.load(path)
    assert back.shape == cache.shape and torch.equal(back.data, cache.data) and torch.equal(back.theta, cache.theta)
    _, _, _, qaux, eps = GC.problem("C")
    assert torch.equal(G.generate(back, qaux, eps=eps), G.generate(cache, qaux, eps=eps))
    assert G.route(back) == ["k_generate"]


# ---------------------------------------------------------------------------------------------- driver: CLI and --restore
def _split(golden, tmp_path):
    gin, _ = golden
    d = str(tmp_path) + "/"
    for name, sl in (("train_data3.p", slice(0, 512)), ("eval_data3.p", slice(512, 576)), ("test_data3.p", slice(576, 640))):
        pickle.dump({"images": gin["images"][sl], "aux_data": gin["aux"][sl]}, open(d + name, "wb"))
    pickle.dump(gin["object_vectors"], open(d + "pca_ov_init3.p", "wb"))
    return d


def _drive(d, expid, extra):
    from svgp_vae_amd import MNIST_experiment as E
    argv = ["--elbo", "SVGPVAE_Hensman", "--mnist_data_path", d, "--train_file", d + "train_data3.p", "--PCA", "--base_dir", d,
            "--expid", expid, "--eval_every", "2", "--save", "--save_model_weights"] + extra
    log = E.run_experiment_rotated_mnist_SVGPVAE(E.build_parser().parse_args(argv))
    (run,) = glob.glob(d + expid + "/*/")
    assert os.path.samefile(run, log["chkpnt_dir"])
    return log, run


def test_generate_cli_from_a_driver_checkpoint(golden, tmp_path):
    from svgp_vae_amd import generate as G
    d = _split(golden, tmp_path)
    _, run = _drive(d, "cli", ["--ip_joint", "--GP_joint", "--ov_joint", "--clip_qs", "--GECO", "--opt_regime", "joint-2"])
    ck, out = run + "model_1.pt", d + "images.npy"
    assert os.path.exists(ck)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    # (no --mnist_data_path: the run's own, from its args.json)
    r = subprocess.run([sys.executable, "-m", "svgp_vae_amd.generate", "--checkpoint", ck, "--ids", "0", "1", "2", "--n_angles", "5",
                        "--out", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "k_generate" in r.stdout
    got = np.load(out)
    assert got.shape == (15, 28, 28, 1) and np.isfinite(got).all()
    train = pickle.load(open(d + "train_data3.p", "rb"))
    img, aux = torch.as_tensor(train["images"], dtype=DT), torch.as_tensor(train["aux_data"], dtype=DT)
    vae, svgp, a = G.models_from_run(ck, aux, d)
    assert svgp.nr_inducing == 32 and svgp.N_train == 512.0 and svgp.object_vectors.shape == (400, 8)
    cache = G.PosteriorCache.build(vae, svgp, img, aux, clip_qs=True)
    mine = G.generate(cache, G.rotation_sweep([0, 1, 2], 5, 8))
    assert np.array_equal(mine.cpu().numpy(), got)
    assert float(np.abs(got[0] - got[1]).max()) > 0                # the angle matters


def test_restore_resumes_the_uninterrupted_run_bit_for_bit(golden, tmp_path):
    from svgp_vae_amd import checkpoint
    d = _split(golden, tmp_path)
    flags = ["--GECO", "--clip_qs", "--ip_joint", "--GP_joint", "--ov_joint", "--epsilon_seed", "3", "--opt_regime", "joint-4"]
    full, run_full = _drive(d, "full", flags)
    assert full["epoch"] == [0, 1, 2, 3] and os.path.exists(run_full + "model_1.pt")
    tail, run_tail = _drive(d, "tail", flags + ["--restore", run_full + "model_1.pt"])
    assert tail["epoch"] == [2, 3]
    assert [e for e, _ in tail["cgen_mse"]] == [3] and not os.path.exists(run_tail + "model_1.pt")
    a, b = checkpoint.load(run_full + "model_3.pt"), checkpoint.load(run_tail + "model_3.pt")
    for k in ("theta", "adam_m", "adam_v", "state"):
        n_diff = int((a[k] != b[k]).sum())
        print(f"{k}: {n_diff} of {a[k].numel()} elements differ, max |diff| {float((a[k] - b[k]).abs().max()):.3e}")
        assert torch.equal(a[k], b[k]), k
    assert full["steps"][4:] == tail["steps"]
    assert full["cgen_mse"][-1] == tail["cgen_mse"][-1] and full["eval_mse"][-1] == tail["eval_mse"][-1]
    with pytest.raises(ValueError) as e:
        _drive(d, "other", flags + ["--restore", run_full + "model_1.pt", "--nr_inducing_points", "1"])
    n_file = a["theta"].numel()
    assert str(n_file) in str(e.value) and str(n_file - 16 * 10) in str(e.value)
