"""SPRITES posterior cache / animate on the GPU (svgp_vae_amd/animate.py, csrc/sprites_generate.hip): the one-launch GP entry
against einsum and against the oracle, the public `animate` against the oracle's prediction for a test character and against the
existing HIP prediction path, the cache file, and the command line on a checkpoint of the driver.  Cases, references and bars:
tests/animate_cases.py (their guards: tests/test_animate_cpu.py)."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import animate_cases as AC
from tests import helpers as H

pytestmark = pytest.mark.gpu
DT = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64                     # canary elements on both sides of every output


def _padded(n, value):
    """(whole buffer, the n-element window in its middle): every element of the buffer holds `value`."""
    buf = torch.full((n + 2 * PAD,), value, dtype=DT, device="cuda")
    return buf, buf[PAD:PAD + n]


def _canaries_intact(buf, n, value):
    return bool((buf[:PAD] == value).all()) and bool((buf[PAD + n:] == value).all())


def _posterior_rows(b, m, L, Kb, kbb, w, X, eps, want_z=True, clip=AC.CLIP):
    """One call of svgp_sprites_posterior_rows into canary-padded outputs; (p_m, p_v, z or None) as (b, L) clones."""
    from svgp_vae_amd import _lib
    lib = _lib.load_library()
    cfg = _lib.PosteriorRowsCfg(b=b, m=m, L=L, clip_lo=clip[0], clip_hi=clip[1])
    n_work = int(lib.svgp_sprites_posterior_rows_workspace_elems(C.byref(cfg)))
    assert 0 <= n_work <= 16 * b * L
    bufs = {k: _padded(b * L, v) for k, v in (("p_m", -7.25), ("p_v", -8.5), ("z", -9.75))}
    wbuf, work = _padded(n_work, -3.5)
    guard_before = {k: v[0].clone() for k, v in bufs.items()}
    s = torch.cuda.current_stream().cuda_stream
    _lib.call("svgp_sprites_posterior_rows", C.byref(cfg), Kb.data_ptr(), kbb.data_ptr(), w.data_ptr(), X.data_ptr(),
              None if eps is None else eps.data_ptr(), bufs["p_m"][1].data_ptr(), bufs["p_v"][1].data_ptr(),
              bufs["z"][1].data_ptr() if want_z else None, work.data_ptr() if n_work else None, s)
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert _canaries_intact(buf, b * L, float(guard_before[k][0])), f"{k}: written outside its {b} x {L} elements"
    assert _canaries_intact(wbuf, n_work, -3.5), "work: written outside its elements"
    if not want_z:
        assert torch.equal(bufs["z"][0], guard_before["z"]), "z = NULL but the buffer next to it changed"
    out = [bufs[k][1].clone().view(b, L) for k in ("p_m", "p_v")]
    return out[0], out[1], (bufs["z"][1].clone().view(b, L) if want_z else None)


# ---------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("case", AC.KERNEL_IDS)
def test_posterior_rows_against_einsum(case):
    b, m, L = AC.kernel_shape(case)
    p = AC.kernel_problem(case)
    d = {k: torch.tensor(v, dtype=DT, device="cuda").contiguous() for k, v in p.items()}
    pm_ref, pv_ref, z_ref, _ = AC.kernel_reference(case)
    args = (b, m, L, d["Kb"], d["kbb"], d["w"], d["X"])
    p_m, p_v, z = _posterior_rows(*args, d["eps"])
    for name, got, ref in (("p_m", p_m, pm_ref), ("p_v", p_v, pv_ref), ("z", z, z_ref)):
        e = H.relerr(got, ref)
        print(f"{case} {name}: {e:.2e}")
        assert e < AC.PATH_TOL, (case, name, e)
    if case == AC.CLAMP_CASE:
        assert float(p_v.min()) == AC.CLIP[0] and float(p_v.max()) == AC.CLIP[1]
    # two calls agree bit for bit
    p_m2, p_v2, z2 = _posterior_rows(*args, d["eps"])
    assert torch.equal(p_m, p_m2) and torch.equal(p_v, p_v2) and torch.equal(z, z2)
    # eps = NULL: z is the posterior mean, bit for bit; z = NULL: the moments alone, the same bits
    p_m3, p_v3, z3 = _posterior_rows(*args, None)
    assert torch.equal(z3, p_m3) and torch.equal(p_m3, p_m) and torch.equal(p_v3, p_v)
    p_m4, p_v4, z4 = _posterior_rows(*args, d["eps"], want_z=False)
    assert z4 is None and torch.equal(p_m4, p_m) and torch.equal(p_v4, p_v)


def test_posterior_rows_takes_x_as_written_and_keeps_a_nan():
    """X is read element for element: with its strict upper triangle zeroed the result follows (a kernel that mirrored one
    triangle could not tell the two apart); a NaN in p_v goes through the clamp (torch.clamp) into that row alone."""
    case = "33-17-3"
    b, m, L = AC.kernel_shape(case)
    d = {k: torch.tensor(v, dtype=DT, device="cuda").contiguous() for k, v in AC.kernel_problem(case).items()}
    wide = (-1e300, 1e300)
    _, pv, _ = _posterior_rows(b, m, L, d["Kb"], d["kbb"], d["w"], d["X"], None, clip=wide)
    Xl = torch.tril(d["X"]).contiguous()
    _, pv_l, _ = _posterior_rows(b, m, L, d["Kb"], d["kbb"], d["w"], Xl, None, clip=wide)
    ref_l = d["kbb"][:, None] + torch.einsum("bi,lij,bj->bl", d["Kb"], Xl, d["Kb"])
    assert H.relerr(pv_l, ref_l) < AC.PATH_TOL and H.relerr(pv_l, pv) > 1e-3
    kbb = d["kbb"].clone()
    kbb[3] = float("nan")
    _, pv_n, z_n = _posterior_rows(b, m, L, d["Kb"], kbb, d["w"], d["X"], d["eps"])
    assert bool(torch.isnan(pv_n[3]).all()) and bool(torch.isnan(z_n[3]).all())
    assert bool(torch.isfinite(pv_n[:3]).all()) and bool(torch.isfinite(pv_n[4:]).all())


# ---------------------------------------------------------------------------------------------- 2. the stage
def _stage_engine(case, p):
    from svgp_vae_amd import sprites as S
    m, L, _, q, K_SE = AC.STAGE_CASES[case]
    svgp = S.spritesSVGP(False, True, p["ip"].numpy(), "main", 0.01, float(p["aux"].shape[0]), AC.LA, p["table"].numpy(), AC.LC, L,
                         K_obj_normalize=not K_SE, K_SE=K_SE)
    eng = S.SpritesStepEngine(S.spritesVAE(L), S.sprites_representation_network(AC.LC), svgp, b_max=max(q, 1), seg_len=1,
                              params=dict(se=torch.tensor(AC.SE, dtype=DT)))
    svgp._engine = eng
    return svgp, eng


@pytest.mark.parametrize("case", list(AC.STAGE_CASES))
def test_kernel_matrix_then_posterior_rows_against_the_oracle(case):
    from svgp_vae_amd import sprites as S
    m, L, _, q, K_SE = AC.STAGE_CASES[case]
    p, ref = AC.stage_problem(case), AC.stage_reference(case)
    svgp, eng = _stage_engine(case, p)
    dev = eng.dev
    _, Kb, kbb = eng.kernel_matrices(p["qaux"].to(dev))                    # svgp_sprites_kernel_matrix_fwd
    w, Si, Ki = ref["w"].to(dev).contiguous(), ref["Si"].to(dev).contiguous(), ref["Ki"].to(dev).contiguous()
    X = (Si - Ki[None]).contiguous()
    p_m, p_v, z = _posterior_rows(q, m, L, Kb, kbb, w, X, p["eps"].to(dev).contiguous())
    for name, got in (("p_m", p_m), ("p_v", p_v), ("z", z)):
        e = H.relerr(got, ref[name])
        print(f"{case} {name}: against the oracle {e:.2e}")
        assert e < AC.TOL, (case, name, e)
    # the same inputs through the existing path (batched GEMM into (L, b, m), row sums, clamp in torch)
    mean, B = S.approximate_posterior_params_precomputed_GP_posterior_params(svgp, p["qaux"].to(dev), w, Si, Ki, engine=eng)
    torch.cuda.synchronize()
    e_m, e_v = H.relerr(p_m, mean), H.relerr(p_v, torch.clamp(B, *AC.CLIP))
    print(f"{case}: against the existing path p_m {e_m:.2e}, p_v {e_v:.2e}")
    assert e_m < AC.PATH_TOL and e_v < AC.PATH_TOL


# ---------------------------------------------------------------------------------------------- 3. end to end
def _pipeline_engine(P, b_max=20):
    from svgp_vae_amd import sprites as S
    gp = P["gp"]
    vae, rnn = S.spritesVAE(P["L"]), S.sprites_representation_network(P["Lc"])
    svgp = S.spritesSVGP(False, False, gp["inducing_index_points"].numpy(), 'main', 0.01, float(P["n_train"]), P["La"],
                         gp["GPLVM_action"].numpy(), P["Lc"], P["L"], K_obj_normalize=not P["K_SE"], K_SE=P["K_SE"])
    init = dict(P["params"])
    init["se"] = torch.stack([gp["l_action"], gp["sigma_action"], gp["l_character"], gp["sigma_character"]])
    eng = S.SpritesStepEngine(vae, rnn, svgp, b_max=b_max, seg_len=1, clip_qs=True, params=init)   # b_max < n_train: chunked
    S._attach(eng, svgp, vae, rnn)
    return vae, rnn, svgp, eng


def _shape_of(P):
    return dict(L=P["L"], L_action=P["La"], L_character=P["Lc"], m=P["m"], n_act=P["n_act"], K_SE=P["K_SE"], normalize=not P["K_SE"],
                jitter=0.01, N_train=float(P["n_train"]), clip_qs=True, net_dtype="float64")


@pytest.mark.parametrize("K_SE", [True, False])
def test_animate_reproduces_the_test_character_prediction(K_SE, tmp_path):
    from svgp_vae_amd import animate as A
    from svgp_vae_amd import sprites as S
    P = AC.pipeline(K_SE)
    vae, rnn, svgp, eng = _pipeline_engine(P)
    na, nc, L = P["N_actions"], P["N_context"], P["L"]
    ctx = P["test_frames"].view(-1, na, 64, 64, 3)[:, :nc]
    acts = P["test_ids"].view(-1, na)[:, nc:]
    n_char, T = acts.shape
    # (a) the oracle's terms loaded into the cache: float64-exact
    exact = A.SpritesPosteriorCache(_shape_of(P), eng.theta.clone(), P["mt_o"], P["inv_o"] - P["Kmm_inv"][None], device=eng.dev,
                                    engine=eng)
    fr, p_m, p_v = A.animate(exact, ctx, acts, eps=P["eps"], return_moments=True)
    assert tuple(fr.shape) == (n_char, T, 64, 64, 3) and tuple(p_m.shape) == (n_char * T, L)
    errs = dict(frames=H.relerr(fr.reshape(-1, 64, 64, 3), P["rec_o"]), p_m=H.relerr(p_m, P["pm_o"]), p_v=H.relerr(p_v, P["pv_o"]))
    print(f"K_SE={K_SE} animate against the oracle: {errs}")
    assert max(errs.values()) < AC.TOL, errs
    # (b) eps = None: the decode of the posterior mean
    fr_mean = A.animate(exact, ctx, acts)
    assert H.relerr(fr_mean.reshape(-1, 64, 64, 3), P["rec_mean_o"]) < AC.TOL
    # (c) the existing HIP prediction path, same terms and draw
    rec2, _, _ = S.predict_SVGPVAE_sprites_test_character((P["test_frames"], P["test_ids"]), vae, svgp, rnn, P["mt_o"], P["inv_o"],
                                                          nc, na, P["bt"], P["cseg"], P["crep"], P["Kmm_inv"], epsilon=P["eps"],
                                                          engine=eng)
    e = H.relerr(fr.reshape(-1, 64, 64, 3), rec2)
    print(f"K_SE={K_SE} animate against the existing HIP path: {e:.2e}")
    assert e < AC.PATH_TOL
    # (d) one character, one context frame, T = 4 targets (the train segments have 8 frames)
    ctx1, acts1, rec1_o, pm1_o, pv1_o = AC.pipeline_single(K_SE)
    fr1, pm1, pv1 = A.animate(exact, ctx1, acts1, return_moments=True)
    assert tuple(fr1.shape) == (1, 4, 64, 64, 3)
    assert max(H.relerr(fr1[0], rec1_o), H.relerr(pm1, pm1_o), H.relerr(pv1, pv1_o)) < AC.TOL
    # (e) the cache built from the train set (float32 streaming statistics: the bar of test_sprites_test_character_pipeline)
    built = A.SpritesPosteriorCache.build(vae, rnn, svgp, P["frames"], P["ids"], frames_per_character=P["fpc"], chunk=2 * P["fpc"],
                                          clip_qs=True, engine=eng)
    assert built.shape == exact.shape and torch.equal(built.theta, eng.theta)
    fr_b = A.animate(built, ctx, acts, eps=P["eps"])
    e_b = H.relerr(fr_b.reshape(-1, 64, 64, 3), P["rec_o"])
    print(f"K_SE={K_SE} animate on the built cache against the oracle: {e_b:.2e}")
    assert e_b < 2e-3
    # ---- 4. the cache: chunk = one group against all rows; save -> load -> animate
    one = A.SpritesPosteriorCache.build(vae, rnn, svgp, P["frames"], P["ids"], frames_per_character=P["fpc"], chunk=P["fpc"],
                                        clip_qs=True, engine=eng)
    full = A.SpritesPosteriorCache.build(vae, rnn, svgp, P["frames"], P["ids"], frames_per_character=P["fpc"], chunk=P["n_train"],
                                         clip_qs=True, engine=eng)
    e_w, e_X = H.relerr(one.w, full.w), H.relerr(one.X, full.X)
    print(f"K_SE={K_SE} chunk = one group against all rows: w {e_w:.2e}, X {e_X:.2e}")
    assert e_w < AC.PATH_TOL and e_X < AC.PATH_TOL
    path = str(tmp_path / "cache.pt")
    built.save(path)
    loaded = A.SpritesPosteriorCache.load(path)
    assert loaded._engine is None and torch.equal(loaded.w, built.w) and torch.equal(loaded.X, built.X)
    state = torch.cuda.get_rng_state()
    fr_l = A.animate(loaded, ctx, acts, eps=P["eps"])                    # on an engine the cache builds from theta
    assert torch.equal(fr_l, fr_b)
    assert torch.equal(torch.cuda.get_rng_state(), state)                 # no random-number state touched
    with pytest.raises(ValueError):
        A.animate(exact, ctx, acts + P["n_act"])
    with pytest.raises(ValueError):
        A.SpritesPosteriorCache.build(vae, rnn, svgp, P["frames"], P["ids"], frames_per_character=P["fpc"], chunk=P["fpc"] + 1,
                                      clip_qs=True, engine=eng)


# ---------------------------------------------------------------------------------------------- 5. from a run of the driver
def test_cli_animates_from_a_checkpoint_of_the_driver(tmp_path):
    from svgp_vae_amd import SPRITES_experiment as E
    from svgp_vae_amd import animate as A
    # (--elbo, --batch_size_test_char 16 and --N_context 3: without them the driver refuses 2 test characters of 8 actions)
    args = E.build_parser().parse_args(
        ["--elbo", "SVGPVAE_Hensman", "--synthetic", "6,2", "--N_actions", "8", "--frames_per_character", "5", "--batch_size", "10",
         "--batch_size_test_char", "16", "--N_context", "3", "--L", "8", "--m", "2", "--K_SE", "--opt_regime", "joint-2",
         "--eval_every", "2", "--save", "--save_model_weights", "--base_dir", str(tmp_path)])
    log = E.run_experiment_sprites_SVGPVAE(args)
    ckpt = glob.glob(str(tmp_path) + "/debug_SPRITES/*/model_1.pt")
    assert len(ckpt) == 1
    ckpt = ckpt[0]
    a = A.run_args_of(ckpt)
    train, test = A.load_run_data(a)
    shape = A.shape_from_run(a, len(train["frames"]))
    assert shape["m"] == 16 and shape["n_act"] == 8 and shape["L"] == 8 and shape["K_SE"] and not shape["clip_qs"]
    theta = A.theta_from_run(ckpt, shape)
    assert torch.equal(theta, log["_engine"].theta.cpu())
    assert list(A.param_shapes(shape)) == list(log["_engine"].shapes)
    # the command line in a fresh process
    out, cache_file = str(tmp_path / "frames.npy"), str(tmp_path / "cache.pt")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "svgp_vae_amd.animate", "--checkpoint", ckpt, "--synthetic", "--characters", "1", "0",
           "--N_context", "3", "--sample", "--seed", "4", "--save_cache", cache_file, "--out", out]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "route: k_sprites_posterior_rows" in r.stdout
    got = np.load(out)
    assert got.shape == (2, 5, 64, 64, 3) and np.isfinite(got).all() and got.min() > -1.5 and got.max() < 2.5
    # the same in process, on a cache built from the same checkpoint
    cache = A.cache_from_run(ckpt, train, a)
    fr = np.asarray(test["frames"], dtype=np.float64).reshape(2, 8, 64, 64, 3)
    ids = np.asarray(test["action_IDs"]).reshape(2, 8)
    eps = np.random.RandomState(4).randn(10, 8)
    mine = A.animate(cache, fr[[1, 0], :3], ids[[1, 0], 3:], eps=eps)
    assert np.array_equal(mine.cpu().numpy(), got)
    # ... and from the cache file the command line wrote
    loaded = A.SpritesPosteriorCache.load(cache_file)
    assert torch.equal(loaded.w, cache.w) and torch.equal(loaded.X, cache.X) and torch.equal(loaded.theta, cache.theta)
    out2 = str(tmp_path / "frames2.npy")
    r = subprocess.run(cmd[:5] + ["--cache", cache_file, "--characters", "1", "0", "--N_context", "3", "--sample", "--seed", "4",
                                  "--out", out2], cwd=ROOT, env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.load(out2), got)
