"""SPRITES posterior cache / animate: everything that needs no GPU.  The C ABI's declarations, exports, refusals, workspace and
launch route; the guards that make the bars of tests/animate_cases.py meaningful; the cache file format on CPU tensors; the
command line's parser."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import svgp_vae_amd
from svgp_vae_amd import _lib
from svgp_vae_amd._lib import PosteriorRowsCfg
from tests import animate_cases as AC
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("svgp_sprites_posterior_rows_workspace_elems", "svgp_sprites_posterior_rows", "svgp_sprites_posterior_rows_route")
FAKE = 4096                         # never dereferenced: every call below fails validation first
SHAPE = dict(L=2, L_action=8, L_character=16, m=3, n_act=9, K_SE=True, normalize=False, jitter=0.01, N_train=48.0, clip_qs=True,
             net_dtype="float64")


def _cfg(b=4, m=12, L=3, lo=AC.CLIP[0], hi=AC.CLIP[1]):
    return PosteriorRowsCfg(b=b, m=m, L=L, clip_lo=lo, clip_hi=hi)


def _rows(q, Kb=FAKE, kbb=FAKE, w=FAKE, X=FAKE, p_m=FAKE, p_v=FAKE):
    return _lib.call("svgp_sprites_posterior_rows", None if q is None else C.byref(q), Kb, kbb, w, X, None, p_m, p_v, None, None, None)


def _route(q):
    buf = C.create_string_buffer(256)
    _lib.call("svgp_sprites_posterior_rows_route", C.byref(q), buf, len(buf))
    return buf.value.decode().split()


def test_header_declares_library_exports_and_binding_covers_the_new_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svgpvae_hip.h")).read(), flags=re.S)
    lib = svgp_vae_amd.load_library()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", src), f"{n} not declared in include/svgpvae_hip.h"
        assert hasattr(lib, n), f"{n} not exported"
        assert n in _lib.SIGNATURES or n in _lib.NON_STATUS
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*svgp_posterior_rows_cfg\s*;", src, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "int32_t b, m, L; double clip_lo, clip_hi;"
    assert [n for n, _ in PosteriorRowsCfg._fields_] == ["b", "m", "L", "clip_lo", "clip_hi"] and C.sizeof(PosteriorRowsCfg) == 32


@pytest.mark.parametrize("call,message", [
    (lambda: _rows(_cfg(m=0)), "m=0"), (lambda: _rows(_cfg(m=2049)), "m=2049"), (lambda: _rows(_cfg(L=65)), "L=65"),
    (lambda: _rows(_cfg(L=0)), "L=0"), (lambda: _rows(_cfg(b=0)), "b=0"), (lambda: _rows(None), "cfg is NULL"),
    (lambda: _rows(_cfg(lo=2.0, hi=1.0)), "clip_lo <= clip_hi"),
    (lambda: _rows(_cfg(), Kb=None), "NULL device pointer"), (lambda: _rows(_cfg(), kbb=None), "NULL device pointer"),
    (lambda: _rows(_cfg(), w=None), "NULL device pointer"), (lambda: _rows(_cfg(), X=None), "NULL device pointer"),
    (lambda: _rows(_cfg(), p_m=None), "NULL device pointer"), (lambda: _rows(_cfg(), p_v=None), "NULL device pointer"),
    (lambda: _route(_cfg(m=2049)), "m=2049"), (lambda: _route(_cfg(L=65)), "L=65"), (lambda: _route(_cfg(b=0)), "b=0"),
    (lambda: _lib.call("svgp_sprites_posterior_rows_route", C.byref(_cfg()), None, 10), "bad argument"),
    (lambda: _lib.call("svgp_sprites_posterior_rows_route", C.byref(_cfg()), C.create_string_buffer(4), 4), "route text"),
])
def test_refusals_are_invalid_with_a_message_and_launch_nothing(call, message):
    """SVGP_ERR_INVALID (-1) before any pointer is looked at: the pointers here are fake, there is no device."""
    with pytest.raises(_lib.SvgpError) as e:
        call()
    assert "status -1" in str(e.value) and message in str(e.value), (message, str(e.value))


@pytest.mark.parametrize("case", AC.KERNEL_IDS)
def test_workspace_is_bounded_and_the_route_has_at_most_two_launches(case):
    b, m, L = AC.kernel_shape(case)
    lib = svgp_vae_amd.load_library()
    n = lib.svgp_sprites_posterior_rows_workspace_elems(C.byref(_cfg(b, m, L)))
    assert 0 <= n <= 16 * b * L
    names = _route(_cfg(b, m, L))
    assert 1 <= len(names) <= 2 and all(re.fullmatch(r"k_[a-z0-9_]+", s) for s in names)


@pytest.mark.parametrize("b,m,L,split", [(288, 72, 64, 1), (288, 256, 64, 1), (1, 1, 1, 1), (100000, 2048, 1, 1), (288, 800, 64, 4),
                                         (72, 800, 64, 8), (1, 2048, 64, 16), (1, 257, 1, 5), (70, 300, 2, 5)])
def test_route_is_one_launch_up_to_256_inducing_points_and_a_bounded_split_beyond(b, m, L, split):
    """Up to m = 256, and wherever (row blocks x L) alone fills the device, ONE launch and no workspace; else the column tiles of a
    row block go to `split` <= 16 workgroups (about 1024 in all, at most one per column tile) and a second launch adds the partials."""
    lib = svgp_vae_amd.load_library()
    one = ["k_sprites_posterior_rows"]
    assert _route(_cfg(b, m, L)) == (one if split == 1 else one + ["k_sprites_posterior_finish"])
    assert lib.svgp_sprites_posterior_rows_workspace_elems(C.byref(_cfg(b, m, L))) == (0 if split == 1 else split * b * L)
    from svgp_vae_amd import animate as A
    assert A.route(dict(m=m, L=L), rows=b) == _route(_cfg(b, m, L))
    if split > 1:
        with pytest.raises(_lib.SvgpError) as e:
            _rows(_cfg(b, m, L))                                 # work = NULL where the split needs it
        assert "status -1" in str(e.value) and "work is NULL" in str(e.value)


# ---------------------------------------------------------------------------------------------- the references themselves
@pytest.mark.parametrize("case", AC.KERNEL_IDS)
def test_einsum_reference_in_a_second_summation_order(case):
    rel = lambda a, c: float(np.abs(a - c).max() / np.abs(c).max())
    ref, ref2 = AC.kernel_reference(case), AC.kernel_reference(case, flip=True)
    for name, a, c in zip(("p_m", "p_v", "z"), ref2, ref):
        e = rel(a, c)
        print(f"{case} {name}: second order {e:.2e}")
        assert e <= 1e-12, (case, name, e)
    assert not np.allclose(AC.kernel_problem(case)["X"][0], AC.kernel_problem(case)["X"][0].T) or AC.kernel_shape(case)[1] == 1


def test_plain_kernel_cases_stay_inside_the_clip_range_mostly():
    """The plain cases test the quadratic form, not the clamp: most of their p_v are strictly inside the range."""
    for case in AC.KERNEL_IDS[:-1]:
        raw = AC.kernel_reference(case)[3]
        assert ((raw > AC.CLIP[0]) & (raw < AC.CLIP[1])).mean() >= 0.9 or raw.size < 4, case


def test_clamp_case_covers_both_bounds_and_the_interior():
    raw = AC.kernel_reference(AC.CLAMP_CASE)[3]
    below, above = int((raw < AC.CLIP[0]).sum()), int((raw > AC.CLIP[1]).sum())
    inside = int(((raw > AC.CLIP[0]) & (raw < AC.CLIP[1])).sum())
    print(f"clamp case: {below} below, {above} above, {inside} inside of {raw.size}")
    assert below >= 1 and above >= 1 and inside >= 1


@pytest.mark.parametrize("case", list(AC.STAGE_CASES))
def test_oracle_response_to_one_ulp_is_within_a_hundredth_of_the_bar(case):
    ref = AC.stage_reference(case)
    ref2 = AC.stage_outputs(case, AC.stage_one_ulp(case))
    for k in ("p_m", "p_v", "z"):
        assert torch.isfinite(ref[k]).all()
        e = H.relerr(ref2[k], ref[k])
        print(f"{case} {k}: oracle response {e:.2e}")
        assert e <= AC.TOL / 100, (case, k, e)
    assert ((ref["p_v"] > AC.CLIP[0]) & (ref["p_v"] < AC.CLIP[1])).all()          # the stage cases do not rest on the clamp


@pytest.mark.parametrize("case", list(AC.STAGE_CASES))
def test_posterior_is_the_kernel_row_against_w_and_X(case):
    """The algebra the cache rests on: k . w and k_bb + k^T (Sigma^-1 - K_mm^-1) k against the oracle's two-term form."""
    p, ref = AC.stage_problem(case), AC.stage_reference(case)
    svgp = AC.stage_svgp(case, p)
    k = svgp.kernel_matrix(p["qaux"], p["ip"], x_inducing=False)
    kbb = svgp.kernel_matrix(p["qaux"], p["qaux"], False, False, diag_only=True)
    X = ref["Si"] - ref["Ki"][None]
    p_m = torch.einsum("bm,lm->bl", k, ref["w"])
    p_v = torch.clamp(kbb[:, None] + torch.einsum("bi,lij,bj->bl", k, X, k), *AC.CLIP)
    e_m, e_v = H.relerr(p_m, ref["p_m"]), H.relerr(p_v, ref["p_v"])
    print(f"{case}: k.w {e_m:.2e}, k_bb + k X k {e_v:.2e}, cond(K_mm) {float(torch.linalg.cond(torch.linalg.inv(ref['Ki']))):.1e}")
    assert e_m < AC.PATH_TOL and e_v < AC.PATH_TOL


# ---------------------------------------------------------------------------------------------- cache file, command line
def _cpu_cache(seed=0):
    from svgp_vae_amd import animate as A
    g = torch.Generator().manual_seed(seed)
    L, m = SHAPE["L"], SHAPE["m"]
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    return A.SpritesPosteriorCache(SHAPE, rn(A.theta_length(SHAPE)), rn(L, m), rn(L, m, m), device="cpu")


def test_cache_file_round_trip_on_cpu_tensors(tmp_path):
    from svgp_vae_amd import animate as A
    cache = _cpu_cache()
    path = str(tmp_path / "cache.pt")
    cache.save(path)
    got = A.SpritesPosteriorCache.load(path, device="cpu")
    assert got.shape == cache.shape and set(got.shape) == set(A._SHAPE_KEYS)
    for k in ("theta", "w", "X"):
        assert getattr(got, k).dtype == torch.float64 and torch.equal(getattr(got, k), getattr(cache, k))
    # theta is the flat vector in SpritesStepEngine.shapes order: networks, inducing points, action table, SE parameters
    names = list(got.params())
    assert names[-3:] == ["inducing_index_points", "GPLVM_action", "se"] and names[0] == "enc_c1_w"
    assert tuple(got.params()["inducing_index_points"].shape) == (SHAPE["m"], 24)
    assert A.route(got) == A.route(got, rows=300) == ["k_sprites_posterior_rows"]


def test_malformed_cache_files_and_wrong_lengths_raise_value_error(tmp_path):
    from svgp_vae_amd import animate as A
    cache = _cpu_cache()
    n = A.theta_length(SHAPE)
    good = {"w": cache.w, "X": cache.X, "theta": cache.theta, "shape": dict(cache.shape)}
    bad = {
        "no_X": {k: v for k, v in good.items() if k != "X"},
        "not_a_dict": [1, 2, 3],
        "shape_field": dict(good, shape={k: v for k, v in SHAPE.items() if k != "n_act"}),
        "theta_len": dict(good, theta=cache.theta[:-1]),
        "w_shape": dict(good, w=cache.w[:, :-1]),
        "X_shape": dict(good, X=cache.X[:, :, :-1]),
        "dtype": dict(good, shape=dict(SHAPE, net_dtype="float16")),
    }
    for name, ck in bad.items():
        path = str(tmp_path / f"{name}.pt")
        torch.save(ck, path)
        with pytest.raises(ValueError) as e:
            A.SpritesPosteriorCache.load(path, device="cpu")
        assert name + ".pt" in str(e.value), (name, str(e.value))
        if name == "theta_len":
            assert str(n) in str(e.value) and str(n - 1) in str(e.value)
    with pytest.raises(ValueError) as e:
        A.SpritesPosteriorCache(SHAPE, torch.zeros(n + 5, dtype=torch.float64), cache.w, cache.X, device="cpu")
    assert str(n) in str(e.value) and str(n + 5) in str(e.value)


def test_checkpoint_theta_must_fit_the_runs_shapes(tmp_path):
    from svgp_vae_amd import animate as A
    a = dict(elbo="SVGPVAE_Hensman", L=2, L_action=8, L_character=16, m=1, N_actions=3, K_SE=True, jitter=0.01, clip_qs=True)
    shape = A.shape_from_run(a, 48)
    assert shape["m"] == 3 and shape["n_act"] == 3 and shape["N_train"] == 48.0
    n = A.theta_length(shape)
    path = str(tmp_path / "model_1.pt")
    torch.save({"theta": torch.arange(n, dtype=torch.float64)}, path)
    assert torch.equal(A.theta_from_run(path, shape), torch.arange(n, dtype=torch.float64))
    torch.save({"theta": torch.zeros(n - 7, dtype=torch.float64)}, path)
    with pytest.raises(ValueError) as e:
        A.theta_from_run(path, shape)
    assert str(n) in str(e.value) and str(n - 7) in str(e.value)
    torch.save({"adam_m": torch.zeros(3)}, path)
    with pytest.raises(ValueError):
        A.theta_from_run(path, shape)
    with pytest.raises(ValueError):
        A.shape_from_run(dict(a, elbo="VAE"), 48)


def test_target_actions_are_checked_before_any_device_work():
    from svgp_vae_amd import animate as A
    cache = _cpu_cache()
    ctx = torch.zeros(1, 1, 64, 64, 3, dtype=torch.float64)
    for bad in ([[0, 9]], [[-1, 2]], [[0.5, 1.0]], [[float("nan"), 1.0]], [0, 1], [[]]):
        with pytest.raises(ValueError):
            A.animate(cache, ctx, np.asarray(bad))
    with pytest.raises(ValueError):
        A.animate(cache, torch.zeros(1, 64, 64, 3), np.asarray([[0, 1]]))
    with pytest.raises(ValueError):
        A.animate(cache, torch.zeros(2, 1, 64, 64, 3), np.asarray([[0, 1]]))


BASE = ["--checkpoint", "run/model_1.pt", "--characters", "0", "1", "--out", "frames.npy"]


@pytest.mark.parametrize("extra", [[], ["--cache", "c.pt", "--synthetic"], ["--cache", "c.pt", "--sprites_data_path", "d/"],
                                   ["--synthetic", "--sprites_data_path", "d/"], ["--cache", "c.pt", "--save_cache", "d.pt"]])
def test_cli_refuses_neither_or_both_of_cache_and_data_source(extra, capsys):
    from svgp_vae_amd import animate as A
    with pytest.raises(SystemExit) as e:
        A.parse_args(BASE + extra)
    assert e.value.code == 2
    assert "--cache" in capsys.readouterr().err


@pytest.mark.parametrize("extra", [["--cache", "c.pt"], ["--synthetic"], ["--sprites_data_path", "d/", "--save_cache", "c.pt"]])
def test_cli_accepts_exactly_one_source(extra):
    from svgp_vae_amd import animate as A
    args = A.parse_args(BASE + extra + ["--N_context", "3", "--actions", "4", "5", "--sample", "--seed", "2"])
    assert args.characters == [0, 1] and args.N_context == 3 and args.actions == [4, 5] and args.sample and args.seed == 2
    assert A.parse_args(BASE + extra).actions is None and A.parse_args(BASE + extra).N_context == 36
