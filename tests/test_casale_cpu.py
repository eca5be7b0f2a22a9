"""Casale GP-VAE, CPU side: the two formulations of the restatement agree far below the GPU bars, the efficient block passes
gradcheck, the numpy helpers keep the reference's semantics, the module's import surface and ABI mirrors are in place and
the engine refuses to run without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import svgp_vae_amd
from svgp_vae_amd import GPVAE_Casale_model  # noqa: F401  (without the feature every test of this file fails here)
from svgp_vae_amd import _lib
from tests import casale_cases as CC
from tests.helpers import relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_ENV = {}


def _env_case(name, normalize=False):
    """Envelope cases are built once per module."""
    if (name, normalize) not in _ENV:
        _ENV[name, normalize] = CC.make_envelope_case(name, normalize)
    return _ENV[name, normalize]


# envelope cases whose literal (L, N, H) tensor B stays under ~50 MB, from the table alone (N <= P Q): no case is built at import
LITERAL_ENVELOPE = [n for n, c in CC.ENVELOPE_CASES.items() if 8 * c["L"] * (c["P"] * c["Q"]) * (c["M"] * c["Q"]) < 50e6]


@pytest.mark.parametrize("name", ["A", "B", "C"] + LITERAL_ENVELOPE)
def test_literal_equals_efficient(name):
    """The N x N form of the reference and the H x H form agree at least 100 times below the bar the GPU tests use for the
    same quantity; the disagreement is printed (NOTEBOOK.md has the values).  Envelope cases: the ragged middle batch."""
    case = CC.make_case(name) if name in CC.CASES else _env_case(name)
    batch = case["batches"][0 if name in CC.CASES else 2]
    lit = CC.gp_stage_reference(case, batch, formulation="literal")
    eff = CC.gp_stage_reference(case, batch, formulation="efficient")
    worst = {}
    for k, bar in (("GP_prior_term", CC.SCALAR_TOL), ("V", CC.FWD_TOL), ("Zbar", CC.GRAD_TOL), ("zbbar", CC.GRAD_TOL),
                   ("l_GP", CC.GRAD_TOL), ("amplitude", CC.GRAD_TOL), ("alpha", CC.GRAD_TOL), ("object_vectors", CC.GRAD_TOL)):
        worst[k] = (relerr(eff[k], lit[k]), bar)
    print(f"case {name} N={case['N']} H={case['H']}: " + ", ".join(f"{k} {e:.1e}" for k, (e, _) in worst.items()))
    for k, (e, bar) in worst.items():
        assert e <= bar / 100, (k, e, bar)


def test_envelope_case_builder_keeps_its_promises():
    """Every object and every angle keeps a row, table rows are unused (0 and the last one in some cases, both used in
    others), one object has a single row unless all pairs are kept, the three batches are the whole set, the last row and a
    ragged middle range, and the sizes the cases are named for hold."""
    assert LITERAL_ENVELOPE == [n for n in CC.ENVELOPE_CASES if n != "H2048_L64"]
    edges = set()
    for name, spec in CC.ENVELOPE_CASES.items():
        c = _env_case(name)
        N, P, Q = c["N"], spec["P"], spec["Q"]
        mask = c["mask"].reshape(P, Q)
        assert mask.any(1).all() and mask.any(0).all() and N == mask.sum()
        assert len(np.unique(c["aux"][:, 2])) == Q and len(np.unique(c["aux"][:, 1])) == P
        assert np.all(np.diff(c["aux"][:, 1]) >= 0) and c["H"] == spec["M"] * Q
        spacing = 2 * np.pi / Q
        assert np.all(np.abs(c["angles"] - np.arange(Q) * spacing) <= 0.2 * spacing + 1e-15)
        used = np.unique(c["aux"][:, 1]).astype(int)
        assert len(c["unused"]) == 3 and not set(c["unused"]) & set(used) and c["n_obj"] == P + 3
        edges.add((0 in used, c["n_obj"] - 1 in used))
        rows = np.bincount(c["aux"][:, 1].astype(int), minlength=c["n_obj"])
        if spec.get("keep", 0.75) < 1.0:
            assert rows[c["single"]] == 1
        else:
            assert N == P * Q
        (a0, a1), (b0, b1), (m0, m1) = c["batches"]
        assert (a0, a1) == (0, N) and (b0, b1) == (N - 1, N) and 0 < m0 < m1 < N
        assert set(c["zb"]) == set(c["batches"])
    assert edges == {(False, False), (True, True)}
    N = {n: _env_case(n)["N"] for n in CC.ENVELOPE_CASES}
    H = {n: _env_case(n)["H"] for n in CC.ENVELOPE_CASES}
    assert (H["H1"], H["Q32"], H["M128"], H["H511"], H["H512"], H["H513"], H["H512_N"], H["H1024"], H["H2048_L64"]) == \
        (1, 64, 384, 511, 512, 513, 512, 1024, 2048)
    assert (N["N64"], N["N65"]) == (64, 65) and N["M128"] < H["M128"] and N["H2048_L64"] < 2048
    assert max(N["H511"], N["H512"], N["H513"]) < 256 <= min(N["H512_N"], N["H1024"])
    assert N["L64"] % 4 != 0 or N["L1"] % 4 != 0


@pytest.mark.parametrize("name,normalize", CC.envelope_variants(), ids=lambda v: {False: "raw", True: "norm"}.get(v, v))
def test_envelope_oracle_response_is_far_below_the_tolerances(name, normalize):
    """The guard of tests/test_gpu_casale_envelope.py: every real input of gp_stage_reference (Z, zb, object vectors, l_GP,
    amplitude, alpha) moved by one ulp moves no compared quantity by more than a hundredth of its bar, for every case and
    batch.  A case that fails here gets other inputs, never a wider bar."""
    case = _env_case(name, normalize)
    gen = torch.Generator().manual_seed(17)
    ulp = lambda x: (CC.t64(x) * (1.0 + 2.0 ** -52 * (torch.randint(0, 2, np.shape(x), generator=gen).to(CC.DT) * 2 - 1))).numpy()
    moved = dict(case, Z=ulp(case["Z"]), object_vectors=ulp(case["object_vectors"]), l_GP=float(ulp(case["l_GP"])),
                 amplitude=float(ulp(case["amplitude"])), alpha=float(ulp(case["alpha"])),
                 zb={b: ulp(v) for b, v in case["zb"].items()})
    assert moved["l_GP"] != case["l_GP"] and not np.array_equal(moved["Z"], case["Z"])
    worst = {}
    for batch in case["batches"]:
        ref, ref2 = CC.gp_stage_reference(case, batch), CC.gp_stage_reference(moved, batch)
        for k, v in ref.items():
            assert torch.isfinite(v).all(), (k, batch)
        resp = {k: (relerr(ref2[k], ref[k]), CC.FWD_TOL) for k in ("K_W", "L_W", "V", "G", "P", "U", "A")}
        resp["terms"] = (relerr(ref2["terms"], ref["terms"]), CC.SCALAR_TOL)
        resp["GP_prior_term"] = (abs(float(ref2["GP_prior_term"]) - float(ref["GP_prior_term"]))
                                 / abs(float(ref["GP_prior_term"])), CC.SCALAR_TOL)
        for k in ("Zbar", "zbbar") + CC.GP_NAMES:
            resp[k] = (relerr(ref2[k], ref[k]), CC.GRAD_TOL)
        for k, (e, bar) in resp.items():
            assert e <= bar / 100, (name, batch, k, e, bar)
            worst[bar] = max(worst.get(bar, 0.0), e)
    print(f"envelope {name}{' norm' if normalize else ''} N={case['N']} H={case['H']} L={case['L']}: worst oracle response "
          + ", ".join(f"{e:.1e} (bar {bar:.0e})" for bar, e in sorted(worst.items())))


def test_v_rowwise_is_the_masked_kronecker_product():
    for normalize in (False, True):
        case = CC.make_case("A", normalize=normalize)
        ov = CC.t64(case["object_vectors"])
        a = CC.V_literal(ov, case["aux"], case["mask"], case["l_GP"], case["amplitude"], normalize)
        b = CC.V_rowwise(ov, case["aux"], case["l_GP"], case["amplitude"], normalize)
        assert a.shape == (case["N"], case["H"]) and torch.equal(a, b)


def test_gradcheck_of_the_efficient_block():
    case = CC.make_case("A")
    lo, hi = case["batches"][0]
    V0 = CC.V_rowwise(CC.t64(case["object_vectors"]), case["aux"], case["l_GP"], case["amplitude"], False)
    leaf = lambda x: CC.t64(x).clone().requires_grad_(True)
    f = lambda Z, zb, V, alpha: CC.gp_prior_efficient(Z, zb, V, alpha, lo, hi)
    assert torch.autograd.gradcheck(f, (leaf(case["Z"]), leaf(case["zb"][(lo, hi)]), leaf(V0), leaf(case["alpha"])),
                                    eps=1e-6, atol=1e-6, rtol=1e-5)


def test_hand_reverse_pass_of_the_header_block():
    """The reverse pass written in include/svgpvae_hip.h's notation (what casale.hip evaluates) against autograd."""
    case = CC.make_case("A")
    lo, hi = case["batches"][1]
    Z, zb, al = CC.t64(case["Z"]), CC.t64(case["zb"][(lo, hi)]), case["alpha"]
    V = CC.V_rowwise(CC.t64(case["object_vectors"]), case["aux"], case["l_GP"], case["amplitude"], False)
    N, H = V.shape
    L = Z.shape[1]
    _, w = CC.gp_prior_efficient(Z, zb, V, CC.t64(al), lo, hi, want=True)
    P, U, A, W = w["P"], w["U"], w["A"], w["W"]
    Vb, Ab = V[lo:hi], A[lo:hi]
    Abar = -al * A
    Abar[lo:hi] += zb - Vb @ U
    Ubar = -Vb.T @ Ab - V.T @ Abar / al
    Vbar = -Abar @ U.T / al
    Vbar[lo:hi] += -Ab @ U.T + 2 * L * Vb @ P
    Pbar = L * Vb.T @ Vb + (al * L / 2) * torch.eye(H, dtype=CC.DT) + Ubar @ W.T
    Wbar = P @ Ubar
    Mbar = -P @ Pbar @ P
    Vbar += Z @ Wbar.T + V @ (Mbar + Mbar.T)
    Zbar = Abar / al + V @ Wbar
    trKinv = (N - H) / al + torch.trace(P)
    alphabar = (-torch.sum(A * A) + L * trKinv) / 2 - L * (N - H) / (2 * al) - torch.sum(Abar * A) / al + torch.trace(Mbar)
    leaf = lambda x: x.clone().requires_grad_(True)
    Zl, zbl, Vl, all_ = leaf(Z), leaf(zb), leaf(V), leaf(CC.t64(al))
    g = torch.autograd.grad(CC.gp_prior_efficient(Zl, zbl, Vl, all_, lo, hi), [Zl, zbl, Vl, all_])
    for mine, ref in zip((Zbar, Ab, Vbar, alphabar), g):
        assert relerr(mine, ref) < 1e-11


def test_numpy_helpers_keep_the_reference_semantics():
    from svgp_vae_amd.GPVAE_Casale_model import _angles_mask, sort_train_data, tf_kron
    case = CC.make_case("A")
    rng = np.random.RandomState(0)
    perm = rng.permutation(case["N"])
    rows = case["aux"][perm, 1:]
    images = rng.rand(case["N"], 28, 28, 1)
    out = sort_train_data(dict(images=images.copy(), aux_data=rows.copy()))
    assert np.array_equal(out["aux_data"], case["aux"])                       # sorted by (id, angle), id column range(N)
    order = np.lexsort((rows[:, 1], rows[:, 0]))
    assert np.array_equal(out["images"], images[order])
    assert np.array_equal(_angles_mask(rows), case["mask"])
    a, b = rng.rand(3, 2), rng.rand(4, 5)
    assert np.array_equal(tf_kron(a, b).numpy(), np.kron(a, b))


def test_import_surface_of_the_reference_driver():
    from svgp_vae_amd.GPVAE_Casale_model import casaleGP, forward_pass_Casale, predict_test_set_Casale, sort_train_data, encode  # noqa: F401
    from svgp_vae_amd.GPVAE_Casale_model import tf_kron, train_angles_mask, CasaleStepEngine  # noqa: F401
    for name in ("kernel_matrix", "V_matrix", "taylor_coeff", "variable_summary"):
        assert callable(getattr(casaleGP, name))
    GP = casaleGP(False, np.ones((3, 2)), False, True)
    assert GP.variable_summary()[0] == 1.0 and GP.variable_summary()[3] == 0.1 and GP.variable_summary()[2].shape == (3, 2)


def _header_struct_fields(name):
    src = open(os.path.join(ROOT, "include", "svgpvae_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + name + r"\s*;", src, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, rest = decl.split(None, 1)
            out += [(ctype, f.strip()) for f in rest.split(",")]
    return out


def test_casale_struct_mirrors_follow_the_header():
    lib = svgp_vae_amd.load_library()
    ct = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    for which, cname, cls in ((8, "svgp_casale_cfg", _lib.CasaleCfg), (9, "svgp_casale_layout", _lib.CasaleLayout)):
        want = _header_struct_fields(cname)
        assert [f for _, f in want] == [n for n, _ in cls._fields_], cname
        assert [ct[t] for t, _ in want] == [t for _, t in cls._fields_], cname
        assert lib.svgp_struct_sizeof(which) == C.sizeof(cls)


def test_layout_and_refusals_without_a_launch():
    """The flat parameter order is encoder, decoder, l_GP, amplitude, alpha, object_vectors (GP variables are a suffix); shapes
    outside the build are refused with a message by the layout call every entry point starts with."""
    ok = dict(N=4050, n_obj=400, Q=15, M=8, L=16, b_cap=256)
    wl = _lib.CasaleLayout()
    _lib.call("svgp_casale_layout_get", C.byref(_lib.CasaleCfg(**ok)), C.byref(wl))
    assert (wl.n_enc, wl.n_vae) == (2304, 5721)
    for L in (3, 16, 64):                                         # the VAE prefix is the MNIST step's own layout
        pl = _lib.ParamLayout()
        _lib.call("svgp_mnist_param_layout_get", C.byref(_lib.MnistCfg(b=1, b_global=1, m=1, L=L, M=1, n_obj=0, N_train=1.0)),
                  C.byref(pl))
        _lib.call("svgp_casale_layout_get", C.byref(_lib.CasaleCfg(**{**ok, "L": L})), C.byref(wl))
        assert (wl.n_enc, wl.n_vae, wl.th_l_GP) == (pl.n_enc, pl.n_vae, pl.n_vae)
    _lib.call("svgp_casale_layout_get", C.byref(_lib.CasaleCfg(**ok)), C.byref(wl))
    assert (wl.th_l_GP, wl.th_amplitude, wl.th_alpha, wl.th_ov, wl.n_total) == (5721, 5722, 5723, 5724, 5724 + 3200)
    offs = sorted(getattr(wl, f) for f in _lib.CASALE_FIELDS[7:] if f not in ("n_lv", "n_chunk", "scr_splitk_len", "total"))
    assert len(set(offs)) == len(offs) and offs[-1] < wl.total
    for change, msg in ((dict(Q=33), "Q <= 32"), (dict(M=128, Q=17), "H <= 2048"), (dict(M=129, Q=2), "M=129"),
                        (dict(L=65), "64 latent channels"), (dict(b_cap=5000), "bad Casale shape")):
        with pytest.raises(svgp_vae_amd.SvgpError, match=msg):
            _lib.call("svgp_casale_layout_get", C.byref(_lib.CasaleCfg(**{**ok, **change})), C.byref(_lib.CasaleLayout()))
    fake = C.c_void_p(4096)                                       # never dereferenced: validation fails first
    cfg = _lib.CasaleCfg(**ok)
    for lo, hi in ((-1, 10), (4000, 4051), (10, 10), (0, 257)):
        with pytest.raises(svgp_vae_amd.SvgpError, match="batch"):
            _lib.call("svgp_casale_gp_fwd", C.byref(cfg), fake, fake, fake, fake, fake, fake, lo, hi, fake, None)
    with pytest.raises(svgp_vae_amd.SvgpError, match="NULL"):
        _lib.call("svgp_casale_gp_bwd", C.byref(cfg), fake, fake, fake, fake, None, fake, 0, 10, 1.0, fake, None)
    # the envelope cases: the split-K scratch is the larger of the two tall products', n_lv and n_chunk follow their formulas
    lib = svgp_vae_amd.load_library()
    scratch = {}
    for name in CC.ENVELOPE_CASES:
        c = _env_case(name)
        N, H, L = c["N"], c["H"], c["L"]
        _lib.call("svgp_casale_layout_get", C.byref(_lib.CasaleCfg(N=N, n_obj=c["n_obj"], Q=c["Q"], M=c["M"], L=L, b_cap=N)),
                  C.byref(wl))
        s1, s2 = (int(lib.svgp_dgemm_splitk_scratch_elems(H, n, N)) for n in (H, L))
        scratch[name] = (s1, s2)
        assert wl.scr_splitk_len == max(s1, s2), name
        assert (wl.n_lv, wl.n_chunk) == (-(-N * L // 256), -(-N // 64)), name
        assert wl.n_total == wl.th_ov + c["n_obj"] * c["M"] and wl.scr_splitk + wl.scr_splitk_len <= wl.total
    # what the cases are there for: both products split at H512_N, only the H x L one at H1024, none below 256 rows
    assert min(scratch["H512_N"]) > 0 and scratch["H1024"][0] == 0 and scratch["H1024"][1] > 0
    assert all(scratch[n] == (0, 0) for n in CC.ENVELOPE_CASES if _env_case(n)["N"] < 256)
    assert (_env_case("N64")["N"] * 17, _env_case("N65")["N"]) == (64 * 17, 65)


def test_engine_refuses_to_run_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from svgp_vae_amd.GPVAE_Casale_model import CasaleStepEngine, casaleGP
    from svgp_vae_amd.VAE_utils import mnistVAE
    case = CC.make_case("A")
    GP = casaleGP(False, case["object_vectors"], False, True)
    with pytest.raises(svgp_vae_amd.SvgpError, match="no CPU execution path"):
        CasaleStepEngine(mnistVAE(L=3), GP, np.zeros((case["N"], 28, 28, 1)), case["aux"], batch_size=8)
    with pytest.raises(svgp_vae_amd.SvgpError, match="single GPU"):
        CasaleStepEngine(mnistVAE(L=3), GP, np.zeros((case["N"], 28, 28, 1)), case["aux"], batch_size=8, world_size=2)
    with pytest.raises(svgp_vae_amd.SvgpError, match="no CPU execution path"):
        GP.V_matrix(case["aux"], case["mask"])


# ---------------------------------------------------------------------------------------------------------- reference-executed fixture
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ref_fixture():
    return np.load(os.path.join(GOLDEN_DIR, "ref_casale_small.npz")), np.load(os.path.join(GOLDEN_DIR, "mnist_cfg2_inputs.npz"))


@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "norm"])
def test_restatement_equals_the_reference_executed_fixture(ref_fixture, normalize):
    """tests/golden/ref_casale_small.npz holds what the reference's own GPVAE_Casale_model.py computes (executed on the
    TensorFlow stand-in); both formulations of the restatement reproduce it."""
    fx, gin = ref_fixture
    tag = "norm" if normalize else "raw"
    prob = CC.fixture_problem(gin, normalize)
    p, L, lo, hi = prob["params"], prob["L"], prob["lo"], prob["hi"]
    aux3, mask = prob["aux"][:, :3], prob["case"]["mask"]
    V = CC.V_literal(p["object_vectors"], aux3, mask, p["l_GP"], p["amplitude"], normalize)
    assert relerr(V, fx[f"{tag}.V"]) < 1e-14
    Z = CC.t64(fx[f"{tag}.Z"])
    for got, k in zip(CC.taylor_coeff_literal(Z, V, p["alpha"]), ("a", "B", "c")):
        assert relerr(got, fx[f"{tag}.{k}"]) < 1e-12, k
    for formulation in ("literal", "efficient"):
        out, grads = CC.step_reference("joint", p, prob["images"], aux3, lo, hi, prob["eps_f"], prob["eps_b"], beta=prob["beta"],
                                       clip=True, normalize=normalize, L=L, ov_joint=True, formulation=formulation, mask=mask)
        CC.assert_clip_margin(out["var_all"], lo, hi)
        for k in ("elbo", "recon_loss", "GP_prior_term", "log_var", "qnet_mu", "qnet_var"):
            assert relerr(out[k], fx[f"{tag}.fwd.{k}"]) < 1e-11, (formulation, k)
        assert relerr(out["recon"], fx[f"{tag}.fwd.recon_images"]) < 1e-11
        for k, g in grads.items():
            assert relerr(g, fx[f"{tag}.grad.{k}"]) < 1e-10, (formulation, k)
    train_aux = CC.t64(prob["aux"])
    for take_mean, kind in ((True, "mean"), (False, "sample")):
        rec, loss, _, var = CC.predict_reference(prob["test_images"], prob["test_aux"], train_aux, p, V, Z, L=L,
                                                 normalize=normalize, ov_joint=True, take_mean=take_mean, epsilon=prob["eps_t"])
        assert relerr(rec, fx[f"{tag}.predict.{kind}.recon"]) < 1e-11 and relerr(loss, fx[f"{tag}.predict.{kind}.loss"]) < 1e-11
    # the sampled prediction pins the reference's tile / reshape layout: one variance per row gives another image
    assert float(var.min()) > 0 and float(var.max() / var.min()) > 1.01
    per_row = CC.O.MnistVAE(p, L).decode(CC.predict_reference(prob["test_images"], prob["test_aux"], train_aux, p, V, Z, L=L,
                                                              normalize=normalize, ov_joint=True, take_mean=True)[2]
                                         + prob["eps_t"] * torch.sqrt(var)[:, None])
    assert relerr(per_row, fx[f"{tag}.predict.sample.recon"]) > 1e-6


def test_eval_every_defaults_per_driver():
    """--eval_every, abbreviated or not, wins; without it the Casale driver evaluates every 5 epochs (:1067) and the others
    every 10; the Casale driver called directly with a bare namespace takes its default too."""
    import argparse

    from svgp_vae_amd.MNIST_experiment import _eval_every, build_parser
    args = build_parser().parse_args(["--elbo", "GPVAE_Casale"])
    assert (_eval_every(args, 5), _eval_every(args, 10)) == (5, 10)
    for flag in ("--eval_every", "--eval_e"):
        args = build_parser().parse_args(["--elbo", "GPVAE_Casale", flag, "2"])
        assert (_eval_every(args, 5), _eval_every(args, 10)) == (2, 2)
    assert _eval_every(argparse.Namespace(), 5) == 5


def test_numpy_helpers_equal_the_fixture_bit_for_bit(ref_fixture):
    from svgp_vae_amd.GPVAE_Casale_model import _angles_mask, sort_train_data
    fx, gin = ref_fixture
    rows = gin["train_aux"]
    shuffled = rows[np.random.RandomState(5).permutation(len(rows))]
    srt = sort_train_data(dict(images=np.arange(len(rows), dtype=np.float64), aux_data=shuffled.copy()))
    assert np.array_equal(srt["images"].astype(np.int32), fx["sort.order"])
    assert np.array_equal(srt["aux_data"][:, 0].astype(np.int32), fx["sort.id_column"])
    assert np.array_equal(srt["aux_data"][:, 1:], shuffled[fx["sort.order"]])
    mask = _angles_mask(shuffled)
    assert mask.dtype == bool and np.array_equal(mask, fx["mask"])
    assert np.array_equal(mask, np.load(os.path.join(GOLDEN_DIR, "mnist_train_ids_mask.npz"))["train_ids_mask"])
