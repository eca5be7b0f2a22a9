"""Casale posterior cache / conditional generation: everything that needs no GPU.  The guard that makes the GPU bars meaningful
(the cache form restated in numpy against the literal N x N oracle, tests/casale_generate_cases.py), the C ABI's declarations,
layout, launch route and refusals, the command line's new flags, casale_models_from_run's refusal and the argument checks of
`generate`."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import svgp_vae_amd
from svgp_vae_amd import _lib
from svgp_vae_amd._lib import CasaleCacheLayout, CasaleCfg
from tests import casale_generate_cases as CG
from tests.helpers import relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("svgp_casale_cache_layout_get", "svgp_casale_cache_build", "svgp_casale_generate_workspace_elems",
               "svgp_casale_generate", "svgp_casale_generate_route")
FAKE = 4096                         # never dereferenced: every call below fails validation first
SPLIT_ROUTE = ["k_casale_generate_rows", "svgp_dgemm_batched", "svgp_dgemm_batched", "k_casale_generate_rowsum",
               "k_casale_generate"]


def _cfg(N=50, n_obj=9, Q=5, M=3, L=3, **kw):
    base = dict(N=N, n_obj=n_obj, Q=Q, M=M, L=L, b_cap=1, normalize_obj=0, train_gp=0, train_ov=1)
    base.update(kw)
    return CasaleCfg(**base)


def _generate(q, b=4, theta=FAKE, cache=FAKE, aux=FAKE, gather=1, images=FAKE, work=FAKE):
    return _lib.call("svgp_casale_generate", None if q is None else C.byref(q), b, theta, cache, aux, gather, None, images, None,
                     None, work, None)


def _route(q):
    buf = C.create_string_buffer(512)
    _lib.call("svgp_casale_generate_route", C.byref(q), buf, len(buf))
    return buf.value.decode().split()


# ---------------------------------------------------------------------------------------------- 1. the guard
@pytest.mark.parametrize("variant", list(CG.VARIANTS))
def test_cache_form_equals_the_literal_posterior(variant):
    """mean* = v*^T U and var* = k** - |v*|^2 + alpha v*^T P v* against K_*n K_inv Z and k** - k*^T K_inv k* of the N x N form."""
    pr, ref, cf = CG.problem(variant), CG.reference(variant), CG.cache_form(variant)
    cond = float(np.linalg.cond(cf["K_W"]))
    e_m, e_v = relerr(cf["mean"], ref["mean"]), relerr(cf["var"], ref["var"])
    print(f"{variant}: H {pr['H']} N {pr['N']} cond(K_W) {cond:.2e}  mean {e_m:.2e}  var {e_v:.2e}  min var {float(ref['var'].min()):.3e}")
    assert cond <= CG.COND_MAX, (variant, cond)
    assert float(ref["var"].min()) > 0
    assert e_m < CG.GUARD_TOL and e_v < CG.GUARD_TOL, (variant, e_m, e_v)
    for k in ("mean", "var", "images", "images_mean"):
        assert torch.isfinite(ref[k]).all()
    q = pr["qaux"]
    assert q.shape == (CG.N_QUERY, 2 + pr["M"]) and float(q[2, 1]) == -0.3 and float(q[3, 1]) == 7.0
    assert int(q[4, 0]) == pr["unused_id"] and pr["unused_id"] not in pr["case"]["aux"][:, 1]


def test_the_case_table_covers_both_routes_and_the_boundary():
    H = {v: CG.problem(v)["H"] for v in CG.VARIANTS}
    assert H["H256-raw"] == 256 and H["H258-raw"] == 258 and H["M128"] == 384 and H["H513-norm"] == 513 and H["Q32-raw"] == 64
    assert CG.problem("H256-raw")["Q"] == 32 and CG.problem("C-norm")["N"] == 447 and CG.problem("M128")["N"] < 384
    assert {CG.problem(v)["L"] for v in CG.VARIANTS} >= {1, 16, 64}


# ---------------------------------------------------------------------------------------------- 2. the C ABI
def test_header_declares_and_library_exports_the_new_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svgpvae_hip.h")).read(), flags=re.S)
    lib = svgp_vae_amd.load_library()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", src), f"{n} not declared in include/svgpvae_hip.h"
        assert hasattr(lib, n), f"{n} not exported"
        assert n in _lib.SIGNATURES or n in _lib.NON_STATUS
    assert lib.svgp_struct_sizeof(18) == C.sizeof(CasaleCacheLayout) == 5 * 8
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*svgp_casale_cache_layout\s*;", src, flags=re.S).group(1)
    assert re.findall(r"[A-Za-z_]\w*", body.replace("int64_t", "")) == [n for n, _ in CasaleCacheLayout._fields_]


@pytest.mark.parametrize("Q,M", [(1, 1), (5, 3), (15, 8), (32, 8), (6, 43), (32, 64)])
def test_route_is_one_launch_up_to_H_256_and_five_beyond(Q, M):
    want = ["k_casale_generate"] if Q * M <= 256 else SPLIT_ROUTE
    assert _route(_cfg(Q=Q, M=M)) == want
    lib = svgp_vae_amd.load_library()
    n = lib.svgp_casale_generate_workspace_elems(C.byref(_cfg(Q=Q, M=M)), 300)
    assert (n == 0) == (Q * M <= 256)
    if n:
        H, L = Q * M, 3
        assert n >= 2 * 256 * H + 256 + 2 * 256 * L
        assert lib.svgp_casale_generate_workspace_elems(C.byref(_cfg(Q=Q, M=M)), 256) == n      # passes of 256 rows
        assert 0 < lib.svgp_casale_generate_workspace_elems(C.byref(_cfg(Q=Q, M=M)), 7) < n
        assert lib.svgp_casale_generate_workspace_elems(C.byref(_cfg(Q=Q, M=M)), 0) == 0


def test_route_of_the_boundary_cases():
    from svgp_vae_amd import generate as G
    shape = lambda pr: dict(N=pr["N"], n_obj=pr["n_obj"], Q=pr["Q"], M=pr["M"], L=pr["L"], normalize_obj=0, ov_joint=1)
    assert G.route(shape(CG.problem("H256-raw"))) == ["k_casale_generate"]
    assert G.route(shape(CG.problem("H258-raw"))) == SPLIT_ROUTE
    assert G.route(dict(m=12, L=3, M=4, n_obj=20, normalize_obj=0, N_train=100.0, jitter=1e-6)) == ["k_generate"]


@pytest.mark.parametrize("Q,M,L", [(1, 1, 1), (5, 3, 3), (15, 8, 16), (32, 8, 64), (19, 27, 3), (32, 64, 64)])
def test_cache_layout_is_increasing_disjoint_and_aligned(Q, M, L):
    cl = CasaleCacheLayout()
    _lib.call("svgp_casale_cache_layout_get", C.byref(_cfg(Q=Q, M=M, L=L)), C.byref(cl))
    H = Q * M
    end = 0
    for name, n in (("angles", Q), ("L_W", Q * Q), ("U", H * L), ("P", H * H)):
        off = getattr(cl, name)
        assert off >= end and off % 16 == 0, (name, off, end)
        end = off + n
    assert cl.total >= end and cl.total == (end + 15) // 16 * 16


@pytest.mark.parametrize("kw,message", [(dict(Q=33), "Q=33"), (dict(Q=17, M=121), "H = M Q = 2057"), (dict(M=129, Q=1), "M=129"),
                                        (dict(L=65), "L=65")])
def test_shapes_past_the_ceilings_are_unsupported(kw, message):
    lib = svgp_vae_amd.load_library()
    q = _cfg(**kw)
    calls = [lambda: lib.svgp_casale_cache_layout_get(C.byref(q), C.byref(CasaleCacheLayout())),
             lambda: lib.svgp_casale_cache_build(C.byref(q), FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None),
             lambda: lib.svgp_casale_generate(C.byref(q), 4, FAKE, FAKE, FAKE, 1, None, FAKE, None, None, FAKE, None),
             lambda: lib.svgp_casale_generate_route(C.byref(q), C.create_string_buffer(64), 64)]
    for f in calls:
        assert f() == -2                                         # SVGP_ERR_UNSUPPORTED
        assert message in lib.svgp_last_error().decode()
    assert lib.svgp_casale_generate_workspace_elems(C.byref(q), 4) == 0


def test_invalid_arguments_are_refused_with_their_message():
    big = _cfg(Q=6, M=43)
    build = lambda **kw: _lib.call("svgp_casale_cache_build", C.byref(_cfg()), *[kw.get(k, FAKE) for k in
                                   ("gp", "angles", "obj_idx", "ang_idx", "Z", "ws", "cache")], None)
    cases = [
        (lambda: _generate(None), "casale cfg is NULL"),
        (lambda: _generate(_cfg(), b=-1), "b = -1"),
        (lambda: _generate(_cfg(), theta=None), "NULL device pointer"),
        (lambda: _generate(_cfg(), cache=None), "NULL device pointer"),
        (lambda: _generate(_cfg(), aux=None), "NULL device pointer"),
        (lambda: _generate(_cfg(), images=None), "NULL device pointer"),
        (lambda: _generate(_cfg(n_obj=0), gather=1), "bad Casale shape"),
        (lambda: _generate(big, work=None), "work is NULL"),
        (lambda: _lib.call("svgp_casale_cache_layout_get", C.byref(_cfg()), None), "out is NULL"),
        (lambda: _lib.call("svgp_casale_generate_route", C.byref(_cfg()), None, 10), "bad argument"),
        (lambda: _lib.call("svgp_casale_generate_route", C.byref(big), C.create_string_buffer(20), 20), "route text needs more"),
    ] + [(lambda k=k: build(**{k: None}), "NULL device pointer") for k in ("gp", "angles", "obj_idx", "ang_idx", "Z", "ws", "cache")]
    for f, message in cases:
        with pytest.raises(_lib.SvgpError) as e:
            f()
        assert "status -1" in str(e.value) and message in str(e.value), (message, str(e.value))
    # b = 0: nothing to do, nothing launched (no device on this path), also with NULL work on the split route
    _generate(_cfg(), b=0)
    _generate(big, b=0, work=None)
    _generate(_cfg(), work=None, b=0)


# ---------------------------------------------------------------------------------------------- 3. Python side
def test_parser_has_the_latent_flags_and_keeps_the_old_ones():
    from svgp_vae_amd.generate import build_parser
    a = build_parser().parse_args(["--checkpoint", "r/model_4.pt", "--out", "o.npy", "--ids", "0", "1"])
    assert a.latent == "sample" and a.latent_seed is None and a.n_angles == 16 and not a.sample and a.seed == 0 and a.chunk == 1024
    a = build_parser().parse_args(["--checkpoint", "r/model_4.pt", "--out", "o.npy", "--aux_file", "q.npy", "--latent", "mean",
                                   "--latent_seed", "3"])
    assert a.latent == "mean" and a.latent_seed == 3 and a.aux_file == "q.npy"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--checkpoint", "c", "--out", "o", "--latent", "mode"])


def _run_dir(tmp_path, n_theta, **args):
    base = dict(elbo="GPVAE_Casale", L=4, M=8, dataset="3", PCA=False, ov_joint=True, GP_joint=True, seed=0,
                object_kernel_normalize=False, mnist_data_path=str(tmp_path) + "/")
    base.update(args)
    json.dump(base, open(tmp_path / "args.json", "wt"))
    f = lambda n: torch.zeros(n, dtype=torch.float64)
    torch.save({"theta": f(n_theta), "adam_m": f(n_theta), "adam_v": f(n_theta), "state": f(16)}, tmp_path / "model_4.pt")
    return str(tmp_path / "model_4.pt")


def test_casale_models_from_run_refuses_a_theta_of_another_shape(tmp_path):
    from svgp_vae_amd import generate as G
    wl = _lib.CasaleLayout()
    _lib.call("svgp_casale_layout_get", C.byref(_cfg(N=1, n_obj=400, Q=1, M=8, L=4)), C.byref(wl))
    assert wl.n_total == wl.n_vae + 3 + 400 * 8
    ck = _run_dir(tmp_path, wl.n_total - 8)
    with pytest.raises(ValueError) as e:
        G.casale_models_from_run(ck, None)
    assert str(wl.n_total) in str(e.value) and str(wl.n_total - 8) in str(e.value)
    ck = _run_dir(tmp_path, wl.n_total, elbo="SVGPVAE_Hensman")
    with pytest.raises(ValueError, match="not a GPVAE_Casale run"):
        G.casale_models_from_run(ck, None)
    ck = _run_dir(tmp_path, wl.n_total)                              # and the SVGPVAE loader still refuses a Casale run
    with pytest.raises(ValueError, match="not an SVGPVAE run"):
        G.models_from_run(ck, None)


def _stand_in(**kw):
    """A CasalePosteriorCache that holds its shape only: `generate` checks its arguments before it needs the device."""
    from svgp_vae_amd.generate import CasalePosteriorCache
    c = object.__new__(CasalePosteriorCache)
    c.shape = dict(N=50, n_obj=9, Q=5, M=3, L=3, normalize_obj=0, ov_joint=1)
    c.shape.update(kw)
    return c


def test_generate_checks_its_arguments_before_the_device_is_needed():
    from svgp_vae_amd.generate import generate
    rows = torch.zeros(4, 5, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"aux must be \(b, 5\)"):
        generate(_stand_in(), torch.zeros(4, 4))
    with pytest.raises(ValueError, match=r"aux must be \(b, 5\)"):
        generate(_stand_in(), torch.zeros(5))
    for bad in (9.0, -1.0, 2.5):
        r = rows.clone()
        r[2, 0] = bad
        with pytest.raises(ValueError, match=r"integers in \[0, 9\)"):
            generate(_stand_in(), r)                             # gather defaults to the model's ov_joint = 1
        with pytest.raises(ValueError, match=r"integers in \[0, 9\)"):
            generate(_stand_in(ov_joint=0), r, gather=True)
    with pytest.raises(ValueError, match=r"eps must be \(4, 3\)"):
        generate(_stand_in(), rows, eps=torch.zeros(4, 2))
    with pytest.raises(ValueError, match=r"eps must be \(4, 3\)"):
        generate(_stand_in(ov_joint=0), rows + 20.0, eps=torch.zeros(3, 3))       # (ids unchecked without gather)
    if not torch.cuda.is_available():
        from svgp_vae_amd.generate import CasalePosteriorCache
        with pytest.raises(_lib.SvgpError, match="no CPU execution path"):
            CasalePosteriorCache(_stand_in().shape, torch.zeros(10), None)
