"""Posterior cache / conditional generation / checkpoint restore: everything that needs no GPU.  The C ABI's declarations,
exports, refusals, layout and launch route; the conditioning guard and the algebra of tests/generate_cases.py; checkpoint.load /
restore on CPU tensors; the driver's new flags; run_sharded_epochs(first_epoch=...)."""
import ctypes as C
import os
import re
import socket
import types

import pytest
import torch

import svgp_vae_amd
from svgp_vae_amd import _lib
from svgp_vae_amd._lib import CacheLayout, MnistCfg
from tests import generate_cases as GC
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("svgp_mnist_cache_layout_get", "svgp_gp_stats_accumulate", "svgp_mnist_cache_workspace_elems",
               "svgp_mnist_cache_build", "svgp_mnist_generate_workspace_elems", "svgp_mnist_generate",
               "svgp_mnist_generate_route")
FAKE = 4096                         # never dereferenced: every call below fails validation first
GEMM_ROUTE = ["k_generate_kx", "svgp_dgemm_batched", "svgp_dgemm_batched", "k_generate_rowsum", "k_generate"]


def _cfg(b=4, m=12, L=3, M=4, n_obj=20, **kw):
    base = dict(b=b, b_global=b, m=m, L=L, M=M, n_obj=n_obj, N_train=100.0, jitter=1e-6, rep_weight=1.0)
    base.update(kw)
    return MnistCfg(**base)


def _generate(q, theta=FAKE, cache=FAKE, aux=FAKE, gather=1, images=FAKE, work=FAKE):
    return _lib.call("svgp_mnist_generate", None if q is None else C.byref(q), theta, cache, aux, gather, None, images, None, None,
                     work, None)


def _route(q):
    buf = C.create_string_buffer(512)
    _lib.call("svgp_mnist_generate_route", C.byref(q), buf, len(buf))
    return buf.value.decode().split()


def test_header_declares_and_library_exports_the_new_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svgpvae_hip.h")).read(), flags=re.S)
    lib = svgp_vae_amd.load_library()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", src), f"{n} not declared in include/svgpvae_hip.h"
        assert hasattr(lib, n), f"{n} not exported"
        assert n in _lib.SIGNATURES or n in _lib.NON_STATUS
    assert lib.svgp_struct_sizeof(11) == C.sizeof(CacheLayout)
    assert lib.svgp_struct_sizeof(12) == -1


@pytest.mark.parametrize("kw,message", [(dict(m=2049), "m=2049"), (dict(L=65), "L=65"), (dict(M=129), "M=129")])
def test_shapes_past_the_ceilings_are_unsupported(kw, message):
    lib = svgp_vae_amd.load_library()
    q = _cfg(**kw)
    calls = [lambda: lib.svgp_mnist_cache_layout_get(C.byref(q), C.byref(CacheLayout())),
             lambda: lib.svgp_gp_stats_accumulate(C.byref(q), FAKE, FAKE, 1, None),
             lambda: lib.svgp_mnist_cache_build(C.byref(q), FAKE, FAKE, FAKE, None),
             lambda: lib.svgp_mnist_generate(C.byref(q), FAKE, FAKE, FAKE, 1, None, FAKE, None, None, FAKE, None),
             lambda: lib.svgp_mnist_generate_route(C.byref(q), C.create_string_buffer(64), 64)]
    for f in calls:
        assert f() == -2                                         # SVGP_ERR_UNSUPPORTED
        assert message in lib.svgp_last_error().decode()
    assert lib.svgp_mnist_generate_workspace_elems(C.byref(q)) == 0 == lib.svgp_mnist_cache_workspace_elems(C.byref(q))


def test_invalid_arguments_are_refused_with_their_message():
    lib = svgp_vae_amd.load_library()
    big = _cfg(m=65, L=4, M=16, n_obj=40)
    cases = [
        (lambda: _generate(_cfg(b=0)), "need 1 <= b"),
        (lambda: _generate(None), "cfg is NULL"),
        (lambda: _generate(_cfg(), theta=None), "NULL device pointer"),
        (lambda: _generate(_cfg(), cache=None), "NULL device pointer"),
        (lambda: _generate(_cfg(), aux=None), "NULL device pointer"),
        (lambda: _generate(_cfg(), images=None), "NULL device pointer"),
        (lambda: _generate(_cfg(n_obj=0), gather=1), "gather needs an object-vector table"),
        (lambda: _generate(big, work=None), "work is NULL"),
        (lambda: _lib.call("svgp_mnist_cache_build", C.byref(big), FAKE, FAKE, None, None), "work is NULL"),
        (lambda: _lib.call("svgp_mnist_cache_build", C.byref(_cfg()), None, FAKE, None, None), "NULL device pointer"),
        (lambda: _lib.call("svgp_mnist_cache_build", C.byref(_cfg()), FAKE, None, None, None), "NULL device pointer"),
        (lambda: _lib.call("svgp_gp_stats_accumulate", C.byref(_cfg()), None, FAKE, 1, None), "NULL device pointer"),
        (lambda: _lib.call("svgp_gp_stats_accumulate", C.byref(_cfg()), FAKE, None, 1, None), "NULL device pointer"),
        (lambda: _lib.call("svgp_mnist_cache_layout_get", C.byref(_cfg()), None), "out is NULL"),
        (lambda: _lib.call("svgp_mnist_generate_route", C.byref(_cfg()), None, 10), "bad argument"),
    ]
    for f, message in cases:
        with pytest.raises(_lib.SvgpError) as e:
            f()
        assert "status -1" in str(e.value) and message in str(e.value), (message, str(e.value))
    assert lib.svgp_mnist_generate_workspace_elems(C.byref(_cfg())) == 0      # m <= 64: no workspace, NULL accepted
    assert lib.svgp_mnist_generate_workspace_elems(C.byref(big)) > 0
    assert lib.svgp_mnist_cache_workspace_elems(C.byref(_cfg())) == 0 < lib.svgp_mnist_cache_workspace_elems(C.byref(big))


@pytest.mark.parametrize("m,L", [(1, 1), (5, 1), (12, 3), (32, 16), (64, 4), (65, 4), (2048, 64)])
def test_cache_layout_is_increasing_disjoint_and_aligned(m, L):
    cl = CacheLayout()
    _lib.call("svgp_mnist_cache_layout_get", C.byref(_cfg(m=m, L=L)), C.byref(cl))
    fields = [("acc_S", L * m * m), ("acc_v", L * m), ("acc_rows", 1), ("w", L * m), ("X", L * m * m)]
    end = 0
    for name, n in fields:
        off = getattr(cl, name)
        assert off >= end and off % 16 == 0, (name, off, end)
        end = off + n
    assert cl.total >= end and cl.total == (end + 15) // 16 * 16


def test_generation_workspace_follows_the_row_capacity():
    lib = svgp_vae_amd.load_library()
    n = lambda **kw: lib.svgp_mnist_generate_workspace_elems(C.byref(_cfg(m=65, L=4, M=16, n_obj=40, **kw)))
    assert n(b=7, b_cap=256) == n(b=256) > n(b=7)
    assert n(b=256) >= 256 * 65 + 4 * 256 * 65 + 2 * 256 * 4


@pytest.mark.parametrize("m", [1, 5, 32, 64])
def test_route_is_one_launch_up_to_64_inducing_points(m):
    assert _route(_cfg(m=m)) == ["k_generate"]


@pytest.mark.parametrize("m", [65, 2048])
def test_route_beyond_64_inducing_points(m):
    assert _route(_cfg(m=m, M=16)) == GEMM_ROUTE


# ---------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("case", list(GC.CASES))
def test_oracle_response_to_one_ulp_is_within_a_hundredth_of_the_bar(case):
    ref = GC.reference(case)
    p2, img2 = GC.one_ulp(case)
    ref2 = GC.oracle_outputs(case, p2, img2)
    for k in ("w", "X", "p_m", "p_v", "images", "images_mean"):
        assert torch.isfinite(ref[k]).all()
        e = H.relerr(ref2[k], ref[k])
        print(f"{case} {k}: oracle response {e:.2e}")
        assert e <= GC.TOL / 100, (case, k, e)


@pytest.mark.parametrize("case", list(GC.CASES))
def test_posterior_is_the_kernel_row_against_w_and_X(case):
    ref = GC.reference(case)
    p_m, p_v = GC.kernel_row_moments(case)
    e_m, e_v = H.relerr(p_m, ref["p_m"]), H.relerr(p_v, ref["p_v"])
    print(f"{case}: k.w {e_m:.2e}, k_xx + k X k {e_v:.2e}")
    assert e_m < GC.PATH_TOL and e_v < GC.PATH_TOL
    assert (ref["p_v"] > 0).all()


# ---------------------------------------------------------------------------------------------- checkpoints
def _stand_in(n=23, fill=0.0):
    f = lambda k: torch.full((k,), fill, dtype=torch.float64)
    return types.SimpleNamespace(pl=types.SimpleNamespace(n_total=n), theta=f(n), adam_m=f(n), adam_v=f(n), state=f(16))


def _write_checkpoint(path, n=23, seed=0):
    g = torch.Generator().manual_seed(seed)
    ck = {"theta": torch.randn(n, dtype=torch.float64, generator=g), "adam_m": torch.randn(n, dtype=torch.float64, generator=g),
          "adam_v": torch.rand(n, dtype=torch.float64, generator=g), "state": torch.randn(16, dtype=torch.float64, generator=g)}
    torch.save(ck, path)                                          # the driver's own call (MNIST_experiment.py)
    return ck


def test_checkpoint_round_trip_and_refusals(tmp_path):
    from svgp_vae_amd import checkpoint
    path = str(tmp_path / "model_7.pt")
    ck = _write_checkpoint(path)
    got = checkpoint.load(path)
    assert set(got) == {"theta", "adam_m", "adam_v", "state"}
    for k in ck:
        assert got[k].dtype == torch.float64 and torch.equal(got[k], ck[k])
    eng = _stand_in()
    checkpoint.restore(eng, path)
    for k in ck:
        assert torch.equal(getattr(eng, k), ck[k])
    other = _stand_in(n=29, fill=1.5)
    with pytest.raises(ValueError) as e:
        checkpoint.restore(other, path)
    assert "23" in str(e.value) and "29" in str(e.value)
    assert bool((other.theta == 1.5).all()) and bool((other.state == 1.5).all())        # refused before anything is copied
    torch.save({"theta": ck["theta"]}, str(tmp_path / "x.pt"))
    with pytest.raises(ValueError):
        checkpoint.load(str(tmp_path / "x.pt"))


def test_first_epoch_follows_the_file_name_and_the_parser_defaults():
    from svgp_vae_amd import checkpoint
    from svgp_vae_amd.MNIST_experiment import build_parser
    assert checkpoint.first_epoch_of("run/model_7.pt") == 8
    assert checkpoint.first_epoch_of("model_0.pt") == 1
    assert checkpoint.first_epoch_of("run/x.pt") == 0 == checkpoint.first_epoch_of("run/model_7.pt.bak")
    args = build_parser().parse_args([])
    assert args.restore is None and args.first_epoch is None
    args = build_parser().parse_args(["--restore", "r/model_3.pt", "--first_epoch", "2"])
    assert args.restore == "r/model_3.pt" and args.first_epoch == 2


@pytest.mark.parametrize("elbo", ["SVIGP_Hensman", "GPVAE_Casale"])
def test_drivers_without_resume_refuse_the_flags(elbo):
    from svgp_vae_amd.MNIST_experiment import main
    for extra in (["--restore", "run/model_1.pt"], ["--first_epoch", "2"]):
        with pytest.raises(NotImplementedError) as e:
            main(["--elbo", elbo] + extra)
        assert "--restore" in str(e.value) and elbo in str(e.value)


@pytest.mark.parametrize("first,expect", [(None, [0, 1, 2, 3]), (2, [2, 3])])
def test_run_sharded_epochs_starts_at_first_epoch(first, expect):
    import torch.distributed as dist
    from svgp_vae_amd.dp import DistContext, run_sharded_epochs
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    old = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT")}
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    ctx = DistContext(rank=0, world=1, backend="gloo", force=True).init()
    try:
        assert dist.is_initialized() and dist.get_world_size() == 1
        seen, started, ended = [], [], []

        def local_step(llo, lhi, lo, hi, epoch, i):
            seen.append((epoch, i, llo, lhi))
            return dict(elbo=1.0, recon_loss=2.0, c_ma=0.0, lagrange=1.0)

        kw = {} if first is None else dict(first_epoch=first)
        log = run_sharded_epochs(ctx, [(0, 4), (4, 6)], 4, local_step, N_train=6, say=lambda *_: None,
                                 on_epoch_start=started.append, on_epoch_end=lambda e, _log: ended.append(e), **kw)
        assert [e for e, i, _, _ in seen if i == 0] == expect
        assert seen == [(e, i, lo, hi) for e in expect for i, (lo, hi) in enumerate([(0, 4), (4, 6)])]
        assert started == ended == log["epoch"] == expect
    finally:
        ctx.close()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
