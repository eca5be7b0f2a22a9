"""CPU-side checks of the global-memory exact per-video GP (pearce_long.hip): the ABI, the argument refusals (each with its
message, before any launch) and the oracle's own response at every case of tests/ball_long_cases.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import svgp_vae_amd
from svgp_vae_amd import _lib
from svgp_vae_amd._lib import PearceBufs
from tests import ball_cases as BC
from tests import ball_long_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("svgp_pearce_long_workspace_elems", "svgp_pearce_long_fwd", "svgp_pearce_long_bwd")
FAKE = 4096                                                     # never dereferenced: every case fails validation first


def test_header_declares_and_library_exports_the_long_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svgpvae_hip.h")).read(), flags=re.S)
    lib = svgp_vae_amd.load_library()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", src), f"{n} not declared in include/svgpvae_hip.h"
        assert hasattr(lib, n), f"{n} not exported"
        assert n in _lib.SIGNATURES or n in _lib.NON_STATUS


def _bufs(B, T, n, idx=None, fill=True):
    q = PearceBufs(B=B, T=T, n=n)
    if fill:
        for name, _ in PearceBufs._fields_[3:]:
            setattr(q, name, FAKE)
        q.idx, q.tmask = idx, None
    return q


def _fwd(q, work=FAKE):
    _lib.call("svgp_pearce_long_fwd", C.byref(q), FAKE, FAKE, FAKE, work, None)


def _bwd(q, work=FAKE):
    _lib.call("svgp_pearce_long_bwd", C.byref(q), 1.0, 0, 1, FAKE, FAKE, FAKE, work, None)


@pytest.mark.parametrize("run", [_fwd, _bwd])
def test_bad_arguments_are_refused_with_their_message(run):
    lib = svgp_vae_amd.load_library()
    with pytest.raises(svgp_vae_amd.SvgpError, match="T=2049"):
        run(_bufs(2, 2049, 2049))
    rc = lib.svgp_pearce_long_fwd(C.byref(_bufs(2, 2049, 2049, fill=False)), None, None, None, None, None)
    assert rc == -2, rc                                         # SVGP_ERR_UNSUPPORTED, before any pointer is looked at
    with pytest.raises(svgp_vae_amd.SvgpError, match="bad shape B=2 T=65 n=0"):
        run(_bufs(2, 65, 0))
    with pytest.raises(svgp_vae_amd.SvgpError, match="bad shape B=2 T=65 n=66"):
        run(_bufs(2, 65, 66, idx=FAKE))
    with pytest.raises(svgp_vae_amd.SvgpError, match="bad shape B=0"):
        run(_bufs(0, 65, 65))
    with pytest.raises(svgp_vae_amd.SvgpError, match="index set"):
        run(_bufs(2, 65, 12))                                   # a context set needs its index list
    with pytest.raises(svgp_vae_amd.SvgpError, match="NULL device pointer"):
        run(_bufs(2, 65, 65), work=None)
    for field in ("times", "ls_y", "s2_x", "Ai", "alpha", "lh"):
        q = _bufs(2, 65, 65)
        setattr(q, field, None)
        with pytest.raises(svgp_vae_amd.SvgpError, match="NULL device pointer"):
            run(q)
    with pytest.raises(svgp_vae_amd.SvgpError, match="bufs is NULL"):
        _lib.call("svgp_pearce_long_fwd", None, None, None, FAKE, FAKE, None)


def test_forward_and_reverse_check_the_pointers_only_they_need():
    q = _bufs(2, 65, 65)
    q.row_ce = None
    with pytest.raises(svgp_vae_amd.SvgpError, match="NULL device pointer"):
        _fwd(q)
    with pytest.raises(svgp_vae_amd.SvgpError, match="both eps"):
        _lib.call("svgp_pearce_long_fwd", C.byref(_bufs(2, 65, 65)), FAKE, None, FAKE, FAKE, None)
    q = _bufs(2, 65, 65)
    q.zbar_y = None
    with pytest.raises(svgp_vae_amd.SvgpError, match="NULL device pointer"):
        _bwd(q)
    # the length-scale outputs are needed when they are asked for (and always by a context set)
    with pytest.raises(svgp_vae_amd.SvgpError, match="NULL device pointer"):
        _lib.call("svgp_pearce_long_bwd", C.byref(_bufs(2, 65, 65)), 1.0, 0, 1, FAKE, None, None, FAKE, None)
    with pytest.raises(svgp_vae_amd.SvgpError, match="NULL device pointer"):
        _lib.call("svgp_pearce_long_bwd", C.byref(_bufs(2, 65, 12, idx=FAKE)), -1.0, 1, 0, FAKE, None, None, FAKE, None)


def test_workspace_grows_with_the_video_length_and_with_the_length_scale_gradient():
    ws = svgp_vae_amd.load_library().svgp_pearce_long_workspace_elems
    sizes = [ws(4, T, T, 0) for T in (1, 33, 64, 65, 130, 511, 512, 2048)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    for T in (65, 257, 513, 2048):
        assert ws(4, T, T, 1) > ws(4, T, T, 0)
        assert ws(4, T, T, 1) >= 2 * 2 * 4 * T * T                    # D Ai and Ai D Ai
        assert ws(4, T, 7, 0) < ws(4, T, T, 0)                        # a context set needs less
        assert ws(8, T, T, 0) > ws(4, T, T, 0)
    for bad in ((4, 2049, 2049, 0), (4, 65, 0, 0), (4, 65, 66, 0), (0, 65, 65, 0)):
        assert ws(*bad) == 0


def test_the_long_engine_needs_a_gpu_and_keeps_the_lds_engine_limit():
    from svgp_vae_amd import ball
    assert ball.pearce_engine_class(64) is ball.PearceStepEngine and ball.pearce_engine_class(65) is ball.PearceLongStepEngine
    with pytest.raises(svgp_vae_amd.SvgpError, match="tmax=2049"):
        ball.PearceLongStepEngine("VAE", 0.001, batch=4, tmax=2049, px=8, py=8, hidden=8)
    with pytest.raises(svgp_vae_amd.SvgpError, match="tmax <= 64"):
        ball.PearceStepEngine("VAE", 0.001, batch=4, tmax=65, px=8, py=8, hidden=8)
    if not torch.cuda.is_available():
        with pytest.raises(svgp_vae_amd.SvgpError, match="no CPU execution path"):
            ball.PearceLongStepEngine("VAE", 0.001, batch=4, tmax=80, px=8, py=8, hidden=8)


@pytest.mark.parametrize("case", list(LC.LONG_CASES))
def test_oracle_is_finite_and_well_conditioned_at_every_case(case):
    """The guard that the inputs stay benign if someone edits the table: the GPU test's bars assume cond(A) of a few tens."""
    cs = LC.LONG_CASES[case]
    p, vid, eps, ran_ind, out, grads = LC.long_reference(case)
    for i, o in enumerate(out[:8]):
        assert torch.isfinite(o).all(), (case, i)
    for k, g in grads.items():
        assert torch.isfinite(g).all(), (case, k)
    assert float(out[4].min()) > 0                                       # posterior variances
    T = cs["tmax"]
    t = torch.arange(T, dtype=BC.DT)
    worst = 0.0
    for c, lk in enumerate(("l_x", "l_y")):
        K = torch.exp(-0.5 * (t[:, None] - t[None, :]) ** 2 / p[lk] ** 2)
        Kc = torch.exp(-0.5 * (t[:, None] - t[None, :]) ** 2 / cs["lt"] ** 2)
        for b in range(cs["batch"]):
            s2 = out[6][b, :, c]
            worst = max(worst, float(np.linalg.cond((K + torch.diag(s2)).numpy())))
            if ran_ind is not None:
                ix = ran_ind[b, :cs["con_tf"]]
                worst = max(worst, float(np.linalg.cond((Kc[ix][:, ix] + torch.diag(s2[ix])).numpy())))
    print(f"{case}: worst cond(A) {worst:.1f}")
    assert worst < 1e3
