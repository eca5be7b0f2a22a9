"""The three Titsias stages through the C ABI (svgp_gp_titsias_stats / _fwd / _bwd, csrc/gp_titsias.hip), each on its own, against the
float64 restatement of oracle/staged_gp.py evaluated on the inputs read back from the workspace -- so a wrong S2, t2 or scalar
term shows where it is made, not only through the end-to-end ELBO -- and a check that each stage writes nowhere but its documented
outputs and scratch areas (the reverse stage aliases four scratch areas: W | cA | cB in ws.Knbar_part, Sb | Ssum | T1 | T2 in
ws.scr_mm, U in ws.scr_bm, Cb in ws.scr_bl).

Tolerances: S2 and v2 are plain sums, 1e-9 of max-abs (helpers.FWD_TOL).  What passes through Sigma2^-1 (the inverse, t2, the
log-determinants, v2.t2) and the row sum is held to max(1e-9, 20 x the restatement's own response to a one-ulp perturbation of
those inputs), computed on the CPU here; the five reverse increments to the same rule with 1e-7 (helpers.GRAD_TOL)."""
import ctypes as C

import pytest
import torch

from oracle import staged_gp as SG
from svgp_vae_amd import _lib
from tests import helpers as H
from tests import titsias_cases as TC

pytestmark = pytest.mark.gpu
DT = torch.float64
_COUNTS = ("statA_len", "stat_parts", "statB_len", "n_part", "n_post", "gradC_len", "xpack_len", "total")
WRITES = {"stats": ("scr_bl", "scr_bm", "tit_S2", "tit_v2"),
          "fwd": ("tit_Si", "tit_t", "tit_scal", "scr_inv"),
          "bwd": ("scr_mm", "scr_bm", "scr_bl", "Knbar_part", "ybar", "s2bar", "Knbar", "knnbar", "Kbar")}


def _extent(wl, name):
    """[start, end) of a workspace field: it ends where the next field of the layout begins."""
    offs = sorted({getattr(wl, f) for f in _lib.WS_FIELDS if f not in _COUNTS} | {wl.total})
    off = getattr(wl, name)
    return off, next(o for o in offs if o > off)


def _call_and_check_writes(eng, stage, *args):
    """Runs one stage; every element of the workspace outside the stage's documented areas must keep its bits."""
    before = eng.ws.clone()
    torch.cuda.synchronize()           # the copy ran on torch's stream, the stage runs on the engine's
    _lib.call("svgp_gp_titsias_" + stage, C.byref(eng.cfg), eng.ws.data_ptr(), *args, eng.stream.cuda_stream)
    torch.cuda.synchronize()
    keep = torch.ones(eng.ws.numel(), dtype=torch.bool, device=eng.ws.device)
    for f in WRITES[stage]:
        lo, hi = _extent(eng.wl, f)
        keep[lo:hi] = False
    changed = (before.view(torch.int64) != eng.ws.view(torch.int64)) & keep
    if bool(changed.any()):
        at = int(changed.nonzero()[0])
        owner = max((f for f in _lib.WS_FIELDS if f not in _COUNTS and getattr(eng.wl, f) <= at), key=lambda f: getattr(eng.wl, f))
        pytest.fail(f"svgp_gp_titsias_{stage} changed {int(changed.sum())} elements outside its areas, first at ws[{at}] (in {owner})")


def _ulp(t, gen):
    return t * (1.0 + 2.0 ** -52 * (torch.randint(0, 2, t.shape, generator=gen).to(DT) * 2 - 1))


@pytest.mark.parametrize("case", TC.STAGE_CASES)
def test_each_stage_matches_the_restatement_and_writes_only_its_areas(case):
    cs = TC.CASES[case]
    b, m, L, j = cs["b"], cs["m"], cs["L"], cs["jitter"]
    eng = TC.engine(case)
    TC.step(eng, *TC.rows_of(case)[1:])            # one step without Adam: the workspace holds real inputs
    wl, ws = eng.wl, eng.ws
    rd = lambda name, shp: eng.ws_view(name, shp).cpu().clone()
    t = dict(y=rd("qnet_mu", (b, L)), var=rd("qnet_var", (b, L)), K=rd("K", (m, m)), Kn=rd("Kn", (b, m)), knn=rd("knn", (b,)))
    q, S = rd("q", (b,)), rd("S", (L, m, m))
    assert H.relerr(S, torch.einsum('nl,ni,nj->lij', 1.0 / t["var"], t["Kn"], t["Kn"])) < H.FWD_TOL      # what the reverse stage sums
    for f, n in (("tit_S2", L * m * m), ("tit_v2", L * m), ("tit_Si", L * m * m), ("tit_t", L * m), ("tit_scal", 2 * L + 1)):
        ws[getattr(wl, f):getattr(wl, f) + n] = float("nan")
    torch.cuda.synchronize()
    st = eng.state.data_ptr()
    bad = []

    def check(name, got, want, tol):
        e = H.relerr(got, want)
        print(f"{case} {name}: {e:.2e} (bound {tol:.1e})")
        if not (bool(torch.isfinite(torch.as_tensor(got)).all()) and e <= tol):
            bad.append(f"{name}: {e:.3e} > {tol:.1e}")

    # ---- statistics
    _call_and_check_writes(eng, "stats")
    S2w, v2w = SG.titsias_stats(t["Kn"], t["y"], t["var"], j)
    S2, v2 = rd("tit_S2", (L, m, m)), rd("tit_v2", (L, m))
    check("S2", S2, S2w, H.FWD_TOL)
    check("v2", v2, v2w, H.FWD_TOL)
    # ---- forward: the restatement on the stage's own inputs (S2, v2 as the GPU left them), and its one-ulp response
    _call_and_check_writes(eng, "fwd", st)
    want = SG.titsias_fwd(t["K"], S2, v2, t["y"], t["var"], t["knn"], q, j)
    gen = torch.Generator().manual_seed(17)
    want2 = SG.titsias_fwd(_ulp(t["K"], gen), _ulp(S2, gen), _ulp(v2, gen), _ulp(t["y"], gen), _ulp(t["var"], gen), _ulp(t["knn"], gen),
                           _ulp(q, gen), j)
    scal = rd("tit_scal", (2 * L + 1,))
    got = (rd("tit_Si", (L, m, m)), scal[:L], rd("tit_t", (L, m)), scal[L:2 * L], scal[2 * L])
    for name, g, w, w2 in zip(("Sigma2^-1", "log det Sigma2", "t2", "v2.t2", "row sum"), got, want, want2):
        check(name, g, w, max(H.FWD_TOL, 20 * H.relerr(w2, w)))
    # ---- reverse: the increments from zero against g2 x autograd of sum_l L_2
    for f, n in (("ybar", b * L), ("s2bar", b * L), ("Knbar", b * m), ("knnbar", b), ("Kbar", m * m)):
        ws[getattr(wl, f):getattr(wl, f) + n] = 0.0
    torch.cuda.synchronize()
    _call_and_check_writes(eng, "bwd", st)
    g2 = -1.0 if cs["geco"] else -TC.BETA / L
    names = ("y", "var", "Kn", "knn", "K")

    def autograd(tt):
        leaf = {k: v.clone().requires_grad_(True) for k, v in tt.items()}
        tot = SG.titsias_l2_sum(leaf["Kn"], leaf["K"], leaf["knn"], leaf["y"], leaf["var"], j)
        return [g2 * g for g in torch.autograd.grad(tot, [leaf[k] for k in names])]

    gw, gw2 = autograd(t), autograd({k: _ulp(v, gen) for k, v in t.items()})
    for (f, shp), w, w2 in zip((("ybar", (b, L)), ("s2bar", (b, L)), ("Knbar", (b, m)), ("knnbar", (b,)), ("Kbar", (m, m))), gw, gw2):
        check(f, rd(f, shp), w, max(H.GRAD_TOL, 20 * H.relerr(w2, w)))
    assert not bad, "\n".join(bad)
