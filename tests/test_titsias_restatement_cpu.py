"""The m x m restatement of the Titsias L_2 (oracle/staged_gp.py: titsias_stats, titsias_fwd, titsias_l2_sum -- the Woodbury form of
csrc/gp_titsias.hip) pinned against the oracle's literal branch (MnistSVGP.variational_loss: the b x b covariance, its inverse and
its Cholesky factor per channel) at the envelope's cases: the two identities the stages rest on, the sum over channels, and the
gradients with respect to the five inputs the reverse stage adds to (y, var, Kn, knn, K).

Bounds: a tenth of the bars of tests/titsias_cases.py, the room its guard leaves between two correct float64 evaluations: 1e-9
relative to max(1, |want|) for scalars, 1e-7 of the tensor's max-abs for gradients.  m520, the case marked ill-conditioned, is
held to 20 x the literal branch's own response to a one-ulp change of K, Kn, y and var where that is more."""
import pytest
import torch

from oracle import staged_gp as SG
from oracle import svgpvae_oracle as O
from tests import helpers as H
from tests import titsias_cases as TC

DT = torch.float64
NAMES = ("y", "var", "Kn", "knn", "K")


class _FixedKernel(O.MnistSVGP):
    """The literal branch on given kernel matrices, so that autograd reaches them."""

    def __init__(self, K, Kn, knn, jitter):
        super().__init__(True, torch.zeros(K.shape[0], 3, dtype=DT), None, None, None, jitter, TC.N_TRAIN)
        self.mats = (K, Kn, knn)

    def kernel_matrix(self, x, y, x_inducing=True, y_inducing=True, diag_only=False):
        K, Kn, knn = self.mats
        return knn if diag_only else (K if x_inducing else Kn)


def _inputs(case):
    cs = TC.CASES[case]
    params, images, aux, _ = TC.problem(case)
    y, var = O.MnistVAE(params, cs["L"]).encode(images)
    if cs["clip_qs"]:
        var = O.clip_by_value(var, 1e-3, 10.0)
    K, Kn, knn = SG.kernel_matrix_fwd(aux, params["inducing_index_points"], params.get("object_vectors"), params["l_GP"],
                                      params["amplitude"], cs["normalize"])
    return dict(y=y.detach(), var=var.detach(), Kn=Kn, knn=knn, K=K)


def _literal(t, jitter):
    """(sum_l L_2, per-channel log det C, per-channel y^T C^-1 y, gradients of the sum) of the literal branch."""
    leaf = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    svgp = _FixedKernel(leaf["K"], leaf["Kn"], leaf["knn"], jitter)
    b, L = t["y"].shape
    tot = sum(svgp.variational_loss(torch.zeros(b, 3, dtype=DT), leaf["y"][:, l], None, None, leaf["var"][:, l])[0]
              for l in range(L))
    with torch.no_grad():
        C = torch.diag_embed(t["var"].T + jitter) + (t["Kn"] @ torch.linalg.inv(t["K"] + jitter * torch.eye(t["K"].shape[0], dtype=DT))
                                                     @ t["Kn"].T)[None]
        ldC = 2 * torch.log(torch.diagonal(torch.linalg.cholesky(C), dim1=-2, dim2=-1)).sum(-1)
        quad = torch.einsum('nl,lnk,kl->l', t["y"], torch.linalg.inv(C), t["y"])
    g = torch.autograd.grad(tot, [leaf[k] for k in NAMES])
    return tot.detach(), ldC, quad, dict(zip(NAMES, g))


@pytest.mark.parametrize("case", TC.ENVELOPE_CASES)
def test_restatement_matches_the_literal_branch(case):
    cs, t = TC.CASES[case], _inputs(case)
    j = cs["jitter"]
    want, ldC, quad, wg = _literal(t, j)
    tol_s, tol_g = TC.SCALAR_TOL / 10, {k: TC.GRAD_TOL / 10 for k in NAMES}
    if cs["ill"]:
        ulp = 1.0 + 2.0 ** -52
        w2, _, _, g2 = _literal({k: (v if k == "knn" else v * ulp) for k, v in t.items()}, j)
        tol_s = max(tol_s, 20 * abs(float(w2 - want)) / max(1.0, abs(float(want))))
        tol_g = {k: max(tol_g[k], 20 * H.relerr(g2[k], wg[k])) for k in NAMES}
    leaf = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    got = SG.titsias_l2_sum(leaf["Kn"], leaf["K"], leaf["knn"], leaf["y"], leaf["var"], j)
    gg = dict(zip(NAMES, torch.autograd.grad(got, [leaf[k] for k in NAMES])))
    # the two identities of the header of gp_titsias.hip, per channel, from the stage functions
    Kj = t["K"] + j * torch.eye(cs["m"], dtype=DT)
    ldK = 2 * torch.log(torch.diagonal(torch.linalg.cholesky(Kj))).sum()
    q = ((t["Kn"] @ torch.linalg.inv(Kj)) * t["Kn"]).sum(1)
    S2, v2 = SG.titsias_stats(t["Kn"], t["y"], t["var"], j)
    _, ld2, _, vt, _ = SG.titsias_fwd(t["K"], S2, v2, t["y"], t["var"], t["knn"], q, j)
    d = t["var"] + j
    bad = []
    for name, a, w in (("sum_l L_2", got.detach(), want), ("log det C", torch.log(d).sum(0) + ld2 - ldK, ldC),
                       ("y^T C^-1 y", (t["y"] ** 2 / d).sum(0) - vt, quad)):
        e = float(((a - w).abs() / w.abs().clamp(min=1.0)).max())
        print(f"{case} {name}: {e:.2e}")
        if not e <= tol_s:
            bad.append(f"{name}: {e:.3e} > {tol_s:.1e}")
    for k in NAMES:
        e = H.relerr(gg[k], wg[k])
        print(f"{case} d/d{k}: {e:.2e}")
        if not e <= tol_g[k]:
            bad.append(f"gradient {k}: {e:.3e} > {tol_g[k]:.1e}")
    assert not bad, "\n".join(bad)
