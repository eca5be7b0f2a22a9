"""Cases, builders and the float64 reference of the posterior cache / conditional generation tests
(tests/test_generate_cpu.py, tests/test_gpu_generate.py).

Reference: the oracle's MnistSVGP.approximate_posterior_params, batching_encode_SVGPVAE,
bacthing_predict_SVGPVAE_rotated_mnist and MnistVAE.decode; w and X are restated from their formulas with torch.linalg.inv:

    Sigma_l = K_mm + c S_l,  S_l = K_mn diag(1/var_l) K_nm,  v_l = K_mn (mu_l / var_l),  c = N_train / rows
    w_l = c (Sigma_l + jI)^-1 v_l          X_l = (Sigma_l + jI)^-1 - (K_mm + jI)^-1

Bars (the project's own, tests/casale_cases.py, tests/test_gpu_api.py::test_bacthing_predict_conditional_generation; relative to
the tensor's max-abs, helpers.relerr): p_m, p_v, images, w, X against the oracle 1e-8; two HIP paths against each other 1e-10.
They hold only where the oracle's own response to a one-ulp change of its inputs stays within 1/100 of the bar, which
test_generate_cpu.py asserts for every case below (the shape of case D with M = 8 responds with 1.2e-10 and is no case)."""
import functools

import torch

from oracle import svgpvae_oracle as O
from tests import helpers as H

DT = torch.float64
TOL, PATH_TOL = 1e-8, 1e-10
JITTER = 1e-6

# name -> m, L, M, n_obj, train rows, query rows, table.  E is the first shape on the GEMM path; A and B have m neither a
# multiple of 4 nor of 16; F has no object-vector table (gather = 0: the object vector is the query row's own columns); G asks
# for the largest LDS of the fused launch (m = 64, L = 64: 151 632 bytes).
CASES = {
    "A": dict(m=5, L=1, M=2, n_obj=6, rows=37, q=3, table=True),
    "B": dict(m=12, L=3, M=4, n_obj=20, rows=37, q=5, table=True),
    "C": dict(m=32, L=16, M=8, n_obj=40, rows=150, q=7, table=True),
    "D": dict(m=64, L=4, M=16, n_obj=40, rows=150, q=7, table=True),
    "E": dict(m=65, L=4, M=16, n_obj=40, rows=150, q=7, table=True),
    "F": dict(m=12, L=3, M=4, n_obj=0, rows=37, q=5, table=False),
    "G": dict(m=64, L=64, M=16, n_obj=40, rows=150, q=7, table=True),
}
SEED = dict(A=1, B=2, C=3, D=4, E=5, F=6, G=7)


@functools.lru_cache(maxsize=None)
def problem(case):
    """(params, train images, train aux, query aux, query eps) of a case; float64 CPU tensors, never modified."""
    cs = CASES[case]
    n = cs["rows"] + cs["q"]
    params, images, aux, eps = H.toy_problem(b=n, m=cs["m"], L=cs["L"], M=cs["M"], n_obj=cs["n_obj"], seed=SEED[case],
                                             with_table=cs["table"])
    r = cs["rows"]
    return params, images[:r].contiguous(), aux[:r].contiguous(), aux[r:].contiguous(), eps[r:].contiguous()


def oracle_models(case, params=None):
    cs = CASES[case]
    params = problem(case)[0] if params is None else params
    return O.make_models(params, False, JITTER, float(cs["rows"]), cs["L"])


def oracle_outputs(case, params=None, images=None):
    """dict(w, X, p_m, p_v, images, images_mean, qnet_mu, qnet_var) of the oracle for a case (optionally at other parameters /
    train images: the one-ulp response)."""
    cs = CASES[case]
    p0, img, aux, qaux, eps = problem(case)
    params = p0 if params is None else params
    img = img if images is None else images
    vae, svgp = oracle_models(case, params)
    mu, var, _ = O.batching_encode_SVGPVAE((img, aux), vae, clipping_qs=True)
    ip = params["inducing_index_points"]
    K = svgp.kernel_matrix(ip, ip)
    Kn = svgp.kernel_matrix(aux, ip, x_inducing=False)
    eye = torch.eye(cs["m"], dtype=DT)
    Ki = torch.linalg.inv(K + JITTER * eye)
    c = float(cs["rows"]) / aux.shape[0]
    w, X, p_m, p_v = [], [], [], []
    for l in range(cs["L"]):
        prec = O.reciprocal_no_nan(var[:, l])
        Si = torch.linalg.inv(K + c * (Kn.T @ (Kn * prec[:, None])) + JITTER * eye)
        w.append(c * (Si @ (Kn.T @ (prec * mu[:, l]))))
        X.append(Si - Ki)
        pm, pv, _, _ = svgp.approximate_posterior_params(qaux, aux, mu[:, l], var[:, l])
        p_m.append(pm); p_v.append(pv)
    p_m, p_v = torch.stack(p_m, 1), torch.stack(p_v, 1)
    zeros = torch.zeros(cs["q"], 28, 28, 1, dtype=DT)
    recon, _ = O.bacthing_predict_SVGPVAE_rotated_mnist((zeros, qaux), vae, svgp, mu, var, aux, epsilon=eps)
    return dict(w=torch.stack(w), X=torch.stack(X), p_m=p_m, p_v=p_v, images=recon, images_mean=vae.decode(p_m),
                qnet_mu=mu, qnet_var=var)


@functools.lru_cache(maxsize=None)
def reference(case):
    return oracle_outputs(case)


def one_ulp(case):
    """The case's parameters and train images with every value moved by one ulp up or down (ids stay integers)."""
    params, img, _, _, _ = problem(case)
    gen = torch.Generator().manual_seed(17)
    ulp = lambda t: t * (1.0 + 2.0 ** -52 * (torch.randint(0, 2, t.shape, generator=gen).to(DT) * 2 - 1))
    p2 = {k: ulp(v) for k, v in params.items()}
    p2["inducing_index_points"][:, 0] = params["inducing_index_points"][:, 0]
    return p2, ulp(img)


def kernel_row_moments(case):
    """p_m = k . w, p_v = k_xx + k^T X k from the restated w, X: the algebra the cache rests on."""
    cs = CASES[case]
    params, _, _, qaux, _ = problem(case)
    ref = reference(case)
    _, svgp = oracle_models(case)
    ip = params["inducing_index_points"]
    k = svgp.kernel_matrix(qaux, ip, x_inducing=False)
    kxx = svgp.kernel_matrix(qaux, qaux, False, False, diag_only=True)
    p_m = torch.stack([k @ ref["w"][l] for l in range(cs["L"])], 1)
    p_v = torch.stack([kxx + ((k @ ref["X"][l]) * k).sum(1) for l in range(cs["L"])], 1)
    return p_m, p_v
