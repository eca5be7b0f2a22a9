"""Case table, problems and engine builder of the global-memory exact per-video GP (PearceLongStepEngine, pearce_long.hip),
shared by tests/test_gpu_ball_long.py (GPU) and tests/test_ball_long_cpu.py (the oracle's own response at every case).

Problems are tests/ball_cases.py's `_problem` at 8 x 8 frames, hidden 16, beta 0.9, seed 60 + tmax, with the length scales set
as `pearce_problem` sets them (--GP_joint: l_x = 1.2 lt, l_y = 0.9 lt; else both lt); NP permutations from generator seed 9.
Each case is the smallest shape that reaches a distinct branch.  Tolerances: ball_cases.OUT_TOL / ELBO_TOL / GRAD_TOL."""
import functools

import torch

from tests import ball_cases as BC
from tests.ball_cases import DT, _problem

LONG_CASES = {
    # first size the LDS engine refuses; the blocked inverse runs 3 blocks of 32 with a 1-row edge
    "T65": dict(batch=5, tmax=65, type_elbo="GPVAE_Pearce", lt=2.0, joint=True, con_tf=None),
    # the reference's batch; reverse pass without the GEMM; l_* gradients exactly 0
    "T96_fixed": dict(batch=35, tmax=96, type_elbo="GPVAE_Pearce", lt=2.0, joint=False, con_tf=None),
    # context set on the blocked path, accumulating scatter, c_dl
    "T130_np": dict(batch=4, tmax=130, type_elbo="NP", lt=2.0, joint=True, con_tf=67),
    "T66_np_c2": dict(batch=4, tmax=66, type_elbo="NP", lt=2.0, joint=True, con_tf=2),       # smallest context set
    "T66_np_c64": dict(batch=4, tmax=66, type_elbo="NP", lt=2.0, joint=True, con_tf=64),     # two target frames
    "T129_vae": dict(batch=3, tmax=129, type_elbo="VAE", lt=0.001, joint=False, con_tf=None),  # near-diagonal K
    "T257": dict(batch=3, tmax=257, type_elbo="GPVAE_Pearce", lt=5.0, joint=True, con_tf=None),  # one row past 256
    "T513": dict(batch=2, tmax=513, type_elbo="GPVAE_Pearce", lt=2.0, joint=True, con_tf=None),  # potrf + potri inverse
    # full set on the Cholesky branch of the inverse, context set on the Gauss-Jordan one
    "T513_np": dict(batch=2, tmax=513, type_elbo="NP", lt=2.0, joint=True, con_tf=300),
}
# sizes the LDS kernels run too: the problems (and shared references) of ball_cases.PEARCE_ENV_CASES
CMP_CASES = ("T33", "T64")


def long_problem(case):
    cs = LONG_CASES[case]
    batch, T, lt = cs["batch"], cs["tmax"], cs["lt"]
    p, vid, eps = _problem(batch, T, BC.ENV_PX, BC.ENV_HIDDEN, 4, seed=60 + T)
    p = {k: v for k, v in p.items() if not k.startswith("ip_")}
    p["l_x"] = torch.tensor(lt * (1.2 if cs["joint"] else 1.0), dtype=DT)
    p["l_y"] = torch.tensor(lt * (0.9 if cs["joint"] else 1.0), dtype=DT)
    ran_ind = None
    if cs["type_elbo"] == "NP":
        g = torch.Generator().manual_seed(9)
        ran_ind = torch.stack([torch.randperm(T, generator=g) for _ in range(batch)])
    return p, vid, eps, ran_ind


@functools.lru_cache(maxsize=None)
def long_reference(case):
    """(params, videos, eps, ran_ind, oracle outputs, oracle gradients) of a LONG_CASES entry; computed once per process and
    shared: callers must not write to it."""
    p, vid, eps, ran_ind = long_problem(case)
    out, _, grads = BC.pearce_oracle(LONG_CASES[case], p, vid, eps, ran_ind)
    return p, vid, eps, ran_ind, out, grads


def long_engine(p, type_elbo, lt, GP_joint, batch, T, px, hidden, beta, **kw):
    from svgp_vae_amd import ball
    flat = {k: (v.reshape(-1) if k.startswith(("encB", "decB", "l_")) else v) for k, v in p.items()}
    return ball.PearceLongStepEngine(type_elbo, lt, 0.5, GP_joint, 2.0, batch=batch, tmax=T, px=px, py=px, hidden=hidden,
                                     beta=beta, params=flat, **kw)
