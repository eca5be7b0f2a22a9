"""The library-call order of one moving-ball step and of one `predict`: the four training engines and the two predictors, with
the module-level `call` of ball.py / ball_predict.py replaced by a recorder that notes the entry name and calls through.  The
oracle suites (test_gpu_ball*.py, test_gpu_*predict.py) check that every pointer is the right one; this file pins the order.

The expected lists were recorded from the host code as it stood before the four engines shared one step body and are spelled out
per case below, so that each can be read against that body: encode, head, GP forward, pack, decode + reconstruction term,
decoder reverse, unpack, GP reverse, head reverse, encoder reverse, clip / Adam, assemble, finalize.  The order does not depend on
size, so the shapes are the smallest every kernel involved accepts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, PX, HIDDEN, M, Q = 2, 5, 4, 8, 3, 3

# ---- the pieces of a step, in the words of the library
GEMM = "svgp_dgemm_splitk"
ENCODE = [GEMM, "svgp_bias_act_fwd", GEMM]
HEAD_FWD, HEAD_BWD = ["svgp_ball_head_fwd"], ["svgp_ball_head_bwd"]
PACK, UNPACK = ["svgp_ball_pack_z"], ["svgp_ball_unpack_zbar"]
DECODE = [GEMM, "svgp_bias_act_fwd", GEMM, "svgp_bias_act_fwd"]
RECON = DECODE + ["svgp_sigmoid_xent"]
SCALE_ROWS = ["svgp_scale_rows"]                              # NP: target frames only, when there is a reverse pass
DEC_BWD = [GEMM, "svgp_act_bwd_bias", GEMM, "svgp_act_bwd_bias", GEMM, GEMM]
ENC_BWD = [GEMM, "svgp_act_bwd_bias", GEMM, "svgp_act_bwd_bias", GEMM]
CLIP, ADAM = ["svgp_clip_by_value"], ["svgp_adam_tf1_step"]
RNG_BUMP = ["svgp_state_add"]
FINALIZE = ["svgp_ball_finalize"]
# one latent coordinate of the sparse GP on the LDS-resident stages
HENSMAN_FWD = ["svgp_se1d_kernel_matrix_fwd", "svgp_gp_stats_fwd", "svgp_gp_factor_fwd", "svgp_gp_posterior_fwd"]
TITSIAS_FWD = ["svgp_se1d_kernel_matrix_fwd", "svgp_gp_stats_fwd", "svgp_gp_titsias_stats", "svgp_gp_factor_fwd",
               "svgp_gp_posterior_fwd", "svgp_gp_titsias_fwd"]
HENSMAN_BWD = ["svgp_gp_stats_bwd", "svgp_gp_factor_bwd", "svgp_gp_posterior_bwd", "svgp_se1d_kernel_matrix_bwd"]
TITSIAS_BWD = ["svgp_gp_stats_bwd", "svgp_gp_factor_bwd", "svgp_gp_posterior_bwd", "svgp_gp_titsias_bwd",
               "svgp_se1d_kernel_matrix_bwd"]
# ... and on the global-memory ones (either ELBO branch: one call)
LARGE_FWD, LARGE_BWD = ["svgp_ball_large_gp_fwd"], ["svgp_ball_large_gp_bwd"]
ASM, LARGE_ASM, PEARCE_ASM = ["svgp_ball_elbo_assemble"], ["svgp_ball_large_elbo_assemble"], ["svgp_pearce_elbo_assemble"]


# (engine, titsias, "train" | "forward" | "clip": backward=True adam=True | backward=False | the former with clip_grad)
SPARSE_EXPECTED = {
    ("BallStepEngine", False, "train"): ENCODE + HEAD_FWD + HENSMAN_FWD + RNG_BUMP + HENSMAN_FWD + PACK + RECON + DEC_BWD + UNPACK
    + HENSMAN_BWD + HENSMAN_BWD + HEAD_BWD + ENC_BWD + ADAM + ASM + FINALIZE,
    ("BallStepEngine", False, "forward"): ENCODE + HEAD_FWD + HENSMAN_FWD + RNG_BUMP + HENSMAN_FWD + PACK + RECON + ASM + FINALIZE,
    ("BallStepEngine", False, "clip"): ENCODE + HEAD_FWD + HENSMAN_FWD + RNG_BUMP + HENSMAN_FWD + PACK + RECON + DEC_BWD + UNPACK
    + HENSMAN_BWD + HENSMAN_BWD + HEAD_BWD + ENC_BWD + CLIP + ADAM + ASM + FINALIZE,
    ("BallStepEngine", True, "train"): ENCODE + HEAD_FWD + TITSIAS_FWD + RNG_BUMP + TITSIAS_FWD + PACK + RECON + DEC_BWD + UNPACK
    + TITSIAS_BWD + TITSIAS_BWD + HEAD_BWD + ENC_BWD + ADAM + ASM + FINALIZE,
    ("BallStepEngine", True, "forward"): ENCODE + HEAD_FWD + TITSIAS_FWD + RNG_BUMP + TITSIAS_FWD + PACK + RECON + ASM + FINALIZE,
    ("BallLargeStepEngine", False, "train"): ENCODE + HEAD_FWD + LARGE_FWD + RNG_BUMP + LARGE_FWD + PACK + RECON + DEC_BWD + UNPACK
    + LARGE_BWD + LARGE_BWD + HEAD_BWD + ENC_BWD + ADAM + LARGE_ASM + FINALIZE,
    ("BallLargeStepEngine", False, "forward"): ENCODE + HEAD_FWD + LARGE_FWD + RNG_BUMP + LARGE_FWD + PACK + RECON + LARGE_ASM
    + FINALIZE,
    ("BallLargeStepEngine", False, "clip"): ENCODE + HEAD_FWD + LARGE_FWD + RNG_BUMP + LARGE_FWD + PACK + RECON + DEC_BWD + UNPACK
    + LARGE_BWD + LARGE_BWD + HEAD_BWD + ENC_BWD + CLIP + ADAM + LARGE_ASM + FINALIZE,
}
# the global-memory engine issues the same calls under either ELBO branch
SPARSE_EXPECTED["BallLargeStepEngine", True, "train"] = SPARSE_EXPECTED["BallLargeStepEngine", False, "train"]
SPARSE_EXPECTED["BallLargeStepEngine", True, "forward"] = SPARSE_EXPECTED["BallLargeStepEngine", False, "forward"]

PEARCE_GP = {"PearceStepEngine": ("svgp_pearce_gp_fwd", "svgp_pearce_gp_bwd"),
             "PearceLongStepEngine": ("svgp_pearce_long_fwd", "svgp_pearce_long_bwd")}
PEARCE_EXPECTED = {}
for _eng, (_f, _b) in PEARCE_GP.items():
    PEARCE_EXPECTED[_eng, "GPVAE_Pearce"] = (ENCODE + HEAD_FWD + [_f] + PACK + RECON + DEC_BWD + UNPACK + [_b] + HEAD_BWD + ENC_BWD
                                             + ADAM + PEARCE_ASM + FINALIZE)
    # the context set follows the full set, forward and reverse
    PEARCE_EXPECTED[_eng, "NP"] = (ENCODE + HEAD_FWD + [_f, _f] + PACK + RECON + SCALE_ROWS + DEC_BWD + UNPACK + [_b, _b] + HEAD_BWD
                                   + ENC_BWD + ADAM + PEARCE_ASM + FINALIZE)
    PEARCE_EXPECTED[_eng, "VAE"] = ENCODE + HEAD_FWD + [_f] + PACK + RECON + PEARCE_ASM + FINALIZE

PREDICT_EXPECTED = {
    ("BallPredictor", 3): ENCODE + HEAD_FWD + ["svgp_ball_predict"] + PACK + DECODE + ["svgp_sigmoid_xent"],
    ("BallPredictor", 65): ENCODE + HEAD_FWD + ["svgp_ball_predict_large"] + PACK + DECODE + ["svgp_sigmoid_xent"],
    ("PearcePredictor", 5): ENCODE + HEAD_FWD + ["svgp_pearce_predict"] + PACK + DECODE + ["svgp_sigmoid_xent"],
    ("PearcePredictor", 65): ENCODE + HEAD_FWD + ["svgp_pearce_predict_long"] + PACK + DECODE + ["svgp_sigmoid_xent"],
}


# ---- the cases (shared with nothing else; seeded, so that two builds of the host code can be run on the same numbers)
def videos(frames=T, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, frames, PX, PX, dtype=torch.float64, generator=g) < 0.3).to(torch.float64)


def epsilon(n=T, seed=1):
    return torch.randn(B, n, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def sparse_engine(name, titsias, clip_grad=False):
    from svgp_vae_amd import ball
    mk = lambda n: ball.SVGP(titsias, M, False, 1, T, 2.0, False, n, 1e-6, 1, T, 2.0)
    return getattr(ball, name)(mk("x"), mk("y"), batch=B, tmax=T, px=PX, py=PX, hidden=HIDDEN, clip_qs=True, clip_grad=clip_grad)


def pearce_engine(name, elbo):
    from svgp_vae_amd import ball
    return getattr(ball, name)(elbo, 2.0, 0.5, elbo == "GPVAE_Pearce", 2.0, batch=B, tmax=T, px=PX, py=PX, hidden=HIDDEN)


def pearce_step_kw(elbo):
    kw = dict(adam=True, backward=elbo != "VAE")
    if elbo == "NP":
        kw.update(ran_ind=np.stack([np.random.RandomState(3 + b).permutation(T) for b in range(B)]), con_tf=2)
    return kw


def predictor(name, size):
    """BallPredictor with m = size inducing points on T frames, PearcePredictor on size frames -> (predictor, frames)."""
    from svgp_vae_amd import ball, ball_predict
    p = dict(ball.truncated_normal_mlp_params(PX, PX, HIDDEN, seed=0), l_x=np.array([2.0]), l_y=np.array([1.5]))
    if name == "PearcePredictor":
        return ball_predict.PearcePredictor(p, tmax=size, hidden=HIDDEN, px=PX, py=PX), size
    p.update(ip_x=np.linspace(1.0, T, size), ip_y=np.linspace(0.5, T + 0.5, size))
    return ball_predict.BallPredictor(p, tmax=T, m=size, hidden=HIDDEN, px=PX, py=PX, jitter=1e-4, clip_qs=True), T


QUERY_TIMES = np.array([0.5, 2.25, 6.0])


@pytest.fixture
def recorded(monkeypatch):
    from svgp_vae_amd import _lib, ball, ball_predict
    names = []

    def recorder(name, *args):
        names.append(name)
        return _lib.call(name, *args)
    monkeypatch.setattr(ball, "call", recorder)
    monkeypatch.setattr(ball_predict, "call", recorder)
    return names


@pytest.mark.parametrize("name,titsias,mode", list(SPARSE_EXPECTED))
def test_sparse_step_issues_its_library_calls_in_the_recorded_order(recorded, name, titsias, mode):
    eng = sparse_engine(name, titsias, clip_grad=mode == "clip")
    del recorded[:]                                             # the constructor's layout call
    eng.step(videos(), epsilon(), adam=True, backward=mode != "forward")
    eng.stream.synchronize()
    assert recorded == SPARSE_EXPECTED[name, titsias, mode]
    assert bool(torch.isfinite(eng.out).all())


@pytest.mark.parametrize("name,elbo", list(PEARCE_EXPECTED))
def test_exact_gp_step_issues_its_library_calls_in_the_recorded_order(recorded, name, elbo):
    eng = pearce_engine(name, elbo)
    del recorded[:]
    eng.step(videos(), epsilon(), **pearce_step_kw(elbo))
    eng.stream.synchronize()
    assert recorded == PEARCE_EXPECTED[name, elbo]
    assert bool(torch.isfinite(eng.out[:3]).all())


@pytest.mark.parametrize("name,size", list(PREDICT_EXPECTED))
def test_predict_issues_its_library_calls_in_the_recorded_order(recorded, name, size):
    pred, frames = predictor(name, size)
    del recorded[:]
    out = pred.predict(videos(frames), QUERY_TIMES, eps=epsilon(Q))
    assert recorded == PREDICT_EXPECTED[name, size]
    assert tuple(out["frames"].shape) == (B, Q, PX, PX) and bool(torch.isfinite(out["frames"]).all())
