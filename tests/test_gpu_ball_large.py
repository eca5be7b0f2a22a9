"""Moving-ball SVGP-VAE with more than 64 inducing points or more than 64 videos per batch (ball.BallLargeStepEngine on
csrc/ball_large.hip + gp_large.hip) against the step oracle of tests/ball_large_cases.py, at the bars of tests/ball_cases.py:
outputs 1e-8, mean ELBO 1e-9, gradients 1e-7 of the tensor's max-abs.  tests/test_ball_large_cpu.py guards the table (the oracle's
own one-ulp response stays within 1/100 of these bars)."""
import numpy as np
import pytest
import torch

from oracle import ball_oracle as BO
from oracle import pearce_vae_oracle as PO
from tests import ball_cases as BC
from tests import ball_large_cases as LC
from tests import helpers as H

pytestmark = pytest.mark.gpu
DT = torch.float64


@pytest.mark.parametrize("case", list(LC.LARGE_CASES))
def test_large_step_matches_oracle(case):
    from svgp_vae_amd import ball
    cs = LC.LARGE_CASES[case]
    p, vid, eps, out, grads = LC.large_reference(case)
    eng = LC.large_engine(p, cs)
    assert type(eng) is ball.BallLargeStepEngine
    eng.step(vid.cuda(), eps.cuda(), adam=False)
    got = eng.outputs()
    assert len(got) == 19 and got[18] is eng
    bad, worst_out, worst_grad = [], 0.0, 0.0
    for i, n in enumerate(LC.OUT_NAMES):
        e = H.relerr(got[i], out[i])
        worst_out = max(worst_out, e)
        if not e < BC.OUT_TOL:
            bad.append(f"{n}: {e:.2e}")
    sc = eng.scalars()
    e_elbo = abs(sc["elbo"] - float(out[0].mean())) / abs(float(out[0].mean()))
    if not e_elbo <= BC.ELBO_TOL:
        bad.append(f"mean elbo {sc['elbo']} vs {float(out[0].mean())}")
    eng.stream.synchronize()
    for k in BO.PARAM_ORDER:
        e = H.relerr(eng.grads[k].reshape(-1), grads[k].reshape(-1))
        worst_grad = max(worst_grad, e)
        if not e < BC.GRAD_TOL:
            bad.append(f"grad {k}: {e:.2e}")
    print(f"{case}: outputs {worst_out:.2e}, mean elbo {e_elbo:.2e}, gradients {worst_grad:.2e}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("titsias", [False, True])
def test_three_adam_steps_match_oracle_trajectory(titsias):
    batch, T, m = 3, 130, 65
    cs = dict(batch=batch, tmax=T, m=m, titsias=titsias)
    p, _, _ = BC._problem(batch, T, BC.ENV_PX, BC.ENV_HIDDEN, m, seed=75)
    g = torch.Generator().manual_seed(11)
    vids = [PO.make_video_batch(tmax=T, px=BC.ENV_PX, py=BC.ENV_PX, lt=2.0, batch=batch, r=2, generator=g, dtype=DT)
            for _ in range(3)]
    epss = [torch.randn(batch, T, 2, dtype=DT, generator=g) for _ in range(3)]
    want, elbos = BO.train_trajectory(p, vids, epss, beta=1.0, titsias=titsias, jitter=BC.SPARSE_JITTER, clipping_qs=True,
                                      lr=1e-3, clip_grad=True, train_ip=True, train_gp=False)
    eng = LC.large_engine(p, cs, beta=1.0, fixed_gp=True, clip_grad=True, lr=1e-3)
    got_elbo = []
    for v, e in zip(vids, epss):
        eng.step(v.cuda(), e.cuda(), adam=True)
        got_elbo.append(eng.scalars()["elbo"])
    print("elbo trajectory", got_elbo, elbos)
    assert np.allclose(got_elbo, elbos, rtol=BC.TRAJ_ELBO_RTOL)
    assert eng.scalars()["adam_t"] == 3.0
    for k in BO.PARAM_ORDER:
        assert H.relerr(eng.params[k].reshape(-1), want[k].reshape(-1)) < BC.TRAJ_PARAM_TOL, k
    assert float(eng.params["l_x"][0]) == float(p["l_x"]) and float(eng.params["l_y"][0]) == float(p["l_y"])


def test_fixed_inducing_points_and_gp_parameters_have_zero_gradients():
    cs = LC.LARGE_CASES["m65"]
    p, vid, eps, _, grads = LC.large_reference("m65")
    eng = LC.large_engine(p, cs, fixed_ip=True, fixed_gp=True)
    eng.step(vid.cuda(), eps.cuda(), adam=False)
    eng.stream.synchronize()
    for k in ("ip_x", "ip_y", "l_x", "l_y"):
        assert float(eng.grads[k].abs().max()) == 0.0, k
    assert H.relerr(eng.grads["encW1"].reshape(-1), grads["encW1"].reshape(-1)) < BC.GRAD_TOL


def test_philox_samples_equal_those_of_the_lds_engine_and_steps_repeat_bitwise():
    """A shape both engines accept (m = 24, 5 videos): the on-device samples are functions of the counter, the frame and the video
    alone, so both engines draw the same ones; the large engine has no float atomics, so a repeated step is bitwise identical."""
    from svgp_vae_amd import ball
    batch, T, m = 5, 40, 24
    cs = dict(batch=batch, tmax=T, m=m, titsias=False)
    p, vid, _ = BC._problem(batch, T, BC.ENV_PX, BC.ENV_HIDDEN, m, seed=77)
    small = BC._engine(p, batch, T, BC.ENV_PX, BC.ENV_HIDDEN, m, titsias=False, jitter=BC.SPARSE_JITTER, clip_qs=True,
                       beta=BC.SPARSE_BETA)
    mk = lambda n: ball.SVGP(False, m, False, 1, T, 2.0, False, n, BC.SPARSE_JITTER, 1, T, 2.0)
    flat = {k: (v.reshape(-1) if k.startswith(("encB", "decB", "l_")) else v) for k, v in p.items()}
    large = [ball.BallLargeStepEngine(mk("x"), mk("y"), batch=batch, tmax=T, px=BC.ENV_PX, py=BC.ENV_PX, hidden=BC.ENV_HIDDEN,
                                      clip_qs=True, beta=BC.SPARSE_BETA, params=flat) for _ in range(2)]
    v = vid.cuda()
    for e in [small] + large:
        e.step(v, None, adam=False)
        e.stream.synchronize()
    for c in range(2):
        es = small._v(c, "eps", (T, batch))
        assert float(es.abs().max()) > 0.5
        assert torch.equal(large[0]._v(c, "eps", (T, batch)), es)
    assert float((small._v(0, "eps", (T, batch)) - small._v(1, "eps", (T, batch))).abs().max()) > 0.1
    # same samples -> same step up to rounding between the two stage implementations
    assert abs(large[0].scalars()["elbo"] - small.scalars()["elbo"]) <= 1e-9 * abs(small.scalars()["elbo"])
    for k in BO.PARAM_ORDER:
        assert H.relerr(large[0].grads[k].reshape(-1), small.grads[k].reshape(-1)) < BC.GRAD_TOL, k
    # two engines, same inputs, same counter: bit for bit
    assert torch.equal(large[0].out, large[1].out) and torch.equal(large[0].grad, large[1].grad)
    assert torch.equal(large[0]._v(1, "z", (T, batch)), large[1]._v(1, "z", (T, batch)))
    # the counter moves on: the next step draws other samples
    e0 = large[0]._v(0, "eps", (T, batch)).clone()
    large[0].step(v, None, adam=False)
    large[0].stream.synchronize()
    assert float((large[0]._v(0, "eps", (T, batch)) - e0).abs().max()) > 0.1


def test_graph_builder_picks_the_large_engine():
    from svgp_vae_amd import ball
    cs = LC.LARGE_CASES["m65"]
    p, vid, eps, out, _ = LC.large_reference("m65")
    mk = lambda n: ball.SVGP(False, cs["m"], False, 1, cs["tmax"], 2.0, False, n, BC.SPARSE_JITTER, 1, cs["tmax"], 2.0)
    flat = {k: (v.reshape(-1) if k.startswith(("encB", "decB", "l_")) else v) for k, v in p.items()}
    got = ball.build_SVGPVAE_elbo_graph(vid.cuda(), BC.SPARSE_BETA, mk("x"), mk("y"), clipping_qs=True, epsilon=eps.cuda(),
                                        params=flat)
    assert type(got[18]) is ball.BallLargeStepEngine
    assert H.relerr(got[0], out[0]) < BC.OUT_TOL


@pytest.mark.parametrize("elbo", ["SVGPVAE_Hensman", "SVGPVAE_Titsias"])
def test_ball_cli_end_to_end_with_80_inducing_points(tmp_path, elbo):
    from svgp_vae_amd import BALL_experiment as BE
    from svgp_vae_amd import ball
    argv = ["--elbo", elbo, "--m", "80", "--tmax", "160", "--steps", "4", "--eval_every", "2", "--hidden", "32", "--clip_qs",
            "--GP_joint", "--ip_joint", "--ip_max", "160", "--jitter", "1e-6", "--base_dir", str(tmp_path), "--seed", "3"]
    assert type(BE.build_engine(BE.build_parser().parse_args(argv))) is ball.BallLargeStepEngine
    log = BE.main(argv)
    assert [r["Step"] for r in log] == [2, 4]
    for r in log:
        assert np.isfinite(r["elbo"]) and np.isfinite(r["MSE"]) and r["min q_var"] > 0
        assert np.isfinite(r["SVGP elbo"]) and len(r["inducing_points_x"]) == 80
