"""The global-memory exact per-video GP (PearceLongStepEngine, pearce_long.hip; 1 <= tmax <= 2048) against the float64 oracle
(oracle/ball_oracle.py) at the shapes where its kernels or the inverse behind them change form.  Case table, problems and the
engine builder: tests/ball_long_cases.py; tolerances: tests/ball_cases.py (no new ones); that the oracle itself is well
conditioned at every case: tests/test_ball_long_cpu.py."""
import numpy as np
import pytest
import torch

from oracle import ball_oracle as BO
from oracle import pearce_vae_oracle as PO
from tests import ball_cases as BC
from tests import ball_long_cases as LC
from tests import helpers as H
from tests.ball_cases import DT, _pearce_engine, _problem

pytestmark = pytest.mark.gpu

PEARCE_NAMES = ("elbo", "recon", "prior_kl", "full_p_mu", "full_p_var", "qnet_mu", "qnet_var", "pred_vid")


def _step(cs, ref, builder=LC.long_engine):
    p, vid, eps, ran_ind, out, grads = ref
    eng = builder(p, cs["type_elbo"], cs["lt"], cs["joint"], cs["batch"], cs["tmax"], BC.ENV_PX, BC.ENV_HIDDEN, BC.PEARCE_BETA)
    eng.step(vid.cuda(), eps.cuda(), adam=False, ran_ind=None if ran_ind is None else ran_ind.numpy(), con_tf=cs["con_tf"])
    return eng


def _compare(tag, cs, eng, out, grads):
    """The 8 outputs at OUT_TOL, the mean ELBO at ELBO_TOL, every gradient at GRAD_TOL (l_* exactly 0 without --GP_joint), and
    for the NP ELBO the context likelihoods' length-scale gradient; every figure is printed before anything is asserted."""
    got = eng.outputs()
    bad = []
    for i, n in enumerate(PEARCE_NAMES):
        e = H.relerr(got[i], out[i])
        print(f"{tag} {n}: {e:.2e}")
        if not e < BC.OUT_TOL:
            bad.append(f"{n}: {e:.2e}")
    mean_elbo = float(out[0].mean())
    e = abs(eng.scalars()["elbo"] - mean_elbo) / abs(mean_elbo)
    print(f"{tag} mean elbo: {e:.2e}")
    if not e <= BC.ELBO_TOL:
        bad.append(f"mean elbo: {e:.2e}")
    eng.stream.synchronize()
    for k in BO.PEARCE_PARAM_ORDER:
        if k.startswith("l_") and not cs["joint"]:
            if float(eng.grads[k].abs().max()) != 0.0:                 # constants when not --GP_joint
                bad.append(f"grad {k} is not exactly 0")
            continue
        e = H.relerr(eng.grads[k].reshape(-1), grads[k].reshape(-1))
        print(f"{tag} grad {k}: {e:.2e}")
        if not e < BC.GRAD_TOL:
            bad.append(f"grad {k}: {e:.2e}")
    if cs["type_elbo"] == "NP":
        want = torch.stack([grads["ctx_l_x"], grads["ctx_l_y"]])
        e = H.relerr(eng.c_dl, want)
        print(f"{tag} c_dl: {e:.2e} (want {want.tolist()})")
        if not e < BC.GRAD_TOL:
            bad.append(f"c_dl: {e:.2e}")
    return bad


@pytest.mark.parametrize("case", list(LC.LONG_CASES))
def test_long_step_matches_oracle(case):
    from svgp_vae_amd import ball
    cs = LC.LONG_CASES[case]
    ref = LC.long_reference(case)
    eng = _step(cs, ref)
    assert type(eng) is ball.PearceLongStepEngine and eng.want_dls == int(cs["joint"])
    bad = _compare(case, cs, eng, ref[4], ref[5])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", LC.CMP_CASES)
def test_both_engines_meet_the_same_bars_where_both_run(case):
    """The new entry points at sizes the LDS kernels run too (n = 33, 64): both engines against the oracle at the same bars;
    their direct difference is information only."""
    cs = BC.PEARCE_ENV_CASES[case]
    ref = BC.pearce_reference(case)
    new, old = _step(cs, ref), _step(cs, ref, _pearce_engine)
    bad = _compare(f"{case} long", cs, new, ref[4], ref[5]) + _compare(f"{case} lds", cs, old, ref[4], ref[5])
    for i, n in enumerate(PEARCE_NAMES):
        print(f"{case} long vs lds {n}: {H.relerr(new.outputs()[i], old.outputs()[i]):.2e}")
    for k in BO.PEARCE_PARAM_ORDER:
        print(f"{case} long vs lds grad {k}: {H.relerr(new.grads[k].reshape(-1), old.grads[k].reshape(-1)):.2e}")
    assert not bad, "\n".join(bad)


def test_long_step_is_bitwise_reproducible():
    cs, ref = LC.LONG_CASES["T130_np"], LC.long_reference("T130_np")
    a, b = _step(cs, ref), _step(cs, ref)
    for x, y in zip(a.outputs()[:8], b.outputs()[:8]):
        assert torch.equal(x, y)
    assert torch.equal(a.grad, b.grad) and torch.equal(a.c_dl, b.c_dl)
    assert float(a.grad.abs().max()) > 0


def test_three_adam_steps_at_96_frames_track_the_oracle():
    batch, T, px, hidden = 6, 96, BC.ENV_PX, BC.ENV_HIDDEN
    p, vid, eps = _problem(batch, T, px, hidden, 4, seed=60 + T)
    p = {k: v for k, v in p.items() if not k.startswith("ip_")}
    p["l_x"], p["l_y"] = torch.tensor(2.0, dtype=DT), torch.tensor(2.0, dtype=DT)
    eng = LC.long_engine(p, "GPVAE_Pearce", 2.0, True, batch, T, px, hidden, 1.0, lr=1e-3)
    from oracle import svgpvae_oracle as O
    q = {k: v.clone() for k, v in p.items()}
    ms, vs = {k: torch.zeros_like(v) for k, v in q.items()}, {k: torch.zeros_like(v) for k, v in q.items()}
    bad = []
    for t in range(1, 4):
        out, loss, g = BO.pearce_loss_and_grads(q, vid, eps, beta=1.0, type_elbo="GPVAE_Pearce", lt=2.0)
        O.adam_tf1_step(q, g, ms, vs, t, 1e-3)
        eng.step(vid.cuda(), eps.cuda(), adam=True)
        want = float(out[0].mean())
        e = abs(eng.scalars()["elbo"] - want) / abs(want)
        print(f"step {t} elbo {want}: {e:.2e}")
        if not e < BC.TRAJ_ELBO_RTOL:
            bad.append(f"step {t} elbo: {e:.2e}")
    assert eng.scalars()["adam_t"] == 3.0
    for k in BO.PEARCE_PARAM_ORDER:
        e = H.relerr(eng.params[k].reshape(-1), q[k].reshape(-1))
        print(f"param {k}: {e:.2e}")
        if not e < BC.TRAJ_PARAM_TOL:
            bad.append(f"param {k}: {e:.2e}")
    assert not bad, "\n".join(bad)


def test_on_device_philox_samples_are_standard_normal():
    cs = LC.LONG_CASES["T65"]
    p, vid, _, _, _, _ = LC.long_reference("T65")
    eng = LC.long_engine(p, cs["type_elbo"], cs["lt"], cs["joint"], cs["batch"], cs["tmax"], BC.ENV_PX, BC.ENV_HIDDEN,
                         BC.PEARCE_BETA)
    eng.step(vid.cuda(), None, adam=False)
    for o in eng.outputs()[:8]:
        assert torch.isfinite(o).all()
    eng.stream.synchronize()
    assert torch.isfinite(eng.grad).all()
    e = eng.buf["eps"].cpu().reshape(-1)
    n = e.numel()                                                     # 2 * 65 * 5 draws: se(mean) = 1/sqrt(n), se(var) = sqrt(2/n)
    print(f"eps: n {n} mean {float(e.mean()):.4f} var {float(e.var()):.4f}")
    assert abs(float(e.mean())) < 5 / np.sqrt(n) and abs(float(e.var()) - 1) < 5 * np.sqrt(2 / n)
    assert eng.scalars()["rng_ctr"] == 1.0


@pytest.mark.parametrize("elbo,extra", [("VAE", []), ("GPVAE_Pearce", ["--GP_joint"]), ("NP", [])])
def test_ball_cli_end_to_end_at_80_frames(tmp_path, elbo, extra):
    from svgp_vae_amd import BALL_experiment as BE
    from svgp_vae_amd import ball
    argv = ["--elbo", elbo, "--steps", "8", "--eval_every", "4", "--hidden", "32", "--tmax", "80", "--base_dir", str(tmp_path),
            "--save", "--save_model", "--seed", "3"] + extra
    log = BE.main(argv)
    assert [r["Step"] for r in log] == [4, 8]
    for r in log:
        assert np.isfinite(r["elbo"]) and np.isfinite(r["MSE"]) and r["min q_var"] > 0
    runs = [d for d in tmp_path.iterdir() if d.is_dir()]
    assert len(runs) == 1 and (runs[0] / "res" / "ELBO_log.jsonl").exists() and (runs[0] / "model.pt").exists()
    assert (tmp_path / "Test_Batches_2_80.pkl").exists()
    args = BE.build_parser().parse_args(argv)
    assert type(BE.build_engine(args, batch=2, px=8, py=8)) is ball.PearceLongStepEngine
    args.tmax = 64
    assert type(BE.build_engine(args, batch=2, px=8, py=8)) is ball.PearceStepEngine


def test_build_pearce_elbo_graphs_takes_a_70_frame_batch():
    from svgp_vae_amd import ball
    from svgp_vae_amd.GPVAE_Pearce_model import build_pearce_elbo_graphs
    g = torch.Generator().manual_seed(3)
    vid = PO.make_video_batch(tmax=70, px=8, py=8, lt=2.0, batch=4, r=2, generator=g, dtype=DT)
    out = build_pearce_elbo_graphs(vid.cuda(), 1.0, "GPVAE_Pearce", lt=2)
    assert len(out) == 11 and type(out[10]) is ball.PearceLongStepEngine
    shapes = [tuple(o.shape) for o in out[:10]]
    assert shapes == [(4,), (4,), (4,), (4, 70, 2), (4, 70, 2), (4, 70, 2), (4, 70, 2), (4, 70, 8, 8), (), ()]
    small = build_pearce_elbo_graphs(vid[:, :60].contiguous().cuda(), 1.0, "GPVAE_Pearce", lt=2)
    assert type(small[10]) is ball.PearceStepEngine
    assert [len(tuple(o.shape)) for o in small[:10]] == [len(s) for s in shapes]
    for o in out[:8]:
        assert torch.isfinite(o).all()
    assert float(out[4].min()) > 0


def test_limits_of_both_exact_gp_engines():
    from svgp_vae_amd import _lib
    with pytest.raises(_lib.SvgpError, match="tmax=2049"):
        LC.long_engine({}, "GPVAE_Pearce", 2.0, True, 1, 2049, 8, 8, 1.0)
    with pytest.raises(_lib.SvgpError, match="tmax <= 64"):
        _pearce_engine({}, "GPVAE_Pearce", 2.0, True, 4, 65, 8, 8, 1.0)
