"""Rotated-MNIST experiment driver with the reference's CLI (MNIST_experiment.py:1115-1174 flags and
defaults) for `--elbo SVGPVAE_Hensman | SVGPVAE_Titsias | SVIGP_Hensman | GPVAE_Casale`, running every step on the HIP library.

    python -m svgp_vae_amd.MNIST_experiment --elbo SVGPVAE_Hensman --ip_joint --GP_joint --ov_joint \
        --clip_qs --GECO --PCA --mnist_data_path "MNIST data/"

Mirrors run_experiment_rotated_mnist_SVGPVAE (MNIST_experiment.py:30-541): model construction with the
inverted `fixed_*` flags (:96-98), the un-shuffled epoch loop with ragged last batch (:319-355), GECO state
carry / first-step alpha=0 (kept on device), and every 10 epochs: eval-set reconstruction MSE, conditional
generation MSE on the test set (:457-486) and `pics/test_metrics.txt` lines `epoch,recon MSE,cgen MSE`
(:509-510).  Plotting / pandas logging of the reference are not reproduced.
`--bias_analysis` (:172-179, 325-363; supplement C.4) prints `Bias for epoch {epoch}: {bias}` after every epoch: the distance
between the epoch's average of the per-step inducing mean vectors and the ones of the whole train set; `--save_latents`
(:181-187, 531-541; needs `--save`) pickles the latent samples of the whole train set after the last epoch to
`latents_train_full.p`.  Both are wired for the two SVGPVAE objectives only.
`--restore RUN/model_<k>.pt [--first_epoch K]` (the two SVGPVAE objectives) resumes a run from a checkpoint that `--save
--save_model_weights` wrote: the epochs K .. nr_epochs - 1 (default K = k + 1) run with their own indices, so with
`--epsilon_seed` the resumed run is the tail of the uninterrupted one (svgp_vae_amd/checkpoint.py).
Accepted without effect: `--test_set_metrics` (it selects the split of the reference's pandas rows, which this build does not
write), `--show_pics` (no plots) and `--ram` (the reference's TensorFlow memory fraction).
`--elbo SVIGP_Hensman` mirrors run_experiment_rotated_mnist_SVIGP_Hensman (:544-760): deep SVIGP with free variational
parameters, same loaders / inducing-point init, per-epoch train MSE and the conditional-generation MSE on the test set.
`--elbo GPVAE_Casale` mirrors run_experiment_rotated_mnist_Casale (:786-1110): Casale's GP-VAE with the three optimisation
regimes of `--opt_regime` (joint / GP / VAE), one Adam state, conditional generation on the test set every 5 epochs.
`--elbo VAE | CVAE` run under `python -m svgp_vae_amd.VAE_experiment` (same flags); this module keeps refusing them and names that
command.  `--elbo GPVAE_Casale_batch` is outside this build.
"""
import argparse
import json
import os
import pickle
import time

import numpy as np
import torch

from .SVGPVAE_model import _runtime, bacthing_predict_SVGPVAE_rotated_mnist, batching_encode_SVGPVAE, mnistSVGP
from .utils import (batches, generate_init_inducing_points, import_rotated_mnist, latent_samples_SVGPVAE,
                    parse_opt_regime)
from .VAE_utils import mnistVAE


def build_parser():
    p = argparse.ArgumentParser(description="Rotated MNIST experiment (MI355X SVGPVAE_Hensman path).")
    p.add_argument('--expid', type=str, default="debug_MNIST")
    p.add_argument('--base_dir', type=str, default=os.getcwd())
    p.add_argument('--elbo', type=str, default="VAE",
                   choices=['VAE', 'CVAE', 'SVGPVAE_Hensman', 'SVGPVAE_Titsias', 'GPVAE_Casale', 'GPVAE_Casale_batch',
                            'SVIGP_Hensman'])
    p.add_argument('--mnist_data_path', type=str, default='MNIST data/')
    p.add_argument('--batch_size', type=int, default=256)
    p.add_argument('--nr_epochs', type=int, default=1000)
    p.add_argument('--beta', type=float, default=0.001)
    p.add_argument('--nr_inducing_points', type=float, default=2)
    p.add_argument('--save', action="store_true")
    p.add_argument('--GP_joint', action="store_true")
    p.add_argument('--ip_joint', action="store_true")
    p.add_argument('--ov_joint', action="store_true")
    p.add_argument('--lr', type=float, default=0.001)
    p.add_argument('--save_model_weights', action="store_true")
    p.add_argument('--dataset', type=str, choices=['3', '36', '13679'], default='3')
    p.add_argument('--show_pics', action="store_true")
    p.add_argument('--opt_regime', type=str, default=['joint-1000'], nargs="+")
    p.add_argument('--L', type=int, default=16)
    p.add_argument('--clip_qs', action="store_true")
    p.add_argument('--ram', type=float, default=1.0)
    p.add_argument('--test_set_metrics', action='store_true')
    p.add_argument('--GECO', action='store_true')
    p.add_argument('--alpha', type=float, default=0.99)
    p.add_argument('--kappa_squared', type=float, default=0.020)
    p.add_argument('--object_kernel_normalize', action='store_true')
    p.add_argument('--save_latents', action='store_true')
    p.add_argument('--jitter', type=float, default=0.000001)
    p.add_argument('--PCA', action="store_true")
    p.add_argument('--bias_analysis', action='store_true')
    p.add_argument('--M', type=int, default=8)
    # additions of this build
    p.add_argument('--train_file', type=str, default=None,
                   help="pickle used as the train set instead of train_data<dataset>.p (absent from the reference checkout)")
    p.add_argument('--eval_every', type=int, default=None,
                   help="evaluation period in epochs; default: the reference's 10, and 5 for GPVAE_Casale")
    p.add_argument('--seed', type=int, default=0, help="seed of the Keras-style weight init and numpy")
    p.add_argument('--epsilon_seed', type=int, default=None,
                   help="reproducible N(0,1) draws of SVGPVAE_model.py:901: batch i of epoch e uses "
                        "numpy.random.RandomState(1000 e + i + seed).randn(rows, L) instead of the on-device generator")
    p.add_argument('--split_grad_exchange', action='store_true',
                   help="data parallel: the gradient all-reduce in two parts, the first (decoder + GP parameters) beside the encoder's "
                        "reverse pass (cfg.split_grad_exchange; a fallback for slow small-message all-reduces)")
    p.add_argument('--restore', type=str, default=None,
                   help="SVGPVAE_Hensman / SVGPVAE_Titsias: a model_<epoch>.pt written by --save --save_model_weights; parameters, Adam "
                        "moments and the device state vector are loaded into the engine before the first step")
    p.add_argument('--first_epoch', type=int, default=None,
                   help="index of the first epoch to run; default: k + 1 when --restore names a model_<k>.pt, else 0")
    p.add_argument('--log_json', type=str, default=None,
                   help="rank 0 writes the per-step log (elbo, recon_loss, C_ma, lagrange_mult), the evaluation series and the "
                        "final flat parameter vector to this file")
    return p


def _eval_every(args, default):
    """--eval_every, or the calling driver's reference period when the flag was not given."""
    given = getattr(args, "eval_every", None)
    return default if given is None else given


def run_experiment_rotated_mnist_SVGPVAE(args, args_dict=None, ctx=None):
    """MNIST_experiment.py:30-541 for elbo == SVGPVAE_Hensman.  Returns a dict of the logged series.

    Data parallel (svgp_vae_amd/dp.py): launched as `python -m torch.distributed.run --nproc-per-node G -m
    svgp_vae_amd.MNIST_experiment ...`, every rank takes a contiguous row range of every batch (incl. the ragged last one),
    c = N_train / b_global, the engines all-reduce statistics and gradients; rank 0 alone evaluates, prints and writes files.

    --bias_analysis: the mean vectors of every optimiser step (ws[mu_hat] of its forward pass, i.e. at the parameters before
    the update; the ragged last batch included) are summed on the device by one extra launch behind the step, outside the
    captured graph and without a read-back; at the end of every epoch rank 0 computes the mean vectors of the whole train
    set at the parameters after the last update (c = N_train / N) and the bias of utils.py:922-948, prints it and appends
    (epoch, bias) to log["bias"].  DEVIATION: the reference fills its list only in the GECO branch (:329-342) and fails on
    the empty list without --GECO; this build collects under both objectives.
    --save_latents: after the last epoch rank 0 writes the latent samples (N, L) of the whole train set to
    chkpnt_dir + "latents_train_full.p" and returns the device tensor as log["_latents"]; with --epsilon_seed s the draw is
    numpy.random.RandomState(1000 nr_epochs + s).randn(N, L), otherwise it is made on the device."""
    from .dp import DistContext, attach_library_comm, run_sharded_epochs
    if args.elbo not in ("SVGPVAE_Hensman", "SVGPVAE_Titsias"):
        raise NotImplementedError(f"--elbo {args.elbo}: only SVGPVAE_Hensman / SVGPVAE_Titsias are built "
                                  f"(see DESIGN.md section 9)")
    if args.save_latents and not args.save:
        raise ValueError("--save_latents writes latents_train_full.p into the checkpoint directory, which exists only with --save")
    ctx = (ctx or DistContext()).init()
    root = ctx.rank == 0
    np.random.seed(args.seed)                    # every rank: the same initial parameters (they are never broadcast)
    n = len(args.dataset)
    ending = args.dataset + ".p"
    train, ev, te, train_batches = import_rotated_mnist(args.mnist_data_path, ending, args.batch_size,
                                                        train_file=args.train_file)
    N_train = len(train["images"]) if args.train_file else n * 4050
    N_eval, N_test = len(ev["images"]), len(te["images"])

    chkpnt_dir = None
    if args.save and root:
        stamp = time.strftime("%d_%m_%Y__at__%H_%M_%S")
        chkpnt_dir = os.path.join(args.base_dir, args.expid, f"{args.elbo}_{args.beta}__on__{stamp}") + "/"
        os.makedirs(chkpnt_dir + "pics/", exist_ok=True)
        json.dump({k: v for k, v in (args_dict or vars(args)).items() if not callable(v)}, open(chkpnt_dir + "args.json", "wt"))

    # ---- model (MNIST_experiment.py:82-115)
    VAE = mnistVAE(L=args.L, seed=args.seed, device=ctx.device)
    inducing_points_init = generate_init_inducing_points(None, n=args.nr_inducing_points, remove_test_angle=None,
                                                         PCA=args.PCA, M=args.M, aux_data=train["aux_data"])
    ip_joint, GP_joint = not args.ip_joint, not args.GP_joint          # sic: passed as fixed_* (:96-98)
    if args.ov_joint:
        if args.PCA:
            object_vectors_init = pickle.load(open(args.mnist_data_path + f'pca_ov_init{args.dataset}.p', 'rb'))
        else:
            object_vectors_init = np.random.normal(0, 1.5, n * 400 * args.M).reshape(n * 400, args.M)
    else:
        object_vectors_init = None
    SVGP_ = mnistSVGP(titsias='Titsias' in args.elbo, fixed_inducing_points=ip_joint, initial_inducing_points=inducing_points_init,
                      fixed_gp_params=GP_joint, object_vectors_init=object_vectors_init, name='main',
                      jitter=args.jitter, N_train=N_train, L=args.L, K_obj_normalize=args.object_kernel_normalize,
                      device=ctx.device)
    kappa = float(np.sqrt(args.kappa_squared))
    # the cgen path runs the statistics over all train rows; the capacity is the SAME on every rank (the layout of the exchange
    # blocks is a function of it)
    b_cap = max(args.batch_size, N_train)
    rt = _runtime(VAE, SVGP_, args.clip_qs, args.GECO, kappa, b_cap, alpha_flag=args.alpha, lr=args.lr,
                  beta=args.beta, rank=ctx.rank, world_size=ctx.world,
                  split_grad_exchange=getattr(args, "split_grad_exchange", False))
    eng = rt.eng
    dev = eng.device
    comm_fallback = attach_library_comm(eng, ctx)
    first_epoch = 0
    if getattr(args, "restore", None):           # every rank loads the same file: the parameters stay replicated
        from . import checkpoint
        checkpoint.restore(eng, args.restore)
        given = getattr(args, "first_epoch", None)
        first_epoch = checkpoint.first_epoch_of(args.restore) if given is None else given
    elif getattr(args, "first_epoch", None):
        first_epoch = args.first_epoch
    if root:
        print(f"Number of train params: {eng.pl.n_total}")
        if getattr(args, "restore", None):
            print(f"Restored {args.restore}; first epoch {first_epoch}", flush=True)
        if ctx.multi:
            print(f"Data parallel over {ctx.world} ranks: " + ("RCCL communicator of the library, collectives on the compute stream"
                  if eng.comm is not None else f"torch.distributed all-reduces between the phases ({comm_fallback})"), flush=True)

    # ---- data resident in HBM; batches are copied device-to-device into fixed staging buffers so that
    #      one captured hipGraph per batch size serves every batch
    t64 = lambda a: torch.tensor(a, dtype=torch.float64, device=dev).contiguous()
    d_train_img, d_train_aux = t64(train["images"]), t64(train["aux_data"])
    d_eval_img, d_eval_aux = t64(ev["images"]), t64(ev["aux_data"])
    d_test_img, d_test_aux = t64(te["images"]), t64(te["aux_data"])
    stage_img = torch.zeros(args.batch_size, 28, 28, 1, dtype=torch.float64, device=dev)
    stage_aux = torch.zeros(args.batch_size, 2 + args.M, dtype=torch.float64, device=dev)
    # the N(0,1) draw of SVGPVAE_model.py:901 is made on device; `args.epsilon_fn(epoch, batch index, rows, L) -> array`
    # (not a CLI flag: set by callers that need a reproducible trajectory, tests/test_gpu_api.py) makes it an input
    eps_fn = getattr(args, "epsilon_fn", None)
    if eps_fn is None and getattr(args, "epsilon_seed", None) is not None:
        eps_fn = lambda epoch, i, rows, L_: np.random.RandomState(1000 * epoch + i + args.epsilon_seed).randn(rows, L_)
    stage_eps = torch.zeros(args.batch_size, args.L, dtype=torch.float64, device=dev) if eps_fn else None
    eng.stream.wait_stream(torch.cuda.current_stream(dev))   # uploads / zero-fills above ran on torch's stream
    graphs = {}

    def local_step(llo, lhi, lo, hi, epoch, i):
        b, b_global = lhi - llo, hi - lo
        with torch.cuda.stream(eng.stream):
            stage_img[:b].copy_(d_train_img[llo:lhi])
            stage_aux[:b].copy_(d_train_aux[llo:lhi])
            if eps_fn:                 # the draw of the GLOBAL batch; this rank's rows of it
                e = np.asarray(eps_fn(epoch, i, b_global, args.L))[llo - lo:lhi - lo]
                stage_eps[:b].copy_(torch.as_tensor(e, dtype=torch.float64), non_blocking=False)
        if ctx.multi:                  # collectives are not captured: the eager step (as fast as the replay)
            eng.set_batch_size(b, b_global)
            eng.bind(stage_img[:b], stage_aux[:b], stage_eps[:b] if eps_fn else None)
            eng.run(adam=True)
        else:
            if b not in graphs:
                eng.set_batch_size(b)
                eng.bind(stage_img[:b], stage_aux[:b], stage_eps[:b] if eps_fn else None)   # None: drawn on device
                eng.capture(("train", b), adam=True)
                graphs[b] = True
            eng.replay(("train", b))
        if args.bias_analysis:         # :341-342: this step's mean vectors into the epoch's sum; a launch of its own behind the graph
            eng.mean_vectors_accumulate()
        # the reference fetches elbo / recon_loss / C_ma / lagrange_mult every step (:334-340); one 128-byte read-back
        eng.synchronize()
        return eng.scalars()

    def on_epoch_start(epoch):
        if args.bias_analysis:         # :325-326
            eng.mean_vectors_begin()

    def bias_of_epoch(epoch, log):
        """:357-363: the whole-train-set mean vectors at the parameters the epoch ends with, against the average of the steps'."""
        if root:
            bias, _ = eng.mean_vectors_bias(eng.mean_vectors_full(d_train_img, d_train_aux))
            log.setdefault("bias", []).append((epoch, bias))
            print("Bias for epoch {}: {}".format(epoch, bias), flush=True)
        ctx.barrier()

    def on_epoch_end(epoch, log):
        if args.bias_analysis:
            bias_of_epoch(epoch, log)
        if not ((epoch + 1) % _eval_every(args, 10) == 0 or epoch + 1 == nr_epochs):
            return
        if root:       # parameters are replicated: rank 0 evaluates alone (collective-free stage calls), the others wait
            # eval-set reconstruction through the posterior (forward only, no optimiser step)
            ev_losses = []
            for lo, hi in batches(N_eval, args.batch_size):
                eng.set_batch_size(hi - lo)
                eng.bind(d_eval_img[lo:hi].contiguous(), d_eval_aux[lo:hi].contiguous(), None)
                with torch.cuda.stream(eng.stream):
                    eng.phase(0); eng.phase(1)
                eng.synchronize()
                rec = eng.ws_view("recon", (hi - lo, 28, 28, 1))
                ev_losses.append(float(torch.sum((d_eval_img[lo:hi] - rec) ** 2)) / 784.0)
            eval_mse = float(np.sum(ev_losses) / N_eval)
            # conditional generation on the test set (:457-486)
            means, vars_ = [], []
            for lo, hi in train_batches:
                mu, var, _ = batching_encode_SVGPVAE((d_train_img[lo:hi], d_train_aux[lo:hi]), VAE,
                                                     clipping_qs=args.clip_qs)
                means.append(mu); vars_.append(var)
            means, vars_ = torch.cat(means), torch.cat(vars_)
            cg = []
            for lo, hi in batches(N_test, args.batch_size):
                _, loss_ = bacthing_predict_SVGPVAE_rotated_mnist((d_test_img[lo:hi], d_test_aux[lo:hi]), VAE, SVGP_,
                                                                  means, vars_, d_train_aux)
                cg.append(float(loss_))
            cgen_mse = float(np.sum(cg) / N_test)
            log.setdefault("eval_mse", []).append((epoch, eval_mse)); log.setdefault("cgen_mse", []).append((epoch, cgen_mse))
            print(f"  eval recon MSE/px {eval_mse:.6f}   cgen test MSE/px {cgen_mse:.6f}   "
                  f"l_GP {float(SVGP_.l_GP):.4f} amplitude {float(SVGP_.amplitude):.4f}", flush=True)
            if chkpnt_dir:
                with open(chkpnt_dir + "pics/test_metrics.txt", "a") as f:
                    f.write(f"{epoch},{eval_mse},{cgen_mse}\n")
                if args.save_model_weights:
                    torch.save({"theta": eng.theta.cpu(), "adam_m": eng.adam_m.cpu(), "adam_v": eng.adam_v.cpu(),
                                "state": eng.state.cpu()}, chkpnt_dir + f"model_{epoch}.pt")
        ctx.barrier()

    nr_epochs, training_regime = parse_opt_regime(args.opt_regime)
    start = time.time()

    log = run_sharded_epochs(ctx, train_batches, nr_epochs, local_step, N_train=N_train, on_epoch_end=on_epoch_end,
                             on_epoch_start=on_epoch_start, first_epoch=first_epoch)
    log.setdefault("eval_mse", []); log.setdefault("cgen_mse", [])
    if args.bias_analysis:
        log.setdefault("bias", [])
    latents = None
    if args.save_latents:              # :181-187, 531-541
        if root:
            N = d_train_img.shape[0]
            eps = None
            if getattr(args, "epsilon_seed", None) is not None:
                eps = torch.as_tensor(np.random.RandomState(1000 * nr_epochs + args.epsilon_seed).randn(N, args.L))
            latents = latent_samples_SVGPVAE(d_train_img, d_train_aux, VAE, SVGP_, clipping_qs=args.clip_qs, epsilon=eps)
            with open(chkpnt_dir + "latents_train_full.p", "wb") as f:
                pickle.dump(latents.cpu().numpy(), f)
        ctx.barrier()
    log["world_size"], log["rank"] = ctx.world, ctx.rank
    log["rccl_ranks"] = eng.comm.world_size if eng.comm is not None else 0
    log["total_time"] = time.time() - start
    if root and getattr(args, "log_json", None):
        eng.synchronize()
        json.dump(dict({k: v for k, v in log.items()}, theta=eng.theta.cpu().tolist(), adam_t=eng.scalars()["adam_t"],
                       param_order=list(eng.shapes)), open(args.log_json, "wt"))
    log["_engine"] = eng                     # (the final parameters / optimiser state for callers; not serialised)
    log["chkpnt_dir"] = chkpnt_dir           # (where --save wrote args.json and the model_<epoch>.pt files; None without it)
    if latents is not None:
        log["_latents"] = latents            # (N, L) device tensor of --save_latents; not serialised
    return log


def _refuse_restore(args):
    """--restore / --first_epoch exist for the two SVGPVAE objectives only; the other drivers refuse them instead of training
    from scratch."""
    if getattr(args, "restore", None) or getattr(args, "first_epoch", None):
        raise NotImplementedError(f"--restore / --first_epoch are implemented for --elbo SVGPVAE_Hensman | SVGPVAE_Titsias, "
                                  f"not for --elbo {args.elbo}")


def run_experiment_rotated_mnist_SVIGP_Hensman(args, args_dict=None):
    """MNIST_experiment.py:544-760.  Returns a dict of the logged series."""
    _refuse_restore(args)
    from .SVIGP_Hensman_model import SVIGP_Hensman, SVIGP_Hensman_decoder, SvigpStepEngine
    np.random.seed(args.seed)
    n = len(args.dataset)
    ending = args.dataset + ".p"
    train, ev, te, train_batches = import_rotated_mnist(args.mnist_data_path, ending, args.batch_size,
                                                        train_file=args.train_file)
    N_train = len(train["images"]) if args.train_file else n * 4050
    N_test = len(te["images"])
    chkpnt_dir = None
    if args.save:
        stamp = time.strftime("%d_%m_%Y__at__%H_%M_%S")
        chkpnt_dir = os.path.join(args.base_dir, args.expid, f"{args.elbo}_{args.beta}__on__{stamp}") + "/"
        os.makedirs(chkpnt_dir + "pics/", exist_ok=True)
        json.dump(args_dict or vars(args), open(chkpnt_dir + "args.json", "wt"))
    VAE = SVIGP_Hensman_decoder(L=args.L, seed=args.seed)                                  # :591
    inducing_points_init = generate_init_inducing_points(None, n=args.nr_inducing_points, remove_test_angle=None,
                                                         PCA=args.PCA, M=args.M, aux_data=train["aux_data"])
    if args.ov_joint:                                                                        # :603-612
        if args.PCA:
            object_vectors_init = pickle.load(open(args.mnist_data_path + f'pca_ov_init{args.dataset}.p', 'rb'))
        else:
            object_vectors_init = np.random.normal(0, 1.5, n * 400 * args.M).reshape(n * 400, args.M)
    else:
        object_vectors_init = None
    SVGP_ = SVIGP_Hensman(fixed_inducing_points=not args.ip_joint, initial_inducing_points=inducing_points_init,
                          fixed_gp_params=not args.GP_joint, object_vectors_init=object_vectors_init, name='main',
                          jitter=args.jitter, N_train=N_train, L=args.L, K_obj_normalize=args.object_kernel_normalize,
                          dtype=np.float64)                                                  # :616-620
    eng = SvigpStepEngine(VAE, SVGP_, b_max=args.batch_size, lr=args.lr)
    dev = eng.dev
    t64 = lambda a: torch.tensor(a, dtype=torch.float64, device=dev).contiguous()
    d_train_img, d_train_aux = t64(train["images"]), t64(train["aux_data"])
    d_test_img, d_test_aux = t64(te["images"]), t64(te["aux_data"])
    nr_epochs = args.nr_epochs if args.opt_regime == ['joint-1000'] else parse_opt_regime(args.opt_regime)[0]
    log = dict(epoch=[], elbo=[], recon_loss=[], cgen_mse=[], epoch_time=[])
    start = time.time()
    for epoch in range(nr_epochs):
        t0 = time.time()
        elbos, losses = [], []
        for lo, hi in train_batches:                                                         # :700-706
            eng.step(d_train_img[lo:hi], d_train_aux[lo:hi], adam=True)
            sc = eng.scalars()
            elbos.append(sc["elbo"]); losses.append(sc["recon_loss"])
        mse = float(np.sum(losses) / N_train)
        log["epoch"].append(epoch); log["elbo"].append(float(np.mean(elbos))); log["recon_loss"].append(mse)
        log["epoch_time"].append(time.time() - t0)
        if (epoch + 1) % _eval_every(args, 10) == 0 or epoch + 1 == nr_epochs:
            print(f"Epoch {epoch}, mean ELBO per batch: {np.mean(elbos)}")
            print(f"MSE loss on train set for epoch {epoch} : {mse}")
            cg = [float(eng.predict(d_test_img[lo:hi], d_test_aux[lo:hi])[1]) for lo, hi in batches(N_test, args.batch_size)]
            cgen = float(np.sum(cg) / N_test)                                               # :733-748
            log["cgen_mse"].append((epoch, cgen))
            l_GP, amp, _, _ = SVGP_.variable_summary()
            print(f"Conditional generation MSE loss on test set for epoch {epoch}: {cgen}   "
                  f"(l_GP {float(l_GP):.4f}, amplitude {float(amp):.4f}, noise {float(eng.vp['noise'][0]):.4f})", flush=True)
            if chkpnt_dir:
                with open(chkpnt_dir + "pics/test_metrics.txt", "a") as f:
                    f.write(f"{epoch},{mse},{cgen}\n")
                if args.save_model_weights:
                    torch.save({"theta": eng.mn.theta.cpu(), "phi": eng.phi.cpu(), "state": eng.mn.state.cpu()},
                               chkpnt_dir + f"model_{epoch}.pt")
    log["total_time"] = time.time() - start
    return log


def run_experiment_rotated_mnist_Casale(args, args_dict=None):
    """MNIST_experiment.py:786-1110.  Returns a dict of the logged series (per-step ELBO included)."""
    _refuse_restore(args)
    from .GPVAE_Casale_model import CasaleStepEngine, _angles_mask, casaleGP, sort_train_data
    np.random.seed(args.seed)
    n = len(args.dataset)
    GPLVM_ending = "" if args.M == 8 else "_{}".format(args.M)                                # :819
    ending = args.dataset + GPLVM_ending + ".p"
    load = lambda path: pickle.load(open(path, "rb"))
    train = sort_train_data(load(args.train_file or (args.mnist_data_path + "train_data" + ending)), dataset=args.dataset)
    mask_path = args.mnist_data_path + "train_ids_mask" + ending
    # the mask is a function of the train rows; a stored one is only used when it fits them
    train_ids_mask = load(mask_path) if os.path.exists(mask_path) and not args.train_file else _angles_mask(train["aux_data"][:, 1:])
    te = load(args.mnist_data_path + "test_data" + ending)
    N_train, N_test = len(train["images"]), len(te["images"])
    if int(np.sum(train_ids_mask)) != N_train:
        raise ValueError(f"train_ids_mask selects {int(np.sum(train_ids_mask))} (object, angle) pairs for {N_train} train rows")
    chkpnt_dir = None
    if args.save:
        stamp = time.strftime("%d_%m_%Y__at__%H_%M_%S")
        chkpnt_dir = os.path.join(args.base_dir, args.expid, f"{args.elbo}_{args.beta}__on__{stamp}") + "/"
        os.makedirs(chkpnt_dir + "pics/", exist_ok=True)
        json.dump({k: v for k, v in (args_dict or vars(args)).items() if not callable(v)}, open(chkpnt_dir + "args.json", "wt"))
    VAE = mnistVAE(L=args.L, seed=args.seed)                                                   # :846
    if args.PCA:                                                                               # :849-855
        object_vectors_init = load(args.mnist_data_path + "pca_ov_init{}{}.p".format(args.dataset, GPLVM_ending))
    else:
        assert args.ov_joint, "If --ov_joint is not used, at least PCA initialization must be utilized."
        object_vectors_init = np.random.normal(0, 1.5, n * 400 * args.M).reshape(n * 400, args.M)
    GP = casaleGP(fixed_gp_params=not args.GP_joint, object_vectors_init=object_vectors_init,
                  object_kernel_normalize=args.object_kernel_normalize, ov_joint=args.ov_joint)   # :848, :857 (sic)
    train_aux = train["aux_data"][:, :3]                       # [global id, object id, angle]: the step reads nothing else
    eng = CasaleStepEngine(VAE, GP, train["images"], train_aux, batch_size=args.batch_size, beta=args.beta,
                           clipping_qs=args.clip_qs)
    print(f"Number of train params: {eng.n_total}")
    nr_epochs, training_regime = parse_opt_regime(args.opt_regime)                              # :978
    train_batches = batches(N_train, args.batch_size)
    every = _eval_every(args, 5)                                                                # :1067
    L = args.L
    d_test_img = torch.tensor(te["images"], dtype=torch.float64, device=eng.dev).contiguous()
    log = dict(epoch=[], regime=[], elbo=[], recon_loss=[], step_elbo=[], cgen_mse=[], epoch_time=[])
    start, recon_images_cgen = time.time(), None
    for epoch in range(nr_epochs):
        regime, t0 = training_regime[epoch], time.time()
        elbos, losses = [], []
        for i, (lo, hi) in enumerate(train_batches):                                            # :1018-1025
            eps_f = eps_b = None
            if args.epsilon_seed is not None:
                eps_f = np.random.RandomState(1000 * epoch + i + args.epsilon_seed).randn(N_train, L)
                eps_b = np.random.RandomState(500000 + 1000 * epoch + i + args.epsilon_seed).randn(hi - lo, L)
            eng.step(regime, lo, hi, eps_full=eps_f, eps_batch=eps_b, adam=True)
            sc = eng.scalars()
            elbos.append(sc["elbo"]); losses.append(sc["recon_loss"])
        mse = float(np.sum(losses) / N_train)
        log["epoch"].append(epoch); log["regime"].append(regime); log["elbo"].append(float(np.mean(elbos)))
        log["recon_loss"].append(mse); log["step_elbo"].extend(elbos); log["epoch_time"].append(time.time() - t0)
        print(f"Epoch {epoch}, opt regime {regime}, mean ELBO per batch: {np.mean(elbos)}")
        print(f"Epoch {epoch}, opt regime {regime}, MSE loss on train set: {mse}")
        print(f"Time elapsed for epoch {epoch}, opt regime {regime}: {time.time() - t0}", flush=True)
        if (epoch + 1) % every == 0:                                                            # :1067-1098
            eps_f = eps_t = None
            if args.epsilon_seed is not None:
                eps_f = np.random.RandomState(900000 + epoch + args.epsilon_seed).randn(N_train, L)
                eps_t = np.random.RandomState(950000 + epoch + args.epsilon_seed).randn(N_test, L)
            recon_images_cgen, cgen = eng.predict(d_test_img, te["aux_data"], eps_full=eps_f, epsilon=eps_t)
            cgen = float(cgen)
            log["cgen_mse"].append((epoch, cgen))
            print(f"Conditional generation MSE loss on test set for epoch {epoch}: {cgen}", flush=True)
            if chkpnt_dir:
                with open(chkpnt_dir + "pics/test_metrics.txt", "a") as f:
                    f.write("{},{}\n".format(epoch + 1, round(cgen, 4)))
                if args.save_model_weights:
                    eng.synchronize()
                    torch.save({"theta": eng.theta.cpu(), "adam_m": eng.adam_m.cpu(), "adam_v": eng.adam_v.cpu(),
                                "state": eng.state.cpu()}, chkpnt_dir + f"model_{int(eng.scalars()['adam_t'])}.pt")
    log["total_time"] = time.time() - start
    print("Running time for {} epochs: {}".format(nr_epochs, round(log["total_time"], 2)))
    if log["cgen_mse"]:
        best = sorted(log["cgen_mse"], key=lambda x: x[1])[0]
        print("Best cgen MSE on test set throughout training at epoch {}: {}".format(best[0], best[1]))
    if chkpnt_dir and recon_images_cgen is not None:
        with open(chkpnt_dir + "cgen_images.p", "wb") as f:
            pickle.dump(recon_images_cgen.cpu().numpy(), f)
    log["chkpnt_dir"] = chkpnt_dir
    if args.log_json:
        eng.synchronize()
        out = {k: v for k, v in log.items()}
        out["theta"] = eng.theta.cpu().tolist()
        json.dump(out, open(args.log_json, "wt"))
    return log


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.elbo in ("SVGPVAE_Hensman", "SVGPVAE_Titsias"):
        from .dp import DistContext
        ctx = DistContext()
        try:
            return run_experiment_rotated_mnist_SVGPVAE(args, vars(args), ctx)
        finally:
            ctx.close()
    if args.elbo == "SVIGP_Hensman":
        return run_experiment_rotated_mnist_SVIGP_Hensman(args, vars(args))
    if args.elbo == "GPVAE_Casale":
        return run_experiment_rotated_mnist_Casale(args, vars(args))
    if args.elbo in ("VAE", "CVAE"):
        raise NotImplementedError(f"--elbo {args.elbo} runs under its own driver: python -m svgp_vae_amd.VAE_experiment --elbo {args.elbo} ... "
                                  f"(same flags; DESIGN.md section 9k)")
    raise NotImplementedError(f"--elbo {args.elbo}: only SVGPVAE_Hensman / SVGPVAE_Titsias / SVIGP_Hensman / GPVAE_Casale are built "
                              f"(see DESIGN.md section 9)")


if __name__ == "__main__":
    main()
