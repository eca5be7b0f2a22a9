"""Rotated-MNIST driver for the two baselines without a GP: `--elbo VAE` (mnistVAE) and `--elbo CVAE` (mnistCVAE).

    python -m svgp_vae_amd.VAE_experiment --elbo CVAE --mnist_data_path "MNIST data/" --nr_epochs 100 --save

The command line is MNIST_experiment.build_parser(), unchanged.  Mirrors run_experiment_rotated_mnist_SVGPVAE
(MNIST_experiment.py:30-541) for these two values of --elbo:
  * nr_epochs = --nr_epochs; --opt_regime is not read (sic, :53-58);
  * un-shuffled batches, the last one ragged; every step minimises -elbo of forward_pass_standard_VAE_rotated_mnist with TF1 Adam
    (:142-148, 205, 343-346) -- one image launch and one reduction + Adam launch (csrc/cvae.hip);
  * the forward pass is built without clipping_qs (:144-148), so --clip_qs has NO effect here (sic);
  * every --eval_every epochs (default 10): the train MSE, the test-set reconstruction MSE (sum of the batches' recon_loss / N_test)
    and, for CVAE, the conditional-generation MSE of predict_CVAE (:488-494); with --save the line `epoch+1,round(MSE,4),round(cgen,4)`
    in pics/test_metrics.txt and cgen_images.p (CVAE), with --save_model_weights also model_<epoch>.pt (theta, adam_m, adam_v, state).
Refused: --GECO (the reference would then descend on +elbo, :202-203), --save_latents (the reference calls a function it does not
define, :187), --bias_analysis, --restore / --first_epoch, and every other --elbo value (python -m svgp_vae_amd.MNIST_experiment).
Plots and the pandas logging of the reference are not reproduced.
"""
import json
import os
import pickle
import time

import numpy as np
import torch

from .MNIST_experiment import _eval_every, build_parser
from .utils import batches, import_rotated_mnist


def check_args(args):
    if args.elbo not in ("VAE", "CVAE"):
        raise NotImplementedError(f"--elbo {args.elbo}: this driver runs --elbo VAE | CVAE; the other objectives run under "
                                  f"python -m svgp_vae_amd.MNIST_experiment --elbo {args.elbo} ...")
    if args.GECO:
        raise NotImplementedError(f"--GECO with --elbo {args.elbo}: the reference would then apply the gradients of +elbo "
                                  f"(MNIST_experiment.py:202-203) and ascend the loss; refused")
    if args.save_latents:
        raise NotImplementedError(f"--save_latents with --elbo {args.elbo}: the reference calls latent_samples_VAE_full_train, "
                                  f"which it does not define (MNIST_experiment.py:187); refused")
    if args.bias_analysis:
        raise NotImplementedError(f"--bias_analysis needs the inducing mean vectors of an SVGPVAE objective, not --elbo {args.elbo}")
    if getattr(args, "restore", None) or getattr(args, "first_epoch", None):
        raise NotImplementedError(f"--restore / --first_epoch are implemented for --elbo SVGPVAE_Hensman | SVGPVAE_Titsias, "
                                  f"not for --elbo {args.elbo}")


def run_experiment_rotated_mnist_VAE(args, args_dict=None):
    """Returns the log dict: per-epoch `elbo` and `recon_loss` (train MSE per pixel: sum of the steps' recon_loss / N_train), per-step
    `step_elbo`, and the (epoch, value) series `test_mse`, `cgen_mse` (CVAE); `chkpnt_dir`, `_engine`."""
    from .CVAE_model import VaeStepEngine, forward_pass_standard_VAE_rotated_mnist, mnistCVAE, predict_CVAE
    from .VAE_utils import mnistVAE
    check_args(args)
    cvae = args.elbo == "CVAE"
    np.random.seed(args.seed)
    ending = args.dataset + ".p"
    train, ev, te, train_batches = import_rotated_mnist(args.mnist_data_path, ending, args.batch_size, train_file=args.train_file)
    N_train, N_test = len(train["images"]), len(te["images"])
    chkpnt_dir = None
    if args.save:
        stamp = time.strftime("%d_%m_%Y__at__%H_%M_%S")
        chkpnt_dir = os.path.join(args.base_dir, args.expid, f"{args.elbo}_{args.beta}__on__{stamp}") + "/"
        os.makedirs(chkpnt_dir + "pics/", exist_ok=True)
        json.dump({k: v for k, v in (args_dict or vars(args)).items() if not callable(v)}, open(chkpnt_dir + "args.json", "wt"))
    VAE = (mnistCVAE if cvae else mnistVAE)(L=args.L, seed=args.seed)
    eng = VaeStepEngine(VAE, b_max=args.batch_size, lr=args.lr, clip_qs=False, sigma=0.01, store=False)
    dev = eng.dev
    print(f"Number of train params: {eng.n_total}")
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64, device=dev).contiguous()
    d_train_img, d_train_aux = t64(train["images"]), t64(train["aux_data"])[:, :2].contiguous()
    d_test_img, d_test_aux = t64(te["images"]), t64(te["aux_data"])[:, :2].contiguous()
    eps_fn = getattr(args, "epsilon_fn", None)
    if eps_fn is None and getattr(args, "epsilon_seed", None) is not None:
        eps_fn = lambda epoch, i, rows, L_: np.random.RandomState(1000 * epoch + i + args.epsilon_seed).randn(rows, L_)
    if eps_fn is None:
        eng.set_rng_counter(float(np.random.randint(0, 2 ** 31)))
    nr_epochs, every = args.nr_epochs, _eval_every(args, 10)
    log = dict(elbo=[], recon_loss=[], step_elbo=[], test_mse=[], cgen_mse=[])
    recon_images_cgen = None
    start = time.time()
    for epoch in range(nr_epochs):
        elbos, losses = [], []
        for i, (lo, hi) in enumerate(train_batches):
            eps = None if eps_fn is None else np.asarray(eps_fn(epoch, i, hi - lo, args.L))
            eng.step(d_train_img[lo:hi], d_train_aux[lo:hi], eps, adam=True)
            sc = eng.scalars()          # the reference fetches elbo and recon_loss every step (:343-346)
            elbos.append(sc["elbo"]); losses.append(sc["recon_loss"])
        log["step_elbo"].extend(elbos)
        log["elbo"].append(float(np.sum(elbos)))
        log["recon_loss"].append(float(np.sum(losses) / N_train))
        if not ((epoch + 1) % every == 0 or epoch + 1 == nr_epochs):
            continue
        print(f"Epoch {epoch}: elbo {log['elbo'][-1]:.4f}   train MSE/px {log['recon_loss'][-1]:.6f}", flush=True)
        te_losses = []
        for lo, hi in batches(N_test, args.batch_size):
            out = forward_pass_standard_VAE_rotated_mnist((d_test_img[lo:hi], d_test_aux[lo:hi]), VAE, CVAE=cvae)
            te_losses.append(float(out[0]))
        MSE = float(np.sum(te_losses) / N_test)
        log["test_mse"].append((epoch, MSE))
        print(f"  test recon MSE/px {MSE:.6f}", flush=True)
        cgen = None
        if cvae:
            recon_images_cgen, loss = predict_CVAE(d_train_img, d_test_img, d_train_aux, d_test_aux, VAE,
                                                   test_indices=te["aux_data"][:, 0])
            cgen = float(loss)
            log["cgen_mse"].append((epoch, cgen))
            print("Conditional generation MSE loss on test set for epoch {}: {}".format(epoch, cgen), flush=True)
        if chkpnt_dir:
            if cvae:
                with open(chkpnt_dir + "pics/test_metrics.txt", "a") as f:
                    f.write("{},{},{}\n".format(epoch + 1, round(MSE, 4), round(cgen, 4)))
            if args.save_model_weights:
                eng.synchronize()
                torch.save({"theta": eng.theta.cpu(), "adam_m": eng.adam_m.cpu(), "adam_v": eng.adam_v.cpu(), "state": eng.state.cpu()},
                           chkpnt_dir + f"model_{epoch}.pt")
    print("Running time for {} epochs: {}".format(nr_epochs, round(time.time() - start, 2)))
    if chkpnt_dir and cvae and recon_images_cgen is not None:
        with open(chkpnt_dir + "cgen_images.p", "wb") as f:
            pickle.dump(recon_images_cgen.cpu().numpy(), f)
    log["chkpnt_dir"] = chkpnt_dir
    if getattr(args, "log_json", None):
        eng.synchronize()
        with open(args.log_json, "wt") as f:
            json.dump(dict({k: v for k, v in log.items()}, theta=eng.theta.cpu().tolist(), adam_t=eng.scalars()["adam_t"],
                           param_order=list(eng.shapes)), f)
    log["_engine"] = eng
    return log


def parser():
    p = build_parser()
    p.description = "Rotated MNIST, --elbo VAE | CVAE (one image launch per step).  --clip_qs has no effect for these two objectives: " \
                    "the reference builds their forward pass without clipping."
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    return run_experiment_rotated_mnist_VAE(args, vars(args))


if __name__ == "__main__":
    main()
