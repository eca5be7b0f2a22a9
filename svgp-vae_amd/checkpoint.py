"""Checkpoints of the rotated-MNIST driver: the dict that `MNIST_experiment --save --save_model_weights` writes as
model_<epoch>.pt -- `theta` (flat parameters), `adam_m`, `adam_v` (Adam moments) and `state` (the device state vector: Adam's
step count, the GECO pair C_ma / lagrange multiplier, the first-step alpha, lr, beta, the RNG counter).  Together they are the
whole training state of a MnistStepEngine, so an engine restored from such a file continues bit for bit."""
import os
import re

import torch

KEYS = ("theta", "adam_m", "adam_v", "state")


def load(path):
    """The checkpoint dict as float64 CPU tensors.  Refuses a file that lacks one of the four entries or whose entries
    disagree in length."""
    ck = torch.load(path, map_location="cpu")
    if not isinstance(ck, dict) or any(k not in ck for k in KEYS):
        raise ValueError(f"{path}: not a checkpoint of the rotated-MNIST driver (needs {', '.join(KEYS)})")
    out = {k: torch.as_tensor(ck[k], dtype=torch.float64).reshape(-1).contiguous() for k in KEYS}
    n = out["theta"].numel()
    if out["adam_m"].numel() != n or out["adam_v"].numel() != n:
        raise ValueError(f"{path}: theta has {n} elements but adam_m / adam_v have {out['adam_m'].numel()} / "
                         f"{out['adam_v'].numel()}")
    return out


def restore(eng, path):
    """Copies a checkpoint into `eng` (anything with pl.n_total, theta, adam_m, adam_v, state; a MnistStepEngine): on the
    engine's stream when it has one.  A file whose theta length is not the engine's n_total belongs to another model shape
    and is refused with both numbers."""
    ck = load(path)
    n_file, n_eng = ck["theta"].numel(), int(eng.pl.n_total)
    if n_file != n_eng:
        raise ValueError(f"{path}: theta has {n_file} elements but the engine's parameter vector has {n_eng} "
                         f"(another --nr_inducing_points / --L / --M / data set?)")
    if ck["state"].numel() != eng.state.numel():
        raise ValueError(f"{path}: state has {ck['state'].numel()} elements but the engine's has {eng.state.numel()}")
    stream = getattr(eng, "stream", None)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(eng.theta.device))
        with torch.cuda.stream(stream):
            for k in KEYS:
                getattr(eng, k).copy_(ck[k])
        stream.synchronize()
    else:
        for k in KEYS:
            getattr(eng, k).copy_(ck[k])
    return ck


def first_epoch_of(path):
    """model_<k>.pt was written after epoch k: the run continues with k + 1; any other name: 0."""
    m = re.fullmatch(r"model_(\d+)\.pt", os.path.basename(path))
    return int(m.group(1)) + 1 if m else 0
