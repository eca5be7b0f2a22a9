"""Conditional generation from a trained rotated-MNIST SVGP-VAE without the train set: the posterior cache.

The GP posterior of mainSVGP.approximate_posterior_params (SVGPVAE_model.py:303-343) depends on the train rows only through
w_l = c (Sigma_l + jI)^-1 v_l and X_l = (Sigma_l + jI)^-1 - (K_mm + jI)^-1.  PosteriorCache.build walks the
train rows ONCE in chunks (an engine of `chunk` rows, not of N), `generate` then turns query rows [id, angle, o_1..o_M] into
images: one launch per batch for m <= 64 (svgp_mnist_generate), no train row touched, no random-number state touched.

    cache = PosteriorCache.build(vae, svgp, train_images, train_aux, chunk=1024, clip_qs=True)
    images = generate(cache, aux)                      # (b, 28, 28, 1): decode of the posterior mean
    images, p_m, p_v = generate(cache, aux, eps=eps, return_moments=True)

Command line (the model's shape and flags come from the args.json the driver writes beside its checkpoints):

    python -m svgp_vae_amd.generate --checkpoint RUN/model_<k>.pt --mnist_data_path DIR [--train_file F]
        (--ids I.. --n_angles A | --aux_file rows.npy) [--sample --seed S] --out images.npy
"""
import argparse
import ctypes as C
import json
import os

import numpy as np
import torch

from . import _lib
from ._lib import CacheLayout, MnistCfg, ParamLayout, call
from .engine import _LAYOUT_NAME, param_shapes

_F64 = torch.float64
GEN_ROWS = 256          # m > 64: query rows per svgp_mnist_generate call (the workspace holds L x GEN_ROWS x m products);
                        # m <= 64 needs no workspace and the kernel strides over any number of rows: one call per batch
_SHAPE_KEYS = ("m", "L", "M", "n_obj", "normalize_obj", "N_train", "jitter")


def _cfg(shape, b, b_cap):
    return MnistCfg(b=b, b_global=b, b_cap=b_cap, m=shape["m"], L=shape["L"], M=shape["M"], n_obj=shape["n_obj"],
                    normalize_obj=shape["normalize_obj"], N_train=shape["N_train"], jitter=shape["jitter"], rep_weight=1.0)


class PosteriorCache:
    """[acc_S | acc_v | acc_rows | w | X] of svgp_mnist_cache_layout (`data`, one float64 device tensor) with the flat parameter
    vector `theta` it was built for and the shape fields: the whole deployed model."""

    def __init__(self, shape, theta, data, device="cuda:0"):
        _lib.load_library()
        if not torch.cuda.is_available():
            raise _lib.SvgpError("PosteriorCache needs a HIP device; there is no CPU execution path")
        self.shape = {k: (float(shape[k]) if k in ("N_train", "jitter") else int(shape[k])) for k in _SHAPE_KEYS}
        self.device = torch.device(device)
        self.cl, self.pl = CacheLayout(), ParamLayout()
        cfg = _cfg(self.shape, 1, GEN_ROWS)
        call("svgp_mnist_cache_layout_get", C.byref(cfg), C.byref(self.cl))
        call("svgp_mnist_param_layout_get", C.byref(cfg), C.byref(self.pl))
        self.theta = torch.as_tensor(theta, dtype=_F64).reshape(-1).to(self.device).contiguous()
        if self.theta.numel() != self.pl.n_total:
            raise ValueError(f"theta has {self.theta.numel()} elements, the shape {self.shape} needs {self.pl.n_total}")
        self.data = (torch.zeros(self.cl.total, dtype=_F64, device=self.device) if data is None
                     else torch.as_tensor(data, dtype=_F64).reshape(-1).to(self.device).contiguous())
        if self.data.numel() != self.cl.total:
            raise ValueError(f"cache has {self.data.numel()} elements, the shape {self.shape} needs {self.cl.total}")
        self.stream = torch.cuda.Stream(device=self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        n_work = int(self.lib_elems("svgp_mnist_generate_workspace_elems", _cfg(self.shape, GEN_ROWS, GEN_ROWS)))
        self.work = torch.empty(n_work, dtype=_F64, device=self.device) if n_work else None

    @staticmethod
    def lib_elems(name, cfg):
        return getattr(_lib.load_library(), name)(C.byref(cfg))

    def field(self, name, shape=None):
        """View of a cache field (acc_S, acc_v, acc_rows, w, X)."""
        m, L = self.shape["m"], self.shape["L"]
        shp = shape or dict(acc_S=(L, m, m), acc_v=(L, m), acc_rows=(1,), w=(L, m), X=(L, m, m))[name]
        off = getattr(self.cl, name)
        return self.data[off:off + int(np.prod(shp))].view(shp)

    # ------------------------------------------------------------------ build
    @classmethod
    def build(cls, vae, svgp, train_images, train_aux, chunk=1024, clip_qs=True):
        """Walks the train rows in chunks of `chunk` (ragged last chunk) on an engine of min(chunk, N) rows: encoder, kernel
        matrices, statistics, svgp_gp_stats_accumulate; then svgp_mnist_cache_build.  c = svgp.N_train / accumulated rows, as
        approximate_posterior_params forms it from the rows it is given."""
        from .engine import MnistStepEngine
        N = int(train_images.shape[0])
        if N < 1 or int(train_aux.shape[0]) != N:
            raise ValueError(f"train_images has {N} rows, train_aux {int(train_aux.shape[0])}")
        chunk = max(1, min(int(chunk), N))
        M = svgp.inducing_index_points.shape[1] - 2
        n_obj = 0 if svgp.object_vectors is None else svgp.object_vectors.shape[0]
        eng = MnistStepEngine(svgp.nr_inducing, vae.L, M, n_obj, N_train=svgp.N_train, jitter=svgp.jitter, clip_qs=clip_qs,
                              geco=False, K_obj_normalize=svgp.K_obj_normalize, b_max=chunk, device=svgp.device)
        params = {k: v.detach() for k, v in vae.params.items()}
        params.update({k: v.detach() for k, v in svgp._params().items()})
        eng.load_params(params)
        shape = dict(m=svgp.nr_inducing, L=vae.L, M=M, n_obj=n_obj, normalize_obj=int(svgp.K_obj_normalize),
                     N_train=svgp.N_train, jitter=svgp.jitter)
        self = cls(shape, eng.theta.clone(), None, device=eng.device)
        dev = eng.device
        d_img = train_images.to(dev, _F64).contiguous()
        d_aux = train_aux.to(dev, _F64).contiguous()
        n_work = int(cls.lib_elems("svgp_mnist_cache_workspace_elems", _cfg(shape, 1, 1)))
        work = torch.empty(n_work, dtype=_F64, device=dev) if n_work else None
        eng.stream.wait_stream(torch.cuda.current_stream(dev))
        eng.stream.wait_stream(self.stream)
        th, ws, s = eng.theta.data_ptr(), eng.ws.data_ptr(), eng.stream.cuda_stream
        with torch.cuda.stream(eng.stream):
            for lo in range(0, N, chunk):
                n = min(chunk, N - lo)
                eng.set_batch_size(n, n)
                cfg = C.byref(eng.cfg)
                call("svgp_mnist_encoder_fwd", cfg, th, d_img[lo:lo + n].data_ptr(), ws, s)
                call("svgp_kernel_matrix_fwd", cfg, th, d_aux[lo:lo + n].data_ptr(), ws, s)
                call("svgp_gp_stats_fwd", cfg, ws, s)
                call("svgp_gp_stats_accumulate", cfg, ws, self.data.data_ptr(), int(lo == 0), s)
            call("svgp_mnist_cache_build", C.byref(eng.cfg), th, self.data.data_ptr(), None if work is None else work.data_ptr(), s)
        eng.synchronize()
        return self

    # ------------------------------------------------------------------ files
    def save(self, path):
        """One tensor (the cache), the parameter vector and the shape fields."""
        torch.cuda.synchronize(self.device)
        torch.save({"cache": self.data.cpu(), "theta": self.theta.cpu(), "shape": dict(self.shape)}, path)

    @classmethod
    def load(cls, path, device="cuda:0"):
        ck = torch.load(path, map_location="cpu")
        if not isinstance(ck, dict) or any(k not in ck for k in ("cache", "theta", "shape")):
            raise ValueError(f"{path}: not a posterior cache file")
        return cls(ck["shape"], ck["theta"], ck["cache"], device=device)


def generate(cache, aux, eps=None, gather=True, return_moments=False):
    """Images (b, 28, 28, 1) at the query rows aux (b, 2+M) = [id, angle, o_1..o_M]: decode(p_m + eps sqrt(p_v)); eps (b, L) None:
    decode of the posterior mean.  gather: the object vector of a row is the model's table row `id` (needs a table); False: the
    row's own columns 2:, the way to generate for an object that is not in the table.  return_moments: (images, p_m, p_v).
    Any b works: m <= 64 is ONE launch for the whole batch, beyond that the rows go through calls of GEN_ROWS rows."""
    sh, dev = cache.shape, cache.device
    aux = torch.as_tensor(aux, dtype=_F64)
    if aux.dim() != 2 or aux.shape[1] != 2 + sh["M"]:
        raise ValueError(f"aux must be (b, {2 + sh['M']}) rows [id, angle, object vector], got {tuple(aux.shape)}")
    b = int(aux.shape[0])
    if gather:
        if sh["n_obj"] < 1:
            raise ValueError("gather=True needs a model with an object-vector table; pass gather=False and the vectors in aux")
        ids = aux[:, 0]
        if b and not bool(((ids >= 0) & (ids < sh["n_obj"]) & (ids == ids.floor())).all()):
            raise ValueError(f"ids in aux[:, 0] must be integers in [0, {sh['n_obj']})")
    d_aux = aux.to(dev).contiguous()
    d_eps = None
    if eps is not None:
        d_eps = torch.as_tensor(eps, dtype=_F64).to(dev).contiguous()
        if d_eps.shape != (b, sh["L"]):
            raise ValueError(f"eps must be ({b}, {sh['L']}), got {tuple(d_eps.shape)}")
    images = torch.empty(b, 28, 28, 1, dtype=_F64, device=dev)
    p_m = torch.empty(b, sh["L"], dtype=_F64, device=dev) if return_moments else None
    p_v = torch.empty(b, sh["L"], dtype=_F64, device=dev) if return_moments else None
    cache.stream.wait_stream(torch.cuda.current_stream(dev))
    ptr = lambda t, lo: None if t is None else t[lo:].data_ptr()
    step = GEN_ROWS if cache.work is not None else max(b, 1)
    for lo in range(0, b, step):
        cfg = _cfg(sh, min(step, b - lo), step)
        call("svgp_mnist_generate", C.byref(cfg), cache.theta.data_ptr(), cache.data.data_ptr(), ptr(d_aux, lo), int(bool(gather)),
             ptr(d_eps, lo), ptr(images, lo), ptr(p_m, lo), ptr(p_v, lo), None if cache.work is None else cache.work.data_ptr(),
             cache.stream.cuda_stream)
    cache.stream.synchronize()
    return (images, p_m, p_v) if return_moments else images


def route(cache_or_shape):
    """The kernels of one generate batch, in launch order (svgp_mnist_generate_route); needs no device."""
    sh = cache_or_shape.shape if hasattr(cache_or_shape, "shape") and isinstance(cache_or_shape.shape, dict) else cache_or_shape
    buf = C.create_string_buffer(1024)
    call("svgp_mnist_generate_route", C.byref(_cfg(sh, 1, 1)), buf, len(buf))
    return buf.value.decode().split()


# ---------------------------------------------------------------------------------------------- command line
def models_from_run(checkpoint_path, train_aux, mnist_data_path=None, device="cuda:0"):
    """(vae, svgp, args dict) of the run that wrote `checkpoint_path`: the shapes and flags from its args.json, the parameters from
    the checkpoint's theta."""
    from . import checkpoint
    from .SVGPVAE_model import mnistSVGP
    from .VAE_utils import mnistVAE
    run_dir = os.path.dirname(os.path.abspath(checkpoint_path))
    with open(os.path.join(run_dir, "args.json")) as f:
        a = json.load(f)
    if a.get("elbo") not in ("SVGPVAE_Hensman", "SVGPVAE_Titsias"):
        raise ValueError(f"{run_dir}/args.json: --elbo {a.get('elbo')} is not an SVGPVAE run")
    ck = checkpoint.load(checkpoint_path)
    L, M = int(a["L"]), int(a["M"])
    n_obj = 0
    # the table as run_experiment_rotated_mnist_SVGPVAE builds it (MNIST_experiment.py, "model": object_vectors_init): the rows of
    # pca_ov_init<dataset>.p with --PCA, else 400 objects per digit; keep the two in step (the checkpoint format carries no shapes)
    if a.get("ov_joint"):
        n_obj = len(a["dataset"]) * 400
        if a.get("PCA"):
            import pickle
            with open((mnist_data_path or a["mnist_data_path"]) + f"pca_ov_init{a['dataset']}.p", "rb") as f:
                n_obj = len(pickle.load(f))
    # the number of inducing points is the one unknown of the parameter count: n_total is affine in m
    cfg0 = MnistCfg(b=1, b_global=1, m=1, L=L, M=M, n_obj=n_obj, N_train=1.0, rep_weight=1.0)
    pl = ParamLayout()
    call("svgp_mnist_param_layout_get", C.byref(cfg0), C.byref(pl))
    m, rem = divmod(ck["theta"].numel() - (pl.n_total - (2 + M)), 2 + M)
    if rem or m < 1:
        raise ValueError(f"{checkpoint_path}: theta has {ck['theta'].numel()} elements, which fits no number of inducing points "
                         f"for L={L}, M={M}, n_obj={n_obj}")
    cfg0.m = m
    call("svgp_mnist_param_layout_get", C.byref(cfg0), C.byref(pl))
    shapes, theta = param_shapes(m, L, M, n_obj), ck["theta"]
    take = lambda k: theta[getattr(pl, _LAYOUT_NAME.get(k, k)):][:int(np.prod(shapes[k], dtype=np.int64))].view(shapes[k]).clone()
    vae = mnistVAE(L=L, seed=int(a.get("seed", 0)), device=device)
    vae.params = {k: take(k) for k in vae.params}
    N_train = len(train_aux) if a.get("train_file") else len(a["dataset"]) * 4050
    svgp = mnistSVGP(titsias="Titsias" in a["elbo"], fixed_inducing_points=not a.get("ip_joint"),
                     initial_inducing_points=take("inducing_index_points").numpy(), fixed_gp_params=not a.get("GP_joint"),
                     object_vectors_init=take("object_vectors").numpy() if n_obj else None, name="main",
                     jitter=float(a["jitter"]), N_train=N_train, L=L, K_obj_normalize=bool(a.get("object_kernel_normalize")),
                     device=device)
    svgp.l_GP, svgp.amplitude = take("l_GP"), take("amplitude")
    return vae, svgp, a


def rotation_sweep(ids, n_angles, M):
    """ids x n_angles equally spaced angles in [0, 2 pi): rows [id, angle, 0..0], id-major."""
    ang = np.linspace(0.0, 2.0 * np.pi, int(n_angles), endpoint=False)
    rows = np.zeros((len(ids) * len(ang), 2 + M))
    rows[:, 0] = np.repeat(np.asarray(ids, dtype=np.float64), len(ang))
    rows[:, 1] = np.tile(ang, len(ids))
    return rows


def build_parser():
    p = argparse.ArgumentParser(description="Images from a trained rotated-MNIST SVGP-VAE checkpoint.")
    p.add_argument("--checkpoint", required=True, help="RUN/model_<k>.pt of MNIST_experiment --save --save_model_weights")
    p.add_argument("--mnist_data_path", type=str, default=None, help="default: the run's own --mnist_data_path (args.json)")
    p.add_argument("--train_file", type=str, default=None, help="train pickle; default: the run's, else train_data<dataset>.p")
    p.add_argument("--ids", type=int, nargs="+", default=None, help="object ids of the rotation sweep")
    p.add_argument("--n_angles", type=int, default=16)
    p.add_argument("--aux_file", type=str, default=None, help=".npy of query rows [id, angle, o_1..o_M] instead of --ids")
    p.add_argument("--sample", action="store_true", help="z = p_m + eps sqrt(p_v) with eps from --seed; default: the posterior mean")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--chunk", type=int, default=1024)
    p.add_argument("--out", required=True)
    return p


def main(argv=None):
    import pickle
    args = build_parser().parse_args(argv)
    if (args.ids is None) == (args.aux_file is None):
        raise SystemExit("give either --ids (with --n_angles) or --aux_file")
    with open(os.path.join(os.path.dirname(os.path.abspath(args.checkpoint)), "args.json")) as f:
        run_args = json.load(f)
    data_path = args.mnist_data_path or run_args["mnist_data_path"]
    train_file = args.train_file or run_args.get("train_file") or (data_path + "train_data" + run_args["dataset"] + ".p")
    with open(train_file, "rb") as f:
        train = pickle.load(f)
    images = torch.as_tensor(np.asarray(train["images"], dtype=np.float64))
    aux = torch.as_tensor(np.asarray(train["aux_data"], dtype=np.float64))
    vae, svgp, a = models_from_run(args.checkpoint, aux, data_path)
    cache = PosteriorCache.build(vae, svgp, images, aux, chunk=args.chunk, clip_qs=bool(a.get("clip_qs")))
    gather = svgp.object_vectors is not None
    rows = rotation_sweep(args.ids, args.n_angles, int(a["M"])) if args.ids is not None else np.load(args.aux_file)
    if args.ids is not None and not gather:
        raise SystemExit("--ids needs a model with an object-vector table (--ov_joint); use --aux_file with the vectors")
    eps = np.random.RandomState(args.seed).randn(len(rows), int(a["L"])) if args.sample else None
    out = generate(cache, rows, eps=eps, gather=gather)
    np.save(args.out, out.cpu().numpy())
    print(f"{len(rows)} images -> {args.out}   route: {' '.join(route(cache))}")
    return out


if __name__ == "__main__":
    main()
