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

The Casale GP-VAE baseline (--elbo GPVAE_Casale) has the same two steps: CasalePosteriorCache keeps P = (alpha I + V^T V)^-1, U = P V^T Z
and L_W, `generate` dispatches on the cache type, and the command line takes a GPVAE_Casale checkpoint too
([--latent sample|mean --latent_seed S] choose the latent rows of the train set).
"""
import argparse
import ctypes as C
import json
import os

import numpy as np
import torch

from . import _lib
from ._lib import CacheLayout, CasaleCacheLayout, CasaleCfg, CasaleLayout, MnistCfg, ParamLayout, call
from .engine import _LAYOUT_NAME, param_shapes

_F64 = torch.float64
GEN_ROWS = 256          # m > 64: query rows per svgp_mnist_generate call (the workspace holds L x GEN_ROWS x m products);
                        # m <= 64 needs no workspace and the kernel strides over any number of rows: one call per batch
_SHAPE_KEYS = ("m", "L", "M", "n_obj", "normalize_obj", "N_train", "jitter")


def _cfg(shape, b, b_cap):
    return MnistCfg(b=b, b_global=b, b_cap=b_cap, m=shape["m"], L=shape["L"], M=shape["M"], n_obj=shape["n_obj"],
                    normalize_obj=shape["normalize_obj"], N_train=shape["N_train"], jitter=shape["jitter"], rep_weight=1.0)


class _Cache:
    """What the two posterior caches share: the parameter vector `theta` and the cache `data` as float64 device tensors of the
    lengths the shape asks for, a stream, and the file {_KEY: data, "theta", "shape"}.  A subclass's _layouts(shape) sets
    self.shape and its layout structs and returns those two lengths."""
    _KEY = _WHAT = None

    def __init__(self, shape, theta, data, device="cuda:0"):
        _lib.load_library()
        if not torch.cuda.is_available():
            raise _lib.SvgpError(f"{type(self).__name__} needs a HIP device; there is no CPU execution path")
        self.device = torch.device(device)
        n_theta, n_data = self._layouts(shape)
        self.theta = torch.as_tensor(theta, dtype=_F64).reshape(-1).to(self.device).contiguous()
        if self.theta.numel() != n_theta:
            raise ValueError(f"theta has {self.theta.numel()} elements, the shape {self.shape} needs {n_theta}")
        self.data = (torch.zeros(n_data, dtype=_F64, device=self.device) if data is None
                     else torch.as_tensor(data, dtype=_F64).reshape(-1).to(self.device).contiguous())
        if self.data.numel() != n_data:
            raise ValueError(f"cache has {self.data.numel()} elements, the shape {self.shape} needs {n_data}")
        self.stream = torch.cuda.Stream(device=self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def save(self, path):
        """One tensor (the cache), the parameter vector and the shape fields."""
        torch.cuda.synchronize(self.device)
        torch.save({self._KEY: self.data.cpu(), "theta": self.theta.cpu(), "shape": dict(self.shape)}, path)

    @classmethod
    def load(cls, path, device="cuda:0"):
        ck = torch.load(path, map_location="cpu")
        if not isinstance(ck, dict) or any(k not in ck for k in (cls._KEY, "theta", "shape")):
            raise ValueError(f"{path}: not a {cls._WHAT} file")
        return cls(ck["shape"], ck["theta"], ck[cls._KEY], device=device)


class PosteriorCache(_Cache):
    """[acc_S | acc_v | acc_rows | w | X] of svgp_mnist_cache_layout (`data`, one float64 device tensor) with the flat parameter
    vector `theta` it was built for and the shape fields: the whole deployed model."""
    _KEY, _WHAT = "cache", "posterior cache"

    def __init__(self, shape, theta, data, device="cuda:0"):
        super().__init__(shape, theta, data, device)
        n_work = int(self.lib_elems("svgp_mnist_generate_workspace_elems", _cfg(self.shape, GEN_ROWS, GEN_ROWS)))
        self.work = torch.empty(n_work, dtype=_F64, device=self.device) if n_work else None

    def _layouts(self, shape):
        self.shape = {k: (float(shape[k]) if k in ("N_train", "jitter") else int(shape[k])) for k in _SHAPE_KEYS}
        self.cl, self.pl = CacheLayout(), ParamLayout()
        cfg = _cfg(self.shape, 1, GEN_ROWS)
        call("svgp_mnist_cache_layout_get", C.byref(cfg), C.byref(self.cl))
        call("svgp_mnist_param_layout_get", C.byref(cfg), C.byref(self.pl))
        return self.pl.n_total, self.cl.total

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


_CASALE_KEYS = ("N", "n_obj", "Q", "M", "L", "normalize_obj", "ov_joint")


def _casale_cfg(shape):
    return CasaleCfg(N=shape["N"], n_obj=shape["n_obj"], Q=shape["Q"], M=shape["M"], L=shape["L"], b_cap=1,
                     normalize_obj=shape["normalize_obj"], train_gp=0, train_ov=shape["ov_joint"])


class CasalePosteriorCache(_Cache):
    """The Casale GP-VAE after training, without the train set: `data` = [angles | L_W | U | P] of
    svgp_casale_cache_layout (one float64 device tensor), `theta` = [encoder | decoder | l_GP, amplitude, alpha | object_vectors]
    and the shape fields (N, n_obj, Q, M, L, normalize_obj, ov_joint).  P = (alpha I + V^T V)^-1 and U = P V^T Z are all the
    posterior of predict_test_set_Casale keeps of the N train rows.

        cache = CasalePosteriorCache.build(vae, GP, train_images, train_aux)      # or eng.posterior_cache()
        images = generate(cache, aux)                                             # decode of the posterior mean
        images, mean, var = generate(cache, aux, eps=eps, return_moments=True)    # mean (b, L), var (b,)"""
    _KEY, _WHAT = "casale_cache", "Casale posterior cache"
    work = None                          # H > 256: svgp_casale_generate_workspace_elems(cfg, b) doubles, allocated by generate

    def _layouts(self, shape):
        self.shape = {k: int(shape[k]) for k in _CASALE_KEYS}
        self.cfg = _casale_cfg(self.shape)
        self.cl, self.wl = CasaleCacheLayout(), CasaleLayout()
        call("svgp_casale_cache_layout_get", C.byref(self.cfg), C.byref(self.cl))       # refuses Q > 32, H > 2048, M > 128, L > 64
        call("svgp_casale_layout_get", C.byref(self.cfg), C.byref(self.wl))
        return self.wl.n_total, self.cl.total

    def field(self, name):
        """View of a cache field (angles, L_W, U, P)."""
        Q, L = self.shape["Q"], self.shape["L"]
        H = self.shape["M"] * Q
        shp = dict(angles=(Q,), L_W=(Q, Q), U=(H, L), P=(H, H))[name]
        off = getattr(self.cl, name)
        return self.data[off:off + int(np.prod(shp))].view(shp)

    # ------------------------------------------------------------------ build
    @classmethod
    def _from_stage(cls, theta, stage, ov_joint, Z):
        """The cache of a _GpStage (its cfg, index arrays and workspace) at the device parameter vector `theta` and the latent
        rows Z (N, L) on the device."""
        c = stage.cfg
        shape = dict(N=c.N, n_obj=c.n_obj, Q=c.Q, M=c.M, L=c.L, normalize_obj=c.normalize_obj, ov_joint=int(bool(ov_joint)))
        self = cls(shape, theta.detach().clone(), None, device=stage.dev)
        Z = Z.to(stage.dev, _F64).contiguous()
        if tuple(Z.shape) != (c.N, c.L):
            raise ValueError(f"Z must be ({c.N}, {c.L}), got {tuple(Z.shape)}")
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        gp = self.theta[self.wl.n_vae:]
        call("svgp_casale_cache_build", C.byref(c), gp.data_ptr(), stage.angles.data_ptr(), stage.obj_idx.data_ptr(),
             stage.ang_idx.data_ptr(), Z.data_ptr(), stage.ws.data_ptr(), self.data.data_ptr(), self.stream.cuda_stream)
        self.stream.synchronize()
        return self

    @classmethod
    def from_latents(cls, vae, GP, train_aux, Z, device="cuda:0"):
        """From the latent rows Z (N, L) of the sorted train rows train_aux = [global id, object id, angle]; no image is read."""
        from .GPVAE_Casale_model import _GpStage, _need_gpu, _row_index
        from .VAE_utils import VAE_SHAPES
        _need_gpu("CasalePosteriorCache")
        dev = torch.device(device)
        aux = np.asarray(train_aux.detach().cpu() if torch.is_tensor(train_aux) else train_aux, dtype=np.float64)
        if aux.ndim != 2 or aux.shape[1] < 3:
            raise ValueError("train_aux must be rows [global id, object id, angle] (sort_train_data)")
        angles, obj, ang = _row_index(aux[:, 1:])
        stage = _GpStage(GP, aux.shape[0], angles, obj, ang, b_cap=1, L=vae.L, device=dev)
        theta = torch.cat([torch.as_tensor(vae.params[k], dtype=_F64).reshape(-1).to(dev) for k, _ in VAE_SHAPES(vae.L)] +
                          [GP._gp_vector(dev)])
        return cls._from_stage(theta, stage, GP.ov_joint, torch.as_tensor(Z, dtype=_F64))

    @staticmethod
    def _latents(mu, var_raw, clip_qs, latent, eps_full):
        """Z as encode forms it (GPVAE_Casale_model.py:69-93): mu + eps sqrt(var), var clipped to [1e-3, 10]; "mean": mu."""
        if latent == "mean":
            return mu.clone()
        if latent != "sample":
            raise ValueError(f"latent {latent!r}: 'sample' or 'mean'")
        var = torch.clamp(var_raw, 1e-3, 10) if clip_qs else var_raw
        eps = (torch.randn(mu.shape, dtype=_F64, device=mu.device) if eps_full is None
               else torch.as_tensor(eps_full, dtype=_F64).to(mu.device).reshape(mu.shape))
        return mu + eps * torch.sqrt(var)

    @classmethod
    def build(cls, vae, GP, train_images, train_aux, chunk=1024, clip_qs=False, latent="sample", eps_full=None, device="cuda:0"):
        """Encodes the sorted train rows in chunks of `chunk` (ragged last chunk) through an encoder workspace of min(chunk, N)
        rows, forms Z as encode does (latent="mean": Z = qnet_mu) and calls from_latents.  eps_full (N, L): the N(0,1) draws of
        the sample; None: torch.randn.  The latent rows it used stay on the returned object as `.Z` (they are not saved)."""
        from .GPVAE_Casale_model import _need_gpu
        from .VAE_utils import VAE_SHAPES
        from ._lib import WsLayout
        _need_gpu("CasalePosteriorCache")
        dev = torch.device(device)
        N, L = int(train_images.shape[0]), vae.L
        if N < 1 or int(np.shape(train_aux)[0]) != N:
            raise ValueError(f"train_images has {N} rows, train_aux {int(np.shape(train_aux)[0])}")
        chunk = max(1, min(int(chunk), N))
        base = dict(m=1, L=L, M=1, n_obj=0, N_train=float(N), jitter=1e-6, rep_weight=1.0, b_cap=chunk)
        wl = WsLayout()
        call("svgp_mnist_ws_layout_get", C.byref(MnistCfg(b=chunk, b_global=chunk, **base)), C.byref(wl))
        ws = torch.zeros(wl.total, dtype=_F64, device=dev)
        th = torch.cat([torch.as_tensor(vae.params[k], dtype=_F64).reshape(-1).to(dev) for k, _ in VAE_SHAPES(L)]).contiguous()
        img = torch.as_tensor(train_images, dtype=_F64).to(dev).reshape(N, 28, 28, 1).contiguous()
        mu, var_raw = torch.empty(N, L, dtype=_F64, device=dev), torch.empty(N, L, dtype=_F64, device=dev)
        s = torch.cuda.current_stream(dev)
        for lo in range(0, N, chunk):
            n = min(chunk, N - lo)
            call("svgp_mnist_encoder_fwd", C.byref(MnistCfg(b=n, b_global=n, **base)), th.data_ptr(), img[lo:lo + n].data_ptr(),
                 ws.data_ptr(), s.cuda_stream)
            mu[lo:lo + n] = ws[wl.qnet_mu:wl.qnet_mu + n * L].view(n, L)
            var_raw[lo:lo + n] = ws[wl.qnet_var_raw:wl.qnet_var_raw + n * L].view(n, L)
        Z = cls._latents(mu, var_raw, clip_qs, latent, eps_full)
        self = cls.from_latents(vae, GP, train_aux, Z, device=dev)
        self.Z = Z
        return self


def _query(cache, aux, eps, gather, return_moments, var_shape):
    """The checks of a generate call and its device tensors: (b, aux, eps or None, images, first moment (b, L) or None, second
    moment (b,) + var_shape or None)."""
    sh = cache.shape
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
    if eps is not None:
        eps = torch.as_tensor(eps, dtype=_F64)
        if tuple(eps.shape) != (b, sh["L"]):
            raise ValueError(f"eps must be ({b}, {sh['L']}), got {tuple(eps.shape)}")
    dev = cache.device                   # (the checks above need no device)
    out = lambda *shape: torch.empty(*shape, dtype=_F64, device=dev)
    return (b, aux.to(dev).contiguous(), None if eps is None else eps.to(dev).contiguous(), out(b, 28, 28, 1), out(b, sh["L"]) if return_moments else None,
            out(b, *var_shape) if return_moments else None)


def _generate_casale(cache, aux, eps, gather, return_moments):
    gather = bool(cache.shape["ov_joint"]) if gather is None else gather
    b, d_aux, d_eps, images, mean, var = _query(cache, aux, eps, gather, return_moments, ())
    dev = cache.device
    ptr = lambda t: None if t is None else t.data_ptr()
    n_work = int(_lib.load_library().svgp_casale_generate_workspace_elems(C.byref(cache.cfg), b))      # 0 for H <= 256
    if n_work and (cache.work is None or cache.work.numel() < n_work):
        cache.work = torch.empty(n_work, dtype=_F64, device=dev)
    cache.stream.wait_stream(torch.cuda.current_stream(dev))
    call("svgp_casale_generate", C.byref(cache.cfg), b, cache.theta.data_ptr(), cache.data.data_ptr(), d_aux.data_ptr(),
         int(bool(gather)), ptr(d_eps), images.data_ptr(), ptr(mean), ptr(var), ptr(cache.work), cache.stream.cuda_stream)
    cache.stream.synchronize()
    return (images, mean, var) if return_moments else images


def generate(cache, aux, eps=None, gather=None, return_moments=False):
    """Images (b, 28, 28, 1) at the query rows aux (b, 2+M) = [id, angle, o_1..o_M]: decode(p_m + eps sqrt(p_v)); eps (b, L) None:
    decode of the posterior mean.  gather: the object vector of a row is the model's table row `id` (needs a table); False: the
    row's own columns 2:, the way to generate for an object that is not in the table.  return_moments: (images, p_m, p_v).
    Any b works: m <= 64 is ONE launch for the whole batch, beyond that the rows go through calls of GEN_ROWS rows.

    A CasalePosteriorCache: gather defaults to the model's ov_joint (a PosteriorCache: True); the moments are (mean (b, L),
    var (b,)); H = M Q <= 256 is ONE launch for any b, beyond that passes of 256 rows inside the one library call.
    DEVIATION from predict_test_set_Casale: the sample of row i uses row i's own variance for all its channels,
    z[i, l] = mean[i, l] + eps[i, l] sqrt(var[i]).  The reference tiles the T variances of a call as var[(i L + l) mod T]
    (GPVAE_Casale_model.py:194, sic), which is no function of the query row; predict_test_set_Casale keeps that tiling.  With
    eps=None the images are those of predict_test_set_Casale(..., take_mean=True) at the same latent rows."""
    if isinstance(cache, CasalePosteriorCache):
        return _generate_casale(cache, aux, eps, gather, return_moments)
    gather = True if gather is None else gather
    sh, dev = cache.shape, cache.device
    b, d_aux, d_eps, images, p_m, p_v = _query(cache, aux, eps, gather, return_moments, (sh["L"],))
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
    """The kernels of one generate batch, in launch order (svgp_mnist_generate_route; for a CasalePosteriorCache or its shape
    dict svgp_casale_generate_route); needs no device."""
    sh = cache_or_shape.shape if hasattr(cache_or_shape, "shape") and isinstance(cache_or_shape.shape, dict) else cache_or_shape
    buf = C.create_string_buffer(1024)
    if "Q" in sh:
        call("svgp_casale_generate_route", C.byref(_casale_cfg(sh)), buf, len(buf))
    else:
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


def casale_models_from_run(checkpoint_path, train, mnist_data_path=None, device="cuda:0"):
    """(vae, GP, args dict, sorted train dict) of the GPVAE_Casale run that wrote `checkpoint_path`: the shapes and flags from its
    args.json, the parameters from the checkpoint's theta = [encoder | decoder | l_GP, amplitude, alpha | object_vectors], the
    train pickle's dict `train` sorted as the driver sorts it (sort_train_data: aux rows [global id, object id, angle, ...])."""
    import pickle
    from . import checkpoint
    from .GPVAE_Casale_model import casaleGP, sort_train_data
    from .VAE_utils import VAE_SHAPES, mnistVAE
    run_dir = os.path.dirname(os.path.abspath(checkpoint_path))
    with open(os.path.join(run_dir, "args.json")) as f:
        a = json.load(f)
    if a.get("elbo") != "GPVAE_Casale":
        raise ValueError(f"{run_dir}/args.json: --elbo {a.get('elbo')} is not a GPVAE_Casale run")
    ck = checkpoint.load(checkpoint_path)
    L, M = int(a["L"]), int(a["M"])
    # the table as run_experiment_rotated_mnist_Casale builds it (MNIST_experiment.py): the rows of pca_ov_init<dataset><ending>.p
    # with --PCA, else 400 objects per digit; keep the two in step (the checkpoint format carries no shapes)
    n_obj = len(a["dataset"]) * 400
    if a.get("PCA"):
        ending = a["dataset"] + ("" if M == 8 else "_{}".format(M))
        with open((mnist_data_path or a["mnist_data_path"]) + f"pca_ov_init{ending}.p", "rb") as f:
            n_obj = len(pickle.load(f))
    wl = CasaleLayout()
    call("svgp_casale_layout_get", C.byref(CasaleCfg(N=1, n_obj=n_obj, Q=1, M=M, L=L, b_cap=1)), C.byref(wl))
    theta = ck["theta"]
    if theta.numel() != wl.n_total:
        raise ValueError(f"{checkpoint_path}: theta has {theta.numel()} elements, but a GPVAE_Casale model with L={L}, M={M} and "
                         f"{n_obj} object vectors has {wl.n_total}")
    vae = mnistVAE(L=L, seed=int(a.get("seed", 0)), device=device)
    off = 0
    for k, s in VAE_SHAPES(L):
        n = int(np.prod(s, dtype=np.int64))
        vae.params[k] = theta[off:off + n].view(s).clone()
        off += n
    GP = casaleGP(fixed_gp_params=not a.get("GP_joint"), object_vectors_init=theta[wl.th_ov:].view(n_obj, M).numpy().copy(),
                  object_kernel_normalize=bool(a.get("object_kernel_normalize")), ov_joint=bool(a.get("ov_joint")))
    GP.set_values(l_GP=float(theta[wl.th_l_GP]), amplitude=float(theta[wl.th_amplitude]), alpha=float(theta[wl.th_alpha]))
    return vae, GP, a, sort_train_data(dict(train), dataset=a["dataset"])


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
    p.add_argument("--latent", choices=("sample", "mean"), default="sample",
                   help="GPVAE_Casale runs: the latent rows of the train set, a sample as in training or the encoder's means")
    p.add_argument("--latent_seed", type=int, default=None,
                   help="GPVAE_Casale runs: the N(0,1) draws of --latent sample are RandomState(S).randn(N, L)")
    p.add_argument("--out", required=True)
    return p


def _main_casale(args, run_args, data_path):
    import pickle
    ending = run_args["dataset"] + ("" if int(run_args["M"]) == 8 else "_{}".format(int(run_args["M"])))
    train_file = args.train_file or run_args.get("train_file") or (data_path + "train_data" + ending + ".p")
    with open(train_file, "rb") as f:
        train = pickle.load(f)
    vae, GP, a, train = casale_models_from_run(args.checkpoint, train, data_path)
    N, L, M = len(train["images"]), int(a["L"]), int(a["M"])
    eps_full = None if args.latent_seed is None else np.random.RandomState(args.latent_seed).randn(N, L)
    cache = CasalePosteriorCache.build(vae, GP, torch.as_tensor(np.asarray(train["images"], dtype=np.float64)),
                                       np.asarray(train["aux_data"], dtype=np.float64)[:, :3], chunk=args.chunk,
                                       clip_qs=bool(a.get("clip_qs")), latent=args.latent, eps_full=eps_full)
    # --ids: the table rows (a Casale model always has the table); --aux_file: as the model reads its rows (ov_joint)
    rows = rotation_sweep(args.ids, args.n_angles, M) if args.ids is not None else np.load(args.aux_file)
    eps = np.random.RandomState(args.seed).randn(len(rows), L) if args.sample else None
    out = generate(cache, rows, eps=eps, gather=True if args.ids is not None else None)
    np.save(args.out, out.cpu().numpy())
    print(f"{len(rows)} images -> {args.out}   route: {' '.join(route(cache))}")
    return out


def main(argv=None):
    import pickle
    args = build_parser().parse_args(argv)
    if (args.ids is None) == (args.aux_file is None):
        raise SystemExit("give either --ids (with --n_angles) or --aux_file")
    with open(os.path.join(os.path.dirname(os.path.abspath(args.checkpoint)), "args.json")) as f:
        run_args = json.load(f)
    data_path = args.mnist_data_path or run_args["mnist_data_path"]
    if run_args.get("elbo") == "GPVAE_Casale":
        return _main_casale(args, run_args, data_path)
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
