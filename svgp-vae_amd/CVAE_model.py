"""Plain VAE and conditional VAE baselines of rotated MNIST under the reference's names, executed by csrc/cvae.hip.

`mnistCVAE` (VAE_utils.py:165-258), `forward_pass_standard_VAE_rotated_mnist` (SVGPVAE_model.py:718-782) and `predict_CVAE`
(:785-820) live here and not in `VAE_utils` / `SVGPVAE_model`, whose import surface is pinned.  `VaeStepEngine` is the training
runtime: one image launch and one reduction + Adam launch per step (include/svgpvae_hip.h, "plain VAE / conditional VAE").

Tensors are float64, NHWC, TF weight layouts; `aux` rows are [id, angle, ...] and only the first two columns are read.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import STATE, STATE_LEN, CvaeCfg, CvaeWsLayout, ParamLayout, call
from .VAE_utils import VAE_SHAPES, mnistVAE

_F64 = torch.float64

CVAE_SHAPES = lambda L: [
    ("enc_c1_w", (3, 3, 3, 8)), ("enc_c1_b", (8,)), ("enc_c2_w", (3, 3, 8, 8)), ("enc_c2_b", (8,)),
    ("enc_c3_w", (3, 3, 8, 8)), ("enc_c3_b", (8,)), ("enc_d_w", (34, 2 * L)), ("enc_d_b", (2 * L,)),
    ("dec_d_w", (L + 2, 128)), ("dec_d_b", (128,)), ("dec_c1_w", (3, 3, 10, 8)), ("dec_c1_b", (8,)),
    ("dec_c2_w", (3, 3, 8, 8)), ("dec_c2_b", (8,)), ("dec_c3_w", (3, 3, 8, 1)), ("dec_c3_b", (1,))]


def param_shapes(L, cvae):
    return CVAE_SHAPES(L) if cvae else VAE_SHAPES(L)


def glorot_uniform_params(L=16, seed=0, cvae=True):
    """VAE_utils.glorot_uniform_params for either variant's shapes (Keras: glorot_uniform kernels, zero biases)."""
    rng = np.random.RandomState(seed)
    out = {}
    for name, shp in param_shapes(L, cvae):
        if name.endswith("_b"):
            out[name] = np.zeros(shp)
            continue
        rf = shp[0] * shp[1] if len(shp) == 4 else 1
        fan_in, fan_out = (rf * shp[2], rf * shp[3]) if len(shp) == 4 else shp
        lim = math.sqrt(6.0 / (fan_in + fan_out))
        out[name] = rng.uniform(-lim, lim, size=shp)
    return out


def _need_gpu(what):
    if not torch.cuda.is_available():
        raise _lib.SvgpError(f"{what} runs HIP kernels and needs a GPU; there is no CPU fallback")


def _aux2(aux, dev):
    """(b, 2) contiguous [id, angle] rows on the device."""
    a = torch.as_tensor(aux, dtype=_F64)
    return a[:, :2].to(dev).contiguous()


def _flat(vae, dev):
    cvae = isinstance(vae, mnistCVAE)
    return torch.cat([torch.as_tensor(vae.params[k], dtype=_F64).reshape(-1) for k, _ in param_shapes(vae.L, cvae)]).to(dev)


def _theta_of(vae, dev):
    """The live flat parameter vector: the bound engine's, else one packed from vae.params."""
    eng = getattr(vae, "_vae_engine", None)
    if eng is None:
        return _flat(vae, dev)
    eng.stream.synchronize()         # the engine's steps run on its own stream
    return eng.theta


def _cfg(vae, b, *, clip=False, store=1, sigma=0.01, b_cap=None):
    return CvaeCfg(b=b, b_cap=b if b_cap is None else b_cap, L=vae.L, cvae=int(isinstance(vae, mnistCVAE)), clip_qs=int(bool(clip)),
                   store=store, sigma=float(sigma))


class mnistCVAE:
    """VAE_utils.py:165-258: the angle enters as two constant input planes, two extra encoder features, two extra latent
    coordinates and two constant planes in front of the first up-convolution."""
    dtype = torch.float64

    def __init__(self, im_width=28, im_height=28, L=16, seed=0, device="cuda:0"):
        if (im_width, im_height) != (28, 28):
            raise NotImplementedError("the HIP encoder/decoder are specialised to 28x28x1 rotated-MNIST images")
        self.L = L
        self.device = device
        self.params = {k: torch.tensor(v, dtype=self.dtype) for k, v in glorot_uniform_params(L, seed, cvae=True).items()}
        self._vae_engine = None

    def encode(self, images, angles):
        """images (b,28,28,1) -- or the reference's (b,28,28,3) with the two angle planes, of which channel 0 is read --,
        angles (b,) -> (means, vars)."""
        _need_gpu("mnistCVAE.encode")
        dev = torch.device(self.device)
        img = torch.as_tensor(images, dtype=_F64)[..., :1].to(dev).contiguous()
        b = img.shape[0]
        aux = torch.stack([torch.zeros(b, dtype=_F64, device=dev), torch.as_tensor(angles, dtype=_F64).to(dev).reshape(b)], 1).contiguous()
        mu, var = torch.empty(b, self.L, dtype=_F64, device=dev), torch.empty(b, self.L, dtype=_F64, device=dev)
        theta = _theta_of(self, dev)
        call("svgp_cvae_encode", C.byref(_cfg(self, b)), theta.data_ptr(), img.data_ptr(), aux.data_ptr(), mu.data_ptr(), var.data_ptr(),
             torch.cuda.current_stream(dev).cuda_stream)
        return mu, var

    def decode(self, latent_samples, angles):
        _need_gpu("mnistCVAE.decode")
        dev = torch.device(self.device)
        z = torch.as_tensor(latent_samples, dtype=_F64).to(dev).contiguous()
        b = z.shape[0]
        aux = torch.stack([torch.zeros(b, dtype=_F64, device=dev), torch.as_tensor(angles, dtype=_F64).to(dev).reshape(b)], 1).contiguous()
        out = torch.empty(b, 28, 28, 1, dtype=_F64, device=dev)
        theta = _theta_of(self, dev)
        call("svgp_cvae_decode", C.byref(_cfg(self, b)), theta.data_ptr(), z.data_ptr(), aux.data_ptr(), out.data_ptr(),
             torch.cuda.current_stream(dev).cuda_stream)
        return out


def _ws_for(cfg, dev):
    wl = CvaeWsLayout()
    call("svgp_cvae_ws_layout_get", C.byref(cfg), C.byref(wl))
    return wl, torch.zeros(wl.total, dtype=_F64, device=dev)


def forward_pass_standard_VAE_rotated_mnist(data_batch, vae, sigma_gaussian_decoder=0.01, clipping_qs=False, CVAE=False, epsilon=None):
    """SVGPVAE_model.py:718-782.  Returns (recon_loss, KL_term, elbo, recon_images, qnet_mu, qnet_var, latent_samples);
    epsilon (b, L) replaces the N(0,1) draw."""
    _need_gpu("forward_pass_standard_VAE_rotated_mnist")
    if bool(CVAE) != isinstance(vae, mnistCVAE):
        raise ValueError("CVAE=True needs an mnistCVAE, CVAE=False an mnistVAE")
    images, aux = data_batch
    dev = torch.device(vae.device)
    img = torch.as_tensor(images, dtype=_F64).to(dev).contiguous()
    b, L = img.shape[0], vae.L
    aux2 = _aux2(aux, dev)
    cfg = _cfg(vae, b, clip=clipping_qs, sigma=sigma_gaussian_decoder)
    wl, ws = _ws_for(cfg, dev)
    state = torch.zeros(STATE_LEN, dtype=_F64, device=dev)
    eps = None if epsilon is None else torch.as_tensor(epsilon, dtype=_F64).to(dev).contiguous()
    if eps is None:
        state[STATE["RNG_CTR"]] = float(torch.randint(0, 2 ** 52, (1,)).item())
    theta = _theta_of(vae, dev)
    call("svgp_cvae_forward", C.byref(cfg), theta.data_ptr(), img.data_ptr(), aux2.data_ptr(), None if eps is None else eps.data_ptr(),
         ws.data_ptr(), state.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    take = lambda name, shape: ws[getattr(wl, name):getattr(wl, name) + int(np.prod(shape))].view(shape)
    return (state[STATE["RECON_LOSS"]], state[STATE["KL_TERM"]], state[STATE["ELBO"]], take("recon", (b, 28, 28, 1)),
            take("qnet_mu", (b, L)), take("qnet_var", (b, L)), take("z", (b, L)))


def predict_CVAE(images_train, images_test, aux_data_train, aux_data_test, vae, test_indices=None, epsilon=None):
    """SVGPVAE_model.py:785-820: (recon_images_test, recon_loss).  test_indices, the reference's loop range, defaults to
    aux_data_test[:, 0]; given, it replaces that column.  A test id without a train row gives a NaN image."""
    _need_gpu("predict_CVAE")
    if not isinstance(vae, mnistCVAE):
        raise ValueError("predict_CVAE needs an mnistCVAE")
    dev = torch.device(vae.device)
    tr = torch.as_tensor(images_train, dtype=_F64)[..., :1].to(dev).contiguous()
    te = torch.as_tensor(images_test, dtype=_F64).to(dev).contiguous()
    atr, ate = _aux2(aux_data_train, dev), _aux2(aux_data_test, dev).clone()
    if test_indices is not None:
        ate[:, 0] = torch.as_tensor(np.asarray(test_indices, dtype=np.float64)).to(dev)
    N, T = tr.shape[0], te.shape[0]
    cfg = _cfg(vae, T)
    work = torch.zeros(int(_lib.load_library().svgp_cvae_predict_workspace_elems(C.byref(cfg), N)), dtype=_F64, device=dev)
    state = torch.zeros(STATE_LEN, dtype=_F64, device=dev)
    eps = None if epsilon is None else torch.as_tensor(epsilon, dtype=_F64).to(dev).contiguous()
    if eps is None:
        state[STATE["RNG_CTR"]] = float(torch.randint(0, 2 ** 52, (1,)).item())
    recon, loss = torch.empty(T, 28, 28, 1, dtype=_F64, device=dev), torch.zeros(1, dtype=_F64, device=dev)
    theta = _theta_of(vae, dev)
    call("svgp_cvae_predict", C.byref(cfg), N, theta.data_ptr(), tr.data_ptr(), atr.data_ptr(), None if eps is None else eps.data_ptr(),
         te.data_ptr(), ate.data_ptr(), work.data_ptr(), recon.data_ptr(), loss.data_ptr(), state.data_ptr(),
         torch.cuda.current_stream(dev).cuda_stream)
    return recon, loss[0]


class VaeStepEngine:
    """Owns theta, grad, the Adam moments, state and ws of the VAE / CVAE step; serves mnistVAE (cvae = 0) and mnistCVAE objects.
    step(images, aux, eps=None, adam=True) issues svgp_cvae_train_step: two launches (route())."""

    def __init__(self, vae, *, b_max, lr, clip_qs=False, sigma=0.01, device="cuda:0", store=True):
        _need_gpu("VaeStepEngine")
        if not isinstance(vae, (mnistVAE, mnistCVAE)):
            raise TypeError("VaeStepEngine serves mnistVAE and mnistCVAE objects")
        self.lib = _lib.load_library()
        self.dev = self.device = torch.device(device)
        self.vae, self.L, self.cvae = vae, vae.L, int(isinstance(vae, mnistCVAE))
        self.b_max, self.clip, self.sigma, self.store = int(b_max), int(bool(clip_qs)), float(sigma), int(bool(store))
        self.pl, self.wl = ParamLayout(), CvaeWsLayout()
        call("svgp_cvae_param_layout_get", C.byref(self._cfg(0)), C.byref(self.pl))
        call("svgp_cvae_ws_layout_get", C.byref(self._cfg(0)), C.byref(self.wl))
        self.n_total = int(self.pl.n_total)
        f64 = dict(dtype=_F64, device=self.dev)
        self.theta, self.grad = torch.zeros(self.n_total, **f64), torch.zeros(self.n_total, **f64)
        self.adam_m, self.adam_v = torch.zeros(self.n_total, **f64), torch.zeros(self.n_total, **f64)
        self.state, self.ws = torch.zeros(STATE_LEN, **f64), torch.zeros(int(self.wl.total), **f64)
        self.shapes, self.params, self._gviews = {}, {}, {}
        for k, s in param_shapes(self.L, self.cvae):
            off, n = int(getattr(self.pl, k)), int(np.prod(s))
            self.shapes[k], self.params[k], self._gviews[k] = s, self.theta[off:off + n].view(s), self.grad[off:off + n].view(s)
        self.stream = torch.cuda.Stream(device=self.dev)
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))
        self.load_params(vae.params)
        self.state[STATE["LR"]] = float(lr)
        self._b = 0
        vae._vae_engine = self
        self.stream.synchronize()

    def _cfg(self, b):
        return CvaeCfg(b=b, b_cap=self.b_max, L=self.L, cvae=self.cvae, clip_qs=self.clip, store=self.store, sigma=self.sigma)

    def load_params(self, params):
        with torch.cuda.stream(self.stream):
            for k, v in params.items():
                self.params[k].copy_(torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v, dtype=_F64).reshape(self.shapes[k]))
        self.stream.synchronize()

    def set_rng_counter(self, value):
        self.state[STATE["RNG_CTR"]] = float(value)

    def route(self, b=None):
        buf = C.create_string_buffer(256)
        call("svgp_cvae_step_route", C.byref(self._cfg(self.b_max if b is None else b)), buf, 256)
        return buf.value.decode().split()

    def _bind(self, images, aux, eps):
        img = torch.as_tensor(images, dtype=_F64).to(self.dev).contiguous()
        b = img.shape[0]
        if b > self.b_max:
            raise _lib.SvgpError(f"{b} rows in a workspace sized for b_max = {self.b_max}")
        aux2 = _aux2(aux, self.dev) if (aux is not None) else None
        if self.cvae and aux2 is None:
            raise ValueError("mnistCVAE needs aux rows [id, angle]")
        e = None if eps is None else torch.as_tensor(eps, dtype=_F64).to(self.dev).contiguous()
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))
        self._keep = (img, aux2, e)          # alive until the stream has run
        self._b = b
        ptr = lambda t: None if t is None else t.data_ptr()
        return b, ptr(img), ptr(aux2), ptr(e)

    def step(self, images, aux, eps=None, adam=True):
        b, img, aux2, e = self._bind(images, aux, eps)
        call("svgp_cvae_train_step", C.byref(self._cfg(b)), self.theta.data_ptr(), img, aux2, e, self.ws.data_ptr(), self.grad.data_ptr(),
             self.adam_m.data_ptr(), self.adam_v.data_ptr(), self.state.data_ptr(), int(bool(adam)), self.stream.cuda_stream)
        return self

    def forward(self, images, aux, eps=None):
        b, img, aux2, e = self._bind(images, aux, eps)
        call("svgp_cvae_forward", C.byref(self._cfg(b)), self.theta.data_ptr(), img, aux2, e, self.ws.data_ptr(), self.state.data_ptr(),
             self.stream.cuda_stream)
        return self

    def synchronize(self):
        self.stream.synchronize()

    def scalars(self):
        self.stream.synchronize()
        st = self.state.cpu()
        return dict(elbo=float(st[STATE["ELBO"]]), recon_loss=float(st[STATE["RECON_LOSS"]]), KL_term=float(st[STATE["KL_TERM"]]),
                    adam_t=float(st[STATE["ADAM_T"]]), lr=float(st[STATE["LR"]]), rng_ctr=float(st[STATE["RNG_CTR"]]))

    def grads(self):
        self.stream.synchronize()
        return {k: v.clone() for k, v in self._gviews.items()}

    def ws_view(self, name):
        """recon / qnet_mu / qnet_var / z of the last call (stored fields)."""
        self.stream.synchronize()
        shape = (self._b, 28, 28, 1) if name == "recon" else (self._b, self.L)
        off = int(getattr(self.wl, name))
        return self.ws[off:off + int(np.prod(shape))].view(shape)
