"""Casale GP-VAE baseline on rotated MNIST, executed by the HIP library (csrc/casale.hip).

Reference call surface mirrored here (eager float64 CUDA tensors instead of TF graph tensors; GPVAE_Casale_model.py):
  tf_kron(a, b)                                                                    :10-21
  train_angles_mask(data_path, save_path)                                          :24-40
  sort_train_data(train_data_dict, dataset='3')                                    :43-66
  encode(train_images, vae, clipping_qs=False, batch=False)                        :69-93
  forward_pass_Casale(data_batch, vae, a, B, c, V, beta, GP, clipping_qs=False)    :96-155
  predict_test_set_Casale(test_images, test_aux_data, train_aux_data, vae, GP, V, latent_samples_train, take_mean=False)
                                                                                   :158-203
  casaleGP(fixed_gp_params, object_vectors_init, object_kernel_normalize, ov_joint, jitter=1e-6) with kernel_matrix,
  V_matrix, taylor_coeff, variable_summary                                         :206-359
Functions that draw N(0,1) numbers take a trailing `epsilon=None` keyword.

The reference's N x N matrix K_inv = (I - V (alpha I + V^T V)^-1 V^T) / alpha never exists here: everything runs in
H x H space (H = M Q; include/svgpvae_hip.h has the restatement).  The functions above are the values-only API; the training
step -- `sess.run` of MNIST_experiment.py:891-906, 987-1011 with its three regimes -- is `CasaleStepEngine.step`.
Every product is a library GEMM; torch supplies memory, streams and element-wise glue only.
"""
import ctypes as C
import pickle

import numpy as np
import torch

from . import _lib
from ._lib import STATE, STATE_LEN, CasaleCfg, CasaleLayout, MnistCfg, WsLayout, call

_F64 = torch.float64
REGIMES = ("joint", "GP", "VAE")
REGIME_LR = dict(joint=0.001, GP=0.01, VAE=0.001)          # MNIST_experiment.py:891-906
_SIGMA_VAE = 0.01                                           # sigma_gaussian_decoder of the VAE regime (:876)


# ------------------------------------------------------------------------------------------------------ library glue
def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _gemm(A, B, ta=0, tb=0, alpha=1.0):
    """op(A) op(B) of two row-major 2-d float64 CUDA tensors through svgp_dgemm_batched."""
    A, B = A.contiguous(), B.contiguous()
    M, K = (A.shape[1], A.shape[0]) if ta else A.shape
    N = B.shape[0] if tb else B.shape[1]
    assert (B.shape[1] if tb else B.shape[0]) == K
    out = torch.empty(M, N, dtype=_F64, device=A.device)
    call("svgp_dgemm_batched", ta, tb, M, N, K, alpha, A.data_ptr(), A.shape[1], 0, B.data_ptr(), B.shape[1], 0, 0.0,
         out.data_ptr(), N, 0, 1, _stream(A.device))
    return out


def _gemm_tall(A, B):
    """A^T B with a long contraction (the N train rows): svgp_dgemm_splitk."""
    A, B = A.contiguous(), B.contiguous()
    K, M = A.shape
    N = B.shape[1]
    lib = _lib.load_library()
    n_scr = int(lib.svgp_dgemm_splitk_scratch_elems(M, N, K))
    scr = torch.empty(max(n_scr, 1), dtype=_F64, device=A.device)
    out = torch.empty(M, N, dtype=_F64, device=A.device)
    call("svgp_dgemm_splitk", 1, 0, M, N, K, 1.0, A.data_ptr(), M, B.data_ptr(), N, 0.0, out.data_ptr(), N,
         scr.data_ptr(), n_scr, _stream(A.device))
    return out


def _spd_inverse(X):
    H = X.shape[0]
    lib = _lib.load_library()
    X = X.clone().contiguous()
    work = torch.empty(int(lib.svgp_spd_inverse_workspace_elems(H, 1)), dtype=_F64, device=X.device)
    logdet = torch.empty(1, dtype=_F64, device=X.device)
    call("svgp_spd_inverse_batched", H, 1, X.data_ptr(), logdet.data_ptr(), work.data_ptr(), _stream(X.device))
    return X


def _hspace(V, Z, alpha):
    """P = (alpha I + V^T V)^-1, U = P V^T Z, A = K_inv Z = (Z - V U) / alpha."""
    H = V.shape[1]
    G = _gemm_tall(V, V)
    P = _spd_inverse(G + alpha * torch.eye(H, dtype=_F64, device=V.device))
    U = _gemm(P, _gemm_tall(V, Z))
    A = (Z - _gemm(V, U)) / alpha
    return P, U, A


def _need_gpu(what):
    _lib.load_library()
    if not torch.cuda.is_available():
        raise _lib.SvgpError(f"{what} needs a HIP device (torch.cuda.is_available() is False); there is no CPU execution path")


def _normal(shape, dev, epsilon):
    if epsilon is None:
        return torch.randn(shape, dtype=_F64, device=dev)
    return torch.as_tensor(epsilon, dtype=_F64).to(dev).reshape(shape)


# ------------------------------------------------------------------------------------------------------ host helpers
def tf_kron(a, b):
    """Kronecker product of two matrices (:10-21); element-wise products only."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return (a.reshape(a.shape[0], 1, a.shape[1], 1) * b.reshape(1, b.shape[0], 1, b.shape[1])).reshape(
        a.shape[0] * b.shape[0], a.shape[1] * b.shape[1])


def _angles_mask(aux_data):
    """The mask of train_angles_mask from aux rows [object id, angle, ...]: for every object (sorted ids) and every unique
    train angle (sorted), whether the pair is in the data."""
    aux_data = np.asarray(aux_data)
    ids, angles = np.sort(np.unique(aux_data[:, 0])), np.sort(np.unique(aux_data[:, 1]))
    train_angles = [np.sort(aux_data[np.where(aux_data[:, 0] == x)][:, 1]) for x in ids]
    return np.array([x in y for y in train_angles for x in angles])


def train_angles_mask(data_path, save_path):
    """Mask for subsampling the rows of kron(object_vectors, L_W) to the (object, angle) pairs of the train data (:24-40)."""
    train_data = pickle.load(open(data_path, "rb"))
    pickle.dump(_angles_mask(train_data["aux_data"]), open(save_path, "wb"))


def sort_train_data(train_data_dict, dataset="3"):
    """Sorts the train data by (object id, angle) and puts a global id column in front of aux_data (:43-66).  The id column
    is range(N), which is the reference's range(4050 * len(dataset)) at its data."""
    images, aux_data = train_data_dict["images"], train_data_dict["aux_data"]
    N = len(aux_data)
    sorted_idx = sorted(list(zip(aux_data[:, 0], aux_data[:, 1], range(N))), key=lambda x: (x[0], x[1]))
    sorted_idx = [x[2] for x in sorted_idx]
    aux_data = aux_data[sorted_idx]
    train_data_dict["aux_data"] = np.hstack((np.expand_dims(np.array(range(N)), axis=1), aux_data))
    train_data_dict["images"] = images[sorted_idx]
    return train_data_dict


def _row_index(aux_rows):
    """(angles (Q), obj_idx (N) int32, ang_idx (N) int32) of sorted train rows [object id, angle, ...]."""
    aux_rows = np.asarray(aux_rows, dtype=np.float64)
    angles = np.sort(np.unique(aux_rows[:, 1]))
    obj = aux_rows[:, 0].astype(np.int32)
    if np.any(np.diff(obj) < 0):
        raise ValueError("train rows must be sorted by object id (sort_train_data)")
    return angles, obj, np.searchsorted(angles, aux_rows[:, 1]).astype(np.int32)


# ------------------------------------------------------------------------------------------------------ values-only API
def encode(train_images, vae, clipping_qs=False, batch=False, epsilon=None):
    """Latent sample of the whole train set (:69-93)."""
    qnet_mu, qnet_var = vae.encode(train_images[0] if batch else train_images)
    if clipping_qs:
        qnet_var = torch.clamp(qnet_var, 1e-3, 10)
    return qnet_mu + _normal(qnet_mu.shape, qnet_mu.device, epsilon) * torch.sqrt(qnet_var)


def forward_pass_Casale(data_batch, vae, a, B, c, V, beta, GP, clipping_qs=False, epsilon=None):
    """The reference's 7-tuple from materialised Taylor coefficients (:96-155); values only."""
    images, aux_data = data_batch
    qnet_mu, qnet_var = vae.encode(images)
    dev = qnet_mu.device
    batch_idx = torch.as_tensor(aux_data)[:, 0].to(dev).long()
    L = qnet_mu.shape[1]
    if clipping_qs:
        qnet_var = torch.clamp(qnet_var, 1e-3, 100)
    log_var = torch.sum(torch.log(qnet_var))
    latent_samples = qnet_mu + _normal(qnet_mu.shape, dev, epsilon) * torch.sqrt(qnet_var)
    a_batch, B_batch, V_batch = a.t()[batch_idx], B.permute(1, 2, 0)[batch_idx], V[batch_idx]
    B_terms = sum(torch.sum(B_batch[:, :, l] * V_batch) for l in range(L))
    GP_prior_term = torch.sum(latent_samples * a_batch) + B_terms + torch.sum(c) * GP.alpha
    recon_images = vae.decode(latent_samples)
    recon_loss = torch.sum((images.to(dev, _F64) - recon_images) ** 2)
    elbo = recon_loss / 784.0 - (beta / L) * (GP_prior_term + 0.5 * log_var)
    return elbo, recon_loss / 784.0, GP_prior_term, log_var, qnet_mu, qnet_var, recon_images


def predict_test_set_Casale(test_images, test_aux_data, train_aux_data, vae, GP, V, latent_samples_train, take_mean=False,
                            epsilon=None):
    """Conditional generation on the test set (:158-203): mean = K_*n K_inv Z; var_i = k_ii - k_i^T K_inv k_i.  With
    take_mean=False the draw of row i, channel l is scaled by sqrt(var[(i L + l) mod T]): the reference tiles the T
    variances L times and reshapes the T L numbers to (T, L) (:194, sic), which is reproduced here."""
    dev = V.device
    test_aux_data = torch.as_tensor(test_aux_data, dtype=_F64).to(dev)
    train_rows = torch.as_tensor(train_aux_data, dtype=_F64).to(dev)[:, 1:]
    K_test_train = GP.kernel_matrix(test_aux_data, train_rows)
    P, _, A = _hspace(V, latent_samples_train.to(dev, _F64), GP.alpha)
    mean = _gemm(K_test_train, A)
    if take_mean:
        latent_samples_test = mean
    else:
        T, N = K_test_train.shape
        k_tt = GP.kernel_matrix(test_aux_data, test_aux_data, diag_only=True)
        R = _gemm(K_test_train, V)
        RP = _gemm(R, P)
        var = torch.empty(T, dtype=_F64, device=dev)
        alpha = torch.tensor([GP.alpha], dtype=_F64, device=dev)
        call("svgp_casale_predict_var", T, N, V.shape[1], K_test_train.data_ptr(), k_tt.data_ptr(), R.data_ptr(),
             RP.data_ptr(), alpha.data_ptr(), var.data_ptr(), _stream(dev))
        var = var.repeat(mean.shape[1]).reshape(-1, mean.shape[1])                # :194 (sic): not one variance per row
        latent_samples_test = mean + _normal(mean.shape, dev, epsilon) * torch.sqrt(var)
    recon_images_test = vae.decode(latent_samples_test)
    recon_loss = torch.mean((test_images.to(dev, _F64) - recon_images_test) ** 2)
    return recon_images_test, recon_loss


class casaleGP:
    """GP of Casale's GP-VAE on rotated MNIST (:206-359).  Holds the values of l_GP, amplitude, alpha and the object
    vectors; while a CasaleStepEngine is attached they are read from its parameter vector."""
    dtype = np.float64

    def __init__(self, fixed_gp_params, object_vectors_init, object_kernel_normalize, ov_joint, jitter=1e-6):
        self.jitter = jitter
        self.object_kernel_normalize = bool(object_kernel_normalize)
        self.ov_joint = bool(ov_joint)
        self.fixed_gp_params = bool(fixed_gp_params)
        self._l_GP, self._amplitude, self._alpha = 1.0, 1.0, 0.1            # :227-233
        self._object_vectors = np.array(object_vectors_init, dtype=np.float64)
        self._engine = None

    def _value(self, name):
        e = self._engine
        if e is None:
            return getattr(self, "_" + name)
        e.stream.synchronize()
        v = e.params[name]
        return float(v) if v.numel() == 1 and name != "object_vectors" else v.detach().cpu().numpy().copy()

    l_GP = property(lambda self: self._value("l_GP"))
    amplitude = property(lambda self: self._value("amplitude"))
    alpha = property(lambda self: self._value("alpha"))
    object_vectors = property(lambda self: self._value("object_vectors"))

    def set_values(self, l_GP=None, amplitude=None, alpha=None, object_vectors=None):
        if self._engine is not None:
            raise RuntimeError("a CasaleStepEngine owns the parameters; use its load_params")
        for k, v in dict(l_GP=l_GP, amplitude=amplitude, alpha=alpha).items():
            if v is not None:
                setattr(self, "_" + k, float(v))
        if object_vectors is not None:
            self._object_vectors = np.array(object_vectors, dtype=np.float64)

    def _gp_vector(self, dev):
        """[l_GP, amplitude, alpha, object_vectors]: the parameter suffix the library reads."""
        ov = np.asarray(self.object_vectors, dtype=np.float64)
        return torch.tensor(np.concatenate(([self.l_GP, self.amplitude, self.alpha], ov.ravel())), dtype=_F64, device=dev)

    def kernel_matrix(self, x, y, diag_only=False):
        """Product kernel ExpSinSquared(angle) * Linear(object vector) (:249-276) through svgp_kernel_matrix_xy.  Rows are
        [id, angle, o_1..o_M]; with ov_joint the object vector is object_vectors[id]."""
        _need_gpu("casaleGP.kernel_matrix")
        x = torch.as_tensor(x, dtype=_F64)
        dev = x.device if x.is_cuda else torch.device("cuda:0")
        x, y = x.to(dev).contiguous(), torch.as_tensor(y, dtype=_F64).to(dev).contiguous()
        gp = self._gp_vector(dev)
        M = self._object_vectors.shape[1]
        if not self.ov_joint and (x.shape[1] != 2 + M or y.shape[1] != 2 + M):
            raise ValueError("without ov_joint the rows carry their object vectors: [id, angle, o_1..o_M]")
        g = int(self.ov_joint)
        if g:       # only columns 0, 1 are read; the library's row stride is 2 + M
            pad = lambda r: torch.cat([r[:, :2], torch.zeros(r.shape[0], M, dtype=_F64, device=dev)], 1).contiguous()
            x, y = pad(x), pad(y)
        nx, ny = x.shape[0], y.shape[0]
        out = torch.empty(nx if diag_only else (nx, ny), dtype=_F64, device=dev)
        call("svgp_kernel_matrix_xy", M, int(self.object_kernel_normalize), nx, x.data_ptr(), g, ny, y.data_ptr(), g,
             gp[3:].data_ptr(), gp[0:].data_ptr(), gp[1:].data_ptr(), int(diag_only), out.data_ptr(), _stream(dev))
        return out

    def V_matrix(self, aux_data_train, train_ids_mask):
        """V (N x H), H = M Q (:278-309): the rows of kron(object vectors, chol(K_W)) that train_ids_mask selects, built
        row-wise as V[i, k Q + r] = ov[p_i, k] L_W[q_i, r]."""
        _need_gpu("casaleGP.V_matrix")
        aux = np.asarray(aux_data_train.detach().cpu() if torch.is_tensor(aux_data_train) else aux_data_train, dtype=np.float64)[:, 1:]
        ids, angles = np.sort(np.unique(aux[:, 0])), np.sort(np.unique(aux[:, 1]))
        mask = np.asarray(train_ids_mask, dtype=bool).reshape(len(ids), len(angles))
        jj, rr = np.nonzero(mask)
        dev = torch.device("cuda:0")
        stage = _GpStage(self, len(jj), angles, ids[jj].astype(np.int32), rr.astype(np.int32), b_cap=1, L=1, device=dev)
        stage.build_V(self._gp_vector(dev))
        torch.cuda.current_stream(dev).synchronize()
        return stage.view("V", (stage.N, stage.H)).clone()

    def taylor_coeff(self, Z, V):
        """a (L,N), B (L,N,H), c (L) of the first-order Taylor expansion (:311-351), materialised from the H x H form:
        a = A^T, B_l = V P - A_l U_l^T, c_l = (-|A_l|^2 + tr K_inv) / 2."""
        _need_gpu("casaleGP.taylor_coeff")
        N, H = V.shape
        alpha = self.alpha
        P, U, A = _hspace(V, Z.to(V.device, _F64), alpha)
        VP = _gemm(V, P)
        a = A.t().contiguous()
        B = VP[None, :, :] - a[:, :, None] * U.t()[:, None, :]
        tr_Kinv = (N - H) / alpha + torch.sum(torch.diagonal(P))
        c = 0.5 * (-torch.sum(a * a, dim=1) + tr_Kinv)
        return a, B, c

    def variable_summary(self):
        return self.l_GP, self.amplitude, self.object_vectors, self.alpha


class _GpStage:
    """Configuration, index arrays and workspace of the library's GP stage for one sorted train set."""

    def __init__(self, GP, N, angles, obj_idx, ang_idx, *, b_cap, L, device, train_gp=None, train_ov=None):
        ov = GP._object_vectors
        self.N, self.Q, self.M, self.L = int(N), len(angles), ov.shape[1], int(L)
        self.H = self.M * self.Q
        if len(obj_idx) and (obj_idx.min() < 0 or obj_idx.max() >= ov.shape[0]):
            raise ValueError("object id outside the object_vectors table")
        self.cfg = CasaleCfg(N=self.N, n_obj=ov.shape[0], Q=self.Q, M=self.M, L=self.L, b_cap=int(b_cap),
                             normalize_obj=int(GP.object_kernel_normalize),
                             train_gp=int(not GP.fixed_gp_params if train_gp is None else train_gp),
                             train_ov=int(GP.ov_joint if train_ov is None else train_ov))
        self.wl = CasaleLayout()
        call("svgp_casale_layout_get", C.byref(self.cfg), C.byref(self.wl))       # refuses Q > 32, H > 2048, M > 128, L > 64
        self.dev = device
        self.ws = torch.zeros(self.wl.total, dtype=_F64, device=device)
        self.angles = torch.tensor(np.asarray(angles, dtype=np.float64), device=device)
        self.obj_idx = torch.tensor(np.asarray(obj_idx, dtype=np.int32), device=device)
        self.ang_idx = torch.tensor(np.asarray(ang_idx, dtype=np.int32), device=device)

    def view(self, name, shape):
        off = getattr(self.wl, name)
        return self.ws[off:off + int(np.prod(shape, dtype=np.int64))].view(shape)

    def ptr(self, name):
        return self.ws[getattr(self.wl, name):].data_ptr()

    def _idx(self):
        return self.angles.data_ptr(), self.obj_idx.data_ptr(), self.ang_idx.data_ptr()

    def build_V(self, gp, stream=None):
        call("svgp_casale_v_fwd", C.byref(self.cfg), gp.data_ptr(), *self._idx(), self.ws.data_ptr(),
             _stream(self.dev) if stream is None else stream)

    def fwd(self, gp, Z, zb, lo, hi, stream):
        call("svgp_casale_gp_fwd", C.byref(self.cfg), gp.data_ptr(), *self._idx(), Z, zb, lo, hi, self.ws.data_ptr(), stream)

    def bwd(self, gp, Z, zb, lo, hi, seed, stream):
        call("svgp_casale_gp_bwd", C.byref(self.cfg), gp.data_ptr(), *self._idx(), Z, zb, lo, hi, float(seed),
             self.ws.data_ptr(), stream)

    SHAPES = dict(K_W="QQ", L_W="QQ", V="NH", G="HH", P="HH", W="HL", U="HL", VU="NL", A="NL", VPb="bH", Z="NL", zb="bL",
                  qvar_b="bL", Abar="NL", Cm="NL", Zbar="NL", zbbar="bL", Vbar="NH", Ubar="HL", Pbar="HH", Wbar="HL", T="HH",
                  Mbar="HH", LWbar="QQ", KWbar="QQ", part_alpha="N", trM="1", terms="8")

    def named(self, name, b):
        dims = dict(N=self.N, H=self.H, L=self.L, Q=self.Q, b=b)
        code = self.SHAPES[name]
        shape = (int(code),) if code.isdigit() else tuple(dims[ch] for ch in code)
        return self.view(name, shape)


def casale_gp_stage(GP, aux_rows, Z, zb, lo, hi, seed=1.0, backward=True):
    """The GP prior stage on its own: aux_rows (N, >= 2) sorted rows [object id, angle, ...], Z (N,L), zb (hi-lo,L).
    Returns the _GpStage whose workspace holds every intermediate (stage.named(name, b)); with backward, also the
    reverse pass of seed * GP_prior_term."""
    _need_gpu("casale_gp_stage")
    dev = torch.device("cuda:0")
    angles, obj, ang = _row_index(aux_rows)
    Z, zb = Z.to(dev, _F64).contiguous(), zb.to(dev, _F64).contiguous()
    stage = _GpStage(GP, len(obj), angles, obj, ang, b_cap=hi - lo if 0 <= lo < hi <= len(obj) else 1, L=Z.shape[1], device=dev)
    gp = GP._gp_vector(dev)
    s = _stream(dev)
    stage.fwd(gp, Z.data_ptr(), zb.data_ptr(), lo, hi, s)
    if backward:
        stage.bwd(gp, Z.data_ptr(), zb.data_ptr(), lo, hi, seed, s)
    torch.cuda.current_stream(dev).synchronize()
    stage.b = hi - lo
    return stage


# ------------------------------------------------------------------------------------------------------ training step
class CasaleStepEngine:
    """Owns theta = [encoder | decoder | l_GP, amplitude, alpha | object_vectors], the Adam state and the workspaces of the
    Casale GP-VAE step: one MNIST workspace sized N for the encoder pass over the whole train set, one sized batch_size for
    the decoder (and the VAE regime), and the GP stage's.

    step(regime, lo, hi): the batch is the row range [lo, hi) of the sorted train set.
      joint : minimise elbo w.r.t. everything                                        lr 0.001
      GP    : minimise elbo w.r.t. l_GP, amplitude, alpha (+ object_vectors if ov_joint)   lr 0.01
      VAE   : minimise -elbo_VAE (plain VAE, no clipping) w.r.t. encoder + decoder    lr 0.001
    One Adam state and one step count for all three; variables outside a regime's list keep their moments."""

    def __init__(self, vae, GP, train_images, train_aux, *, batch_size=256, beta=0.001, clipping_qs=False, device="cuda:0",
                 world_size=1, params=None, lr=None):
        if world_size != 1:
            raise _lib.SvgpError(f"CasaleStepEngine: world size {world_size}: the Casale GP-VAE step runs on a single GPU only")
        _need_gpu("CasaleStepEngine")
        self.lib = _lib.load_library()
        self.dev = torch.device(device)
        aux = np.asarray(train_aux.detach().cpu() if torch.is_tensor(train_aux) else train_aux, dtype=np.float64)
        N, L = aux.shape[0], vae.L
        if not np.array_equal(aux[:, 0], np.arange(N)):
            raise ValueError("train_aux needs the global id column range(N) in front (sort_train_data)")
        angles, obj, ang = _row_index(aux[:, 1:])
        self.N, self.L, self.beta, self.clip = N, L, float(beta), int(bool(clipping_qs))
        self.batch_size = min(int(batch_size), N)
        self.GP, self.vae = GP, vae
        self.lr = dict(REGIME_LR if lr is None else lr)
        self.stage = _GpStage(GP, N, angles, obj, ang, b_cap=self.batch_size, L=L, device=self.dev)
        wl = self.stage.wl
        self.n_enc, self.n_vae, self.n_total = int(wl.n_enc), int(wl.n_vae), int(wl.n_total)
        f64 = dict(dtype=_F64, device=self.dev)
        self.theta, self.grad = torch.zeros(self.n_total, **f64), torch.zeros(self.n_total, **f64)
        self.adam_m, self.adam_v = torch.zeros(self.n_total, **f64), torch.zeros(self.n_total, **f64)
        self.state, self.out = torch.zeros(STATE_LEN, **f64), torch.zeros(8, **f64)
        # the two MNIST workspaces (encoder / decoder stage entry points; no GP part: m = 1)
        base = dict(m=1, L=L, M=1, n_obj=0, N_train=float(N), jitter=1e-6, rep_weight=1.0)
        self._cfgN = MnistCfg(b=N, b_global=N, b_cap=N, **base)
        self._baseB = dict(b_cap=self.batch_size, **base)
        self.wlN, self.wlB = WsLayout(), WsLayout()
        call("svgp_mnist_ws_layout_get", C.byref(self._cfgN), C.byref(self.wlN))
        call("svgp_mnist_ws_layout_get", C.byref(self._cfgB(self.batch_size)), C.byref(self.wlB))
        self.wsN, self.wsB = torch.zeros(self.wlN.total, **f64), torch.zeros(self.wlB.total, **f64)
        self.images = torch.as_tensor(train_images, dtype=_F64).to(self.dev).reshape(N, 28, 28, 1).contiguous()
        # parameter views
        from .VAE_utils import VAE_SHAPES
        self.shapes, off = {}, 0
        self.params, self._gviews = {}, {}
        shp = list(VAE_SHAPES(L)) + [("l_GP", ()), ("amplitude", ()), ("alpha", ()),
                                     ("object_vectors", tuple(GP._object_vectors.shape))]
        for k, s in shp:
            n = int(np.prod(s, dtype=np.int64))
            self.shapes[k], self.params[k], self._gviews[k] = s, self.theta[off:off + n].view(s), self.grad[off:off + n].view(s)
            off += n
        assert off == self.n_total
        init = {k: v for k, v in vae.params.items()}
        init.update(l_GP=GP._l_GP, amplitude=GP._amplitude, alpha=GP._alpha, object_vectors=GP._object_vectors)
        if params:
            init.update(params)
        self.stream = torch.cuda.Stream(device=self.dev)
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))
        self.load_params(init)
        self._last, self._state_set = None, None
        self._marks = None              # stage timing (tools/casale_bench.py): [(stage name, event)] of the last step
        GP._engine = self

    def _cfgB(self, b):
        return MnistCfg(b=b, b_global=b, **self._baseB)

    def enable_stage_timing(self, on=True):
        self._marks = [] if on else None

    def _mark(self, name):
        if self._marks is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(self.stream)
            self._marks.append((name, ev))

    def stage_times_ms(self):
        """{stage: milliseconds} of the last step (enable_stage_timing): time between consecutive events on the stream."""
        self.stream.synchronize()
        out = {}
        for (_, e0), (name, e1) in zip(self._marks[:-1], self._marks[1:]):
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        return out

    def load_params(self, params):
        with torch.cuda.stream(self.stream):
            for k, v in params.items():
                self.params[k].copy_(torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v, dtype=_F64).reshape(self.shapes[k]))
        self.stream.synchronize()

    # ---------------------------------------------------------------------------------------------- the step
    def trainable(self, regime):
        """Contiguous theta ranges a regime updates."""
        gp_hi = self.n_total if self.GP.ov_joint else self.n_vae + 3
        gp_lo = self.n_vae + (3 if self.GP.fixed_gp_params else 0)
        if regime == "VAE":
            return [(0, self.n_vae)]
        if regime == "GP":
            return [(gp_lo, gp_hi)] if gp_hi > gp_lo else []
        return [(0, self.n_vae)] + ([(gp_lo, gp_hi)] if gp_hi > gp_lo else [])

    def step(self, regime, lo, hi, eps_full=None, eps_batch=None, adam=True):
        if regime not in REGIMES:
            raise ValueError(f"regime {regime!r}: one of {REGIMES}")
        if not (0 <= lo < hi <= self.N) or hi - lo > self.batch_size:
            raise _lib.SvgpError(f"batch range [{lo}, {hi}) outside [0, N = {self.N}] or longer than batch_size = {self.batch_size}")
        b, L, N, st = hi - lo, self.L, self.N, self.stage
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self.stream):        # drawn on the stream whose kernels read them: no reuse before they ran
            eps_b = _normal((b, L), self.dev, eps_batch).contiguous()
            eps_f = _normal((N, L), self.dev, eps_full).contiguous() if regime != "VAE" else None
        s = self.stream.cuda_stream
        th, cfgN, cfgB = self.theta.data_ptr(), C.byref(self._cfgN), C.byref(self._cfgB(b))
        wsN, wsB, img, img_b = self.wsN.data_ptr(), self.wsB.data_ptr(), self.images.data_ptr(), self.images[lo:hi].data_ptr()
        vN = lambda n: self.wsN[getattr(self.wlN, n):].data_ptr()
        vB = lambda n: self.wsB[getattr(self.wlB, n):].data_ptr()
        ccfg, cws, state = C.byref(st.cfg), st.ws.data_ptr(), self.state.data_ptr()
        gp = self.theta[self.n_vae:]
        mk = self._mark
        if self._marks is not None:
            self._marks = []
        with torch.cuda.stream(self.stream):
            mk("start")
            self.grad.zero_()
            if self._state_set != (self.lr[regime], self.beta):          # host-to-device writes only when a value changes
                self.state[STATE["LR"]] = self.lr[regime]
                self.state[STATE["BETA"]] = self.beta
                self._state_set = (self.lr[regime], self.beta)
            if regime == "VAE":
                scale = 0.5 / _SIGMA_VAE ** 2 * 784.0
                mk("setup")
                call("svgp_mnist_encoder_fwd", cfgB, th, img_b, wsB, s)
                mk("encoder_fwd")
                call("svgp_casale_vae_sample", ccfg, b, vB("qnet_mu"), vB("qnet_var_raw"), eps_b.data_ptr(), vB("z"), cws, s)
                mk("sample")
                call("svgp_mnist_decoder_fwd", cfgB, th, img_b, wsB, s)
                mk("decoder_fwd")
                call("svgp_mnist_decoder_bwd", cfgB, th, img_b, wsB, state, s)
                mk("decoder_bwd")
                call("svgp_casale_vae_seeds", ccfg, b, scale, vB("qnet_mu"), vB("qnet_var_raw"), eps_b.data_ptr(), vB("zbar"),
                     vB("ybar"), vB("s2bar"), s)
                mk("seeds")
                call("svgp_mnist_encoder_bwd", cfgB, th, img_b, wsB, s)
                mk("encoder_bwd")
                call("svgp_mnist_grad_reduce", cfgB, wsB, s)
                g = self.wsB[self.wlB.grad:self.wlB.grad + self.n_vae]
                call("svgp_scale_f64", self.n_vae - self.n_enc, scale, g[self.n_enc:].data_ptr(), s)
                self.grad[:self.n_vae].copy_(g)
                mk("grad_reduce")
            else:
                mk("setup")
                call("svgp_mnist_encoder_fwd", cfgN, th, img, wsN, s)
                mk("encoder_fwd")
                call("svgp_casale_sample", ccfg, self.clip, lo, hi, vN("qnet_mu"), vN("qnet_var_raw"), eps_f.data_ptr(),
                     eps_b.data_ptr(), vB("z"), cws, s)
                mk("sample")
                st.fwd(gp, st.ptr("Z"), st.ptr("zb"), lo, hi, s)
                mk("gp_fwd")
                call("svgp_mnist_decoder_fwd", cfgB, th, img_b, wsB, s)
                mk("decoder_fwd")
                seed = -self.beta / L
                st.bwd(gp, st.ptr("Z"), st.ptr("zb"), lo, hi, seed, s)
                mk("gp_bwd")
                if regime == "joint":
                    call("svgp_mnist_decoder_bwd", cfgB, th, img_b, wsB, state, s)
                    mk("decoder_bwd")
                    call("svgp_casale_seeds", ccfg, self.clip, lo, hi, vN("qnet_var_raw"), eps_f.data_ptr(), eps_b.data_ptr(),
                         vB("zbar"), 0.5 * seed, vN("ybar"), vN("s2bar"), cws, s)
                    mk("seeds")
                    call("svgp_mnist_encoder_bwd", cfgN, th, img, wsN, s)
                    mk("encoder_bwd")
                    call("svgp_mnist_grad_reduce", cfgN, wsN, s)
                call("svgp_mnist_grad_reduce", cfgB, wsB, s)        # decoder weights (joint) and the squared-error sum
                if regime == "joint":
                    self.grad[:self.n_enc].copy_(self.wsN[self.wlN.grad:self.wlN.grad + self.n_enc])
                    self.grad[self.n_enc:self.n_vae].copy_(self.wsB[self.wlB.grad + self.n_enc:self.wlB.grad + self.n_vae])
                n_gp = self.n_total - self.n_vae
                self.grad[self.n_vae:].copy_(st.ws[st.wl.grad_gp:st.wl.grad_gp + n_gp])
                mk("grad_reduce")
            if adam:
                for a0, a1 in self.trainable(regime):
                    call("svgp_adam_tf1_step", a1 - a0, self.theta[a0:].data_ptr(), self.grad[a0:].data_ptr(),
                         self.adam_m[a0:].data_ptr(), self.adam_v[a0:].data_ptr(), state, 0.9, 0.999, 1e-8, s)
            call("svgp_casale_finalize", ccfg, int(regime == "VAE"), b, self.beta, _SIGMA_VAE, vB("sums"), int(bool(adam)), cws,
                 self.out.data_ptr(), state, s)
            mk("adam_finalize")
        self._last = (regime, lo, hi)
        return self

    # ---------------------------------------------------------------------------------------------- results
    def synchronize(self):
        self.stream.synchronize()

    def scalars(self):
        self.stream.synchronize()
        o, stt = self.out.cpu(), self.state.cpu()
        d = dict(elbo=float(o[0]), recon_loss=float(o[1]), adam_t=float(stt[STATE["ADAM_T"]]), lr=float(stt[STATE["LR"]]))
        if self._last and self._last[0] == "VAE":
            d["KL_term"] = float(o[4])
        else:
            d.update(GP_prior_term=float(o[2]), log_var=float(o[3]))
        return d

    def grads(self):
        """Gradient of the regime's objective; exactly zero outside the regime's variable list."""
        self.stream.synchronize()
        return {k: v.clone() for k, v in self._gviews.items()}

    def ws_view(self, name):
        """An intermediate of the last step: the GP stage's fields (K_W, L_W, V, G, P, W, U, A, Abar, Zbar, zbbar, Vbar, ...),
        or qnet_mu / qnet_var / recon / z of the batch."""
        self.stream.synchronize()
        regime, lo, hi = self._last
        b = hi - lo
        if name in _GpStage.SHAPES:
            return self.stage.named(name, b)
        mn = lambda ws, wl, n, shape: ws[getattr(wl, n):getattr(wl, n) + int(np.prod(shape))].view(shape)
        if name == "recon":
            return mn(self.wsB, self.wlB, "recon", (b, 28, 28, 1))
        if name == "z":
            return mn(self.wsB, self.wlB, "z", (b, self.L))
        if regime == "VAE":
            return mn(self.wsB, self.wlB, dict(qnet_mu="qnet_mu", qnet_var="qnet_var_raw")[name], (b, self.L))
        if name == "qnet_mu":
            return mn(self.wsN, self.wlN, "qnet_mu", (self.N, self.L))[lo:hi]
        if name == "qnet_var":
            return self.stage.named("qvar_b", b)
        raise KeyError(name)

    def posterior_cache(self, latent="sample", eps_full=None):
        """generate.CasalePosteriorCache of the engine's live parameters: the encoder pass over the N train images on the
        engine's own workspace, Z as `encode` forms it (latent="mean": qnet_mu), then the cache on the engine's GP stage.
        No parameter leaves the device.  The stage's workspace is rewritten: ws_view of the last step is void afterwards."""
        from .generate import CasalePosteriorCache
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self.stream):
            call("svgp_mnist_encoder_fwd", C.byref(self._cfgN), self.theta.data_ptr(), self.images.data_ptr(), self.wsN.data_ptr(),
                 self.stream.cuda_stream)
            take = lambda n: self.wsN[getattr(self.wlN, n):getattr(self.wlN, n) + self.N * self.L].view(self.N, self.L)
            Z = CasalePosteriorCache._latents(take("qnet_mu"), take("qnet_var_raw"), bool(self.clip), latent, eps_full)
        self.stream.synchronize()
        return CasalePosteriorCache._from_stage(self.theta, self.stage, self.GP.ov_joint, Z)

    def predict(self, test_images, test_aux, take_mean=False, eps_full=None, epsilon=None):
        """predict_test_set_Casale with the engine's current parameters: a fresh latent sample of the train set, then the
        GP predictive posterior at the test rows."""
        self.stream.synchronize()
        vae, GP = self.vae, self.GP
        vae.params = {k: self.params[k].detach().cpu().clone() for k in vae.params}
        Z = encode(self.images, vae, clipping_qs=bool(self.clip), epsilon=eps_full)
        st = self.stage
        st.build_V(self.theta[self.n_vae:])
        V = st.view("V", (st.N, st.H))
        aux = torch.cat([torch.arange(self.N, dtype=_F64, device=self.dev)[:, None],
                         torch.stack([st.obj_idx.to(_F64), st.angles[st.ang_idx.long()]], 1)], 1)
        if not GP.ov_joint:
            aux = torch.cat([aux, self.params["object_vectors"][st.obj_idx.long()]], 1)
        return predict_test_set_Casale(test_images, test_aux, aux, vae, GP, V, Z, take_mean=take_mean, epsilon=epsilon)
