"""Moving-ball models after training (DESIGN.md sections 9h, 9i): reconstruct dropped frames, render a video at another time grid,
extrapolate a few frames -- from a `BALL_experiment --save_model` checkpoint.

    python -m svgp_vae_amd.ball_predict --checkpoint RUN/model.pt (--videos F.npy | --test_batch K --base_dir D)
        [--drop 0.5 --drop_seed S | --observed mask.npy] [--upsample R | --query_times t1 t2 ..]
        [--sample | --sample_paths [--path_jitter J]] [--seed S] [--save_cov cov.npy] [--stream_chunk K] --out frames.npy

BallPredictor (SVGPVAE_Hensman / SVGPVAE_Titsias): the GP posterior of SVGP.approximate_posterior_params (SVGPVAE_model.py:142-171)
is evaluated at arbitrary query times from the frames that are observed (a dropped frame is a frame of precision 0):
svgp_ball_predict, ONE launch per batch for m <= 64 whatever the number of videos and query times, svgp_ball_predict_large beyond.
`predict(paths=True)` draws one coherent path per video, z = p_m + chol(C + path_jitter I) eps with the full posterior covariance C
over the query times, and `return_cov=True` returns C: svgp_ball_predict_joint, ONE launch for m <= 64 and
Q <= 64, svgp_ball_predict_joint_large beyond.
`BallPredictor.state(B)` returns a BallPosteriorState: `observe` adds frames as they arrive to the two additive
statistics the sparse posterior depends on (svgp_ball_state_update), `predict` finalises them once (svgp_ball_state_finalize) and then
serves any number of query grids without an encoder pass (svgp_ball_state_query, svgp_ball_state_query_joint).
PearcePredictor (the exact-GP baselines GPVAE_Pearce / NP / VAE): build_1d_gp (GPVAE_Pearce_model.py:8-86) with a general X_test on
the observed frames of each video: svgp_pearce_predict, ONE launch, up to 64 frames, svgp_pearce_predict_long beyond.
load_predictor picks the class from the checkpoint, so the command line serves all five --elbo values.  Encoder and decoder are
those of the training engines (ball._BallMlpEngine).  Forward only: no gradient, no Adam state, no random-number state is touched."""
import argparse
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import (BALL_STATE_OPS, BallPredictBufs, BallPredictCfg, BallPredictJointBufs, BallPredictJointCfg, BallStateBufs,
                   BallStateCfg, PearcePredictBufs, PearcePredictCfg, SvgpError, call)
from .ball import _BallMlpEngine, mlp_param_shapes

_F64 = torch.float64
CLIP_PV = (1e-4, 1000.0)                                  # SVGPVAE_model.py:701: only the sample clamps
FUSED_M_MAX = 64
JOINT_FUSED_Q_MAX = 64
PEARCE_FUSED_T_MAX = 64
STATE_UPDATE_T_MAX = {False: 16384, True: 2048}           # frames of one svgp_ball_state_update call: fused route, large route
META_KEYS = ("tmax", "m", "hidden", "px", "py", "jitter", "clip_qs")
PEARCE_META_KEYS = ("tmax", "hidden", "px", "py")          # all an exact-GP model's shape needs; m, jitter, clip_qs are ignored
_PEARCE_ELBOS = ("GPVAE_Pearce", "NP", "VAE")


def joint_is_fused(m, Q):
    return m <= FUSED_M_MAX and Q <= JOINT_FUSED_Q_MAX


def route(shape, joint=False):
    """The kernels of the GP stage of one `predict` call of shape (B, T, m, Q), in launch order (svgp_ball_predict_route); needs
    no device.  joint: those of the joint entry a call with paths / return_cov adds (svgp_ball_predict_joint_route)."""
    B, T, m, Q = shape
    buf = C.create_string_buffer(1 << 16)
    if joint:
        cfg = BallPredictJointCfg(B=int(B), T=int(T), m=int(m), Q=int(Q), jitter=0.0, path_jitter=0.0)
        call("svgp_ball_predict_joint_route", C.byref(cfg), int(not joint_is_fused(m, Q)), buf, len(buf))
        return buf.value.decode().split()
    cfg = BallPredictCfg(B=int(B), T=int(T), m=int(m), Q=int(Q), jitter=0.0, clip_lo=CLIP_PV[0], clip_hi=CLIP_PV[1])
    call("svgp_ball_predict_route", C.byref(cfg), int(m > FUSED_M_MAX), buf, len(buf))
    return buf.value.decode().split()


def state_route(op, shape, q_slices=0):
    """The kernels of one svgp_ball_state_<op> call (op: update, finalize, query, query_joint) of shape (B, T, m, Q), in launch order
    (svgp_ball_state_route); needs no device.  The large routes serve m > 64; the joint query has no other."""
    B, T, m, Q = shape
    buf = C.create_string_buffer(1 << 16)
    cfg = BallStateCfg(B=int(B), T=int(T), m=int(m), Q=int(Q), large=int(m > FUSED_M_MAX), q_slices=int(q_slices), jitter=0.0,
                       clip_lo=CLIP_PV[0], clip_hi=CLIP_PV[1], path_jitter=0.0)
    call("svgp_ball_state_route", C.byref(cfg), BALL_STATE_OPS[op], buf, len(buf))
    return buf.value.decode().split()


def pearce_route(shape, q_slices=0):
    """The kernels of the GP stage of one `PearcePredictor.predict` call of shape (B, T, Q), in launch order
    (svgp_pearce_predict_route); needs no device."""
    B, T, Q = shape
    buf = C.create_string_buffer(1 << 16)
    cfg = PearcePredictCfg(B=int(B), T=int(T), Q=int(Q), q_slices=int(q_slices))
    call("svgp_pearce_predict_route", C.byref(cfg), int(T > PEARCE_FUSED_T_MAX), buf, len(buf))
    return buf.value.decode().split()


def param_shapes(m, px=32, py=32, hidden=500):
    """The flat parameter vector of the sparse-GP ball engines: the MLPs, then ip_x, l_x, ip_y, l_y."""
    sh = dict(mlp_param_shapes(px, py, hidden))
    sh.update(ip_x=(m,), l_x=(1,), ip_y=(m,), l_y=(1,))
    return sh


def pearce_param_shapes(px=32, py=32, hidden=500):
    """The flat parameter vector of the exact-GP ball engines: the MLPs, then l_x, l_y."""
    sh = dict(mlp_param_shapes(px, py, hidden))
    sh.update(l_x=(1,), l_y=(1,))
    return sh


def _read_checkpoint(path):
    """(checkpoint dict, its shapes as name -> tuple) of a `model.pt` of the moving-ball driver."""
    ck = torch.load(path, map_location="cpu")
    if not isinstance(ck, dict) or "theta" not in ck or "shapes" not in ck:
        raise ValueError(f"{path}: not a checkpoint of the moving-ball driver (needs theta and shapes)")
    return ck, {k: tuple(v) for k, v in dict(ck["shapes"]).items()}


def _split_theta(path, ck, got, want, what):
    """name -> slice of the checkpoint's theta, after its shapes were checked against the model's (`what` describes the model)."""
    want = {k: tuple(v) for k, v in want.items()}
    if got != want:
        bad = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k, ()))
        raise ValueError(f"{path}: the checkpoint's shapes do not fit {what} (differing: {bad})")
    theta = torch.as_tensor(ck["theta"], dtype=_F64).reshape(-1)
    need = sum(int(np.prod(s)) for s in want.values())
    if theta.numel() != need:
        raise ValueError(f"{path}: theta has {theta.numel()} elements, the shapes describe {need}")
    params, off = {}, 0
    for k, s in got.items():
        n = int(np.prod(s))
        params[k] = theta[off:off + n]
        off += n
    return params


def _as_times(t):
    return torch.as_tensor(np.asarray(t, dtype=np.float64) if not torch.is_tensor(t) else t, dtype=_F64).reshape(-1)


def _check_observed(observed, B, T):
    if observed is not None:
        observed = torch.as_tensor(np.asarray(observed) if not torch.is_tensor(observed) else observed)
        if tuple(observed.shape) != (B, T):
            raise ValueError(f"observed must be (B, T) = ({B}, {T}), got {tuple(observed.shape)}")
    return observed


def _check_frame_times(frame_times, T):
    if frame_times is not None:
        frame_times = _as_times(frame_times)
        if frame_times.numel() != T:
            raise ValueError(f"frame_times must have T = {T} entries, got {frame_times.numel()}")
    return frame_times


def _check_eps(eps, B, Q):
    if eps is not None:
        eps = torch.as_tensor(np.asarray(eps) if not torch.is_tensor(eps) else eps, dtype=_F64)
        if tuple(eps.shape) != (B, Q, 2):
            raise ValueError(f"eps must be (B, Q, 2) = ({B}, {Q}, 2), got {tuple(eps.shape)}")
    return eps


def _check_paths_finite(out, path_jitter):
    bad = (~torch.isfinite(out["z"])).any(2).any(1).nonzero().reshape(-1).tolist()
    if bad:
        raise SvgpError(f"sample paths of video{'s' if len(bad) != 1 else ''} {', '.join(str(b) for b in bad)} are not finite: "
                        f"C + path_jitter I has no Cholesky factor in float64 at path_jitter = {path_jitter:g} (or the inputs "
                        "are not finite); raise path_jitter")


class _Predictor(_BallMlpEngine):
    """What the two predictors share: the flat parameter vector on the device (_BallMlpEngine._init_params), loading a checkpoint,
    `predict` around the GP stage, and the GP call itself.  A subclass sets `clip_qs` (the clamp of the encoder head), names its
    family (_KIND, _SPARSE, and _REFUSAL for a checkpoint of the other one), its meta keys and shapes (_META_KEYS, _SHAPE_KEYS,
    _shapes) and its two GP entries (_ENTRIES), and provides _gp_stage."""

    def _setup(self, params, shapes, *, tmax, hidden, px, py, device):
        self._init_params(shapes, params, self._KIND, px=px, py=py, hidden=hidden, device=device)
        self.tmax = int(tmax)
        self._work = torch.empty(0, dtype=_F64, device=self.dev)

    # ------------------------------------------------------------------ checkpoints
    @classmethod
    def load(cls, path, **overrides):
        """A predictor from the `model.pt` of `BALL_experiment --save_model`.  The model's shape comes from the checkpoint's "meta"
        dict (of which the class reads its _META_KEYS only); keywords override it, and stand in for it where an older checkpoint
        has none."""
        ck, shapes = _read_checkpoint(path)
        meta = dict(ck.get("meta") or {})
        device = overrides.pop("device", "cuda:0")
        meta.update(overrides)
        # the family is told by the inducing points, and by the meta dict's elbo where it has one
        if ("ip_x" in shapes) != cls._SPARSE or ("elbo" in meta and (meta["elbo"] not in _PEARCE_ELBOS) != cls._SPARSE):
            raise ValueError(f"{path}: {cls._REFUSAL}")
        missing = [k for k in cls._META_KEYS if k not in meta]
        if missing:
            raise ValueError(f"{path}: the checkpoint has no meta entry for {', '.join(missing)}; pass "
                             f"{', '.join(k + '=...' for k in missing)} to {cls.__name__}.load")
        want = cls._shapes(**{k: int(meta[k]) for k in cls._SHAPE_KEYS})
        params = _split_theta(path, ck, shapes, want, " ".join(f"{k}={meta[k]}" for k in cls._SHAPE_KEYS))
        return cls(params, device=device, **{k: meta[k] for k in cls._META_KEYS})

    # ------------------------------------------------------------------ the GP call
    @staticmethod
    def _set_xy(q, **pairs):
        """q.<name>_x, q.<name>_y = the device pointers of each pair (None stays NULL)."""
        for k, pair in pairs.items():
            for cn, t in zip("xy", pair):
                setattr(q, f"{k}_{cn}", None if t is None else t.data_ptr())

    def _run_gp(self, fused, cfg, q, entries=None):
        """The one-launch entry, or the workspace entry on `self._work` sized by its *_workspace_elems entry."""
        one, many = entries or self._ENTRIES
        if fused:
            return call(one, C.byref(cfg), C.byref(q), self.stream.cuda_stream)
        need = int(getattr(self.lib, many + "_workspace_elems")(C.byref(cfg)))      # 0: a shape the entry refuses (it says why)
        if self._work.numel() < need:
            self._work = torch.empty(need, dtype=_F64, device=self.dev)              # grows once per shape
        call(many, C.byref(cfg), C.byref(q), self._work.data_ptr() if need else None, self.stream.cuda_stream)

    # ------------------------------------------------------------------ frames
    def _check_joint(self, paths, return_cov, eps, path_jitter):
        """The joint arguments of `predict`, checked before anything else; returns the path jitter to use."""
        if paths or return_cov:
            if not self._SPARSE:
                raise NotImplementedError(f"{type(self).__name__}: the joint posterior over the query times (paths / return_cov) is "
                                          "implemented for the sparse-GP models only, by BallPredictor")
            if paths and eps is None:
                raise ValueError("paths=True needs eps (B, Q, 2)")
            path_jitter = self.jitter if path_jitter is None else float(path_jitter)
            if not (path_jitter >= 0.0 and np.isfinite(path_jitter)):
                raise ValueError(f"path_jitter must be finite and >= 0, got {path_jitter}")
        elif path_jitter is not None:
            raise ValueError("path_jitter applies to paths=True / return_cov=True only")
        return path_jitter

    def _check_videos(self, videos):
        videos = torch.as_tensor(np.asarray(videos) if not torch.is_tensor(videos) else videos)
        if videos.dim() != 4 or tuple(videos.shape[2:]) != (self.px, self.py):
            raise ValueError(f"videos must be (B, T, {self.px}, {self.py}), got {tuple(videos.shape)}")
        return videos

    def _encode_head(self, videos):
        """videos (B, T, px, py) -> mu, var: two (T, B) tensors each, the frame-major layout of svgp_ball_head_fwd.  On self.stream."""
        B, T = int(videos.shape[0]), int(videos.shape[1])
        f64 = dict(dtype=_F64, device=self.dev)
        X = videos.to(self.dev, _F64).contiguous().view(B * T, self.P)
        _, h2 = self._encode(X)
        mu, var_raw, var = ([torch.empty(T, B, **f64) for _ in range(2)] for _ in range(3))
        call("svgp_ball_head_fwd", B, T, int(self.clip_qs), self.params["encB2"].data_ptr(), h2.data_ptr(), mu[0].data_ptr(),
             var_raw[0].data_ptr(), var[0].data_ptr(), mu[1].data_ptr(), var_raw[1].data_ptr(), var[1].data_ptr(), self.stream.cuda_stream)
        return mu, var

    def _decode_out(self, B, Q, p_m, p_v, zc, extra):
        """The dict `predict` returns from the GP stage's (Q, B) pairs: svgp_ball_pack_z, the decoder, the sigmoid.  On self.stream."""
        s, P = self.stream.cuda_stream, self.P
        f64 = dict(dtype=_F64, device=self.dev)
        z = torch.empty(B * Q, 2, **f64)
        call("svgp_ball_pack_z", B, Q, zc[0].data_ptr(), zc[1].data_ptr(), z.data_ptr(), s)
        _, logits = self._decode_logits(z)
        # sigmoid by the training engines' kernel; its cross-entropy row sums (against the logits themselves) are not used
        frames, row = torch.empty(B * Q, P, **f64), torch.empty(B * Q, **f64)
        call("svgp_sigmoid_xent", B * Q, P, 1.0, logits.data_ptr(), logits.data_ptr(), frames.data_ptr(), row.data_ptr(),
             None, s)
        st2 = lambda v: torch.stack([v[0].t(), v[1].t()], 2).contiguous()
        return dict(frames=frames.view(B, Q, self.px, self.py), p_m=st2(p_m), p_v=st2(p_v), z=z.view(B, Q, 2), **extra)

    def predict(self, videos, query_times, observed=None, frame_times=None, eps=None, paths=False, return_cov=False, path_jitter=None):
        """videos (B, T, px, py); query_times (Q) arbitrary reals; observed (B, T) bool, default all; frame_times (T), default 1..T;
        eps (B, Q, 2) or None (decode the posterior mean).  Returns dict(frames (B, Q, px, py) in [0, 1], p_m, p_v, z (B, Q, 2));
        PearcePredictor adds lh (B, 2).
        BallPredictor only: paths=True (needs eps) makes z, and with it frames, ONE coherent sample path per video, z = p_m +
        chol(C + path_jitter I) eps with C the posterior covariance over the query times (path_jitter defaults to the model's
        jitter) instead of an independent draw per query time; return_cov=True adds p_cov (B, 2, Q, Q) = C."""
        path_jitter = self._check_joint(paths, return_cov, eps, path_jitter)
        videos = self._check_videos(videos)
        B, T = int(videos.shape[0]), int(videos.shape[1])
        tq = _as_times(query_times)
        Q = int(tq.numel())
        if B < 1 or T < 1 or Q < 1:
            raise ValueError(f"need at least one video, frame and query time (B={B} T={T} Q={Q})")
        if not bool(torch.isfinite(tq).all()):
            raise ValueError("query_times must be finite")
        observed = _check_observed(observed, B, T)
        frame_times = _check_frame_times(frame_times, T)
        eps = _check_eps(eps, B, Q)
        f64 = dict(dtype=_F64, device=self.dev)
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self.stream):
            times = torch.arange(1, T + 1, **f64) if frame_times is None else frame_times.to(self.dev).contiguous()
            tq = tq.to(self.dev).contiguous()
            mask = None if observed is None else observed.to(self.dev).to(_F64).t().contiguous()
            eps_c = None if eps is None else [eps[:, :, c].to(self.dev).t().contiguous() for c in range(2)]
            mu, var = self._encode_head(videos)
            if paths or return_cov:
                p_m, p_v, zc, extra = self._gp_stage_joint(mu, var, times, tq, mask, eps_c, paths, return_cov, path_jitter)
            else:
                p_m, p_v, zc, extra = self._gp_stage(mu, var, times, tq, mask, eps_c)
            out = self._decode_out(B, Q, p_m, p_v, zc, extra)
        self.stream.synchronize()
        if paths:
            _check_paths_finite(out, path_jitter)
        return out


class BallPredictor(_Predictor):
    """A trained moving-ball SVGP-VAE, forward only.  `params`: name -> array for every entry of param_shapes(m, px, py, hidden)."""

    _KIND, _SPARSE, _META_KEYS, _SHAPE_KEYS = "a sparse-GP", True, META_KEYS, ("m", "hidden", "px", "py")
    _REFUSAL = ("a checkpoint of an exact-GP baseline (GPVAE_Pearce / NP / VAE: no inducing points); BallPredictor handles the "
                "sparse-GP models SVGPVAE_Hensman / SVGPVAE_Titsias only, use PearcePredictor")
    _ENTRIES = ("svgp_ball_predict", "svgp_ball_predict_large")
    _shapes = staticmethod(param_shapes)

    def __init__(self, params, *, tmax, m, hidden=500, px=32, py=32, jitter, clip_qs, device="cuda:0"):
        self.m, self.jitter, self.clip_qs = int(m), float(jitter), bool(clip_qs)
        self._setup(params, param_shapes(int(m), int(px), int(py), int(hidden)), tmax=tmax, hidden=hidden, px=px, py=py,
                    device=device)

    def route(self, B, T, Q, joint=False):
        return route((B, T, self.m, Q), joint)

    def state(self, B):
        """An empty BallPosteriorState for B videos: observe frames as they arrive, query as often as wanted."""
        return BallPosteriorState(self, B)

    # ------------------------------------------------------------------ the GP stage alone
    def _gp(self, mu, var, times, tq, mask, eps_c, force_large=False):
        """mu, var: two (T, B) tensors each; mask (T, B) or None; eps_c: two (Q, B) tensors or None.  Returns p_m, p_v, z lists.
        force_large: the workspace entry also where the one-launch entry takes the shape (timings)."""
        T, B = mu[0].shape
        Q, p = tq.numel(), self.params
        out = {k: [torch.empty(Q, B, dtype=_F64, device=self.dev) for _ in range(2)] for k in ("p_m", "p_v", "z")}
        cfg = BallPredictCfg(B=B, T=T, m=self.m, Q=Q, jitter=self.jitter, clip_lo=CLIP_PV[0], clip_hi=CLIP_PV[1])
        q = BallPredictBufs()
        q.times, q.tq, q.mask = times.data_ptr(), tq.data_ptr(), None if mask is None else mask.data_ptr()
        self._set_xy(q, ip=(p["ip_x"], p["ip_y"]), ls=(p["l_x"], p["l_y"]), mu=mu, var=var, eps=eps_c or (None, None), **out)
        self._run_gp(self.m <= FUSED_M_MAX and not force_large, cfg, q)
        return out["p_m"], out["p_v"], out["z"]

    def _gp_stage(self, mu, var, times, tq, mask, eps_c):
        return self._gp(mu, var, times, tq, mask, eps_c) + ({},)

    def _gp_joint(self, mu, var, times, tq, mask, eps_c, path_jitter, want_cov=True, want_chol=False, want_z=True,
                  force_large=False):
        """The joint entry alone.  Returns dict(p_m, z: two (Q, B) tensors each; cov, chol: two (B, Q, Q) tensors each); an output
        that was not asked for is None.  force_large: as in _gp."""
        T, B = mu[0].shape
        Q, p = tq.numel(), self.params
        new = lambda *shape: [torch.empty(*shape, dtype=_F64, device=self.dev) for _ in range(2)]
        out = dict(p_m=new(Q, B), cov=new(B, Q, Q) if want_cov else None, chol=new(B, Q, Q) if want_chol else None,
                   z=new(Q, B) if want_z else None)
        cfg = BallPredictJointCfg(B=B, T=T, m=self.m, Q=Q, jitter=self.jitter, path_jitter=path_jitter)
        q = BallPredictJointBufs()
        q.times, q.tq, q.mask = times.data_ptr(), tq.data_ptr(), None if mask is None else mask.data_ptr()
        self._set_xy(q, ip=(p["ip_x"], p["ip_y"]), ls=(p["l_x"], p["l_y"]), mu=mu, var=var, eps=eps_c or (None, None),
                     **{k: v or (None, None) for k, v in out.items()})
        self._run_gp(joint_is_fused(self.m, Q) and not force_large, cfg, q, ("svgp_ball_predict_joint", "svgp_ball_predict_joint_large"))
        return out

    def _gp_stage_joint(self, mu, var, times, tq, mask, eps_c, paths, return_cov, path_jitter):
        """p_v (and, without paths, p_m and the independent draw z) from the marginal entry, whose keys keep their bits; the path
        and the covariance from the joint one, whose p_m the path is built on."""
        p_m, p_v, z = self._gp(mu, var, times, tq, mask, None if paths else eps_c)
        j = self._gp_joint(mu, var, times, tq, mask, eps_c if paths else None, path_jitter, want_cov=return_cov, want_z=paths)
        extra = dict(p_cov=torch.stack(j["cov"], 1)) if return_cov else {}
        return (j["p_m"], p_v, j["z"], extra) if paths else (p_m, p_v, z, extra)


class BallPosteriorState:
    """The streamed posterior of B videos under a BallPredictor, on the predictor's device and stream.

    The sparse posterior depends on the frames only through S = Kn^T diag(p) Kn and r = Kn^T (p y) per video and latent coordinate.
    `stats` (B, 2, m m + m) holds them (zeros: nothing observed, the prior), `post` (B, 2, m m + m) the X and w the queries need; it
    is formed from `stats` by the first `predict` after an `observe`.  m <= 64 runs the one-launch routes of svgp_ball_state_*,
    larger m their large routes; the joint query is the large one for every shape."""

    def __init__(self, pred, B):
        if not isinstance(pred, BallPredictor):
            raise TypeError(f"BallPosteriorState needs a BallPredictor (the sparse-GP models), got {type(pred).__name__}")
        if int(B) < 1:
            raise ValueError(f"need at least one video (B={B})")
        self.pred, self.B, self.large = pred, int(B), pred.m > FUSED_M_MAX
        pred.stream.wait_stream(torch.cuda.current_stream(pred.dev))
        with torch.cuda.stream(pred.stream):
            self.stats, self.post = (torch.zeros(self.B, 2, pred.m * pred.m + pred.m, dtype=_F64, device=pred.dev) for _ in range(2))
        self.n_seen, self._dirty = 0, True

    # ------------------------------------------------------------------ the library calls
    def _cfg(self, T=0, Q=0, path_jitter=0.0, q_slices=0):
        pred = self.pred
        return BallStateCfg(B=self.B, T=int(T), m=pred.m, Q=int(Q), large=int(self.large), q_slices=int(q_slices), jitter=pred.jitter,
                            clip_lo=CLIP_PV[0], clip_hi=CLIP_PV[1], path_jitter=float(path_jitter))

    def _bufs(self, **pairs):
        pred, p = self.pred, self.pred.params
        q = BallStateBufs()
        q.stats, q.post = self.stats.data_ptr(), self.post.data_ptr()
        pred._set_xy(q, ip=(p["ip_x"], p["ip_y"]), ls=(p["l_x"], p["l_y"]), **pairs)
        return q

    def _call(self, op, cfg, q):
        pred = self.pred
        need = int(pred.lib.svgp_ball_state_workspace_elems(C.byref(cfg), BALL_STATE_OPS[op]))    # 0: a fused route, or a refusal
        if pred._work.numel() < need:
            pred._work = torch.empty(need, dtype=_F64, device=pred.dev)                           # grows once per shape
        call("svgp_ball_state_" + op, C.byref(cfg), C.byref(q), pred._work.data_ptr() if need else None, pred.stream.cuda_stream)

    # ------------------------------------------------------------------ the GP stage alone (on the predictor's stream)
    def _update(self, mu, var, times, mask):
        """mu, var: two (T, B) tensors each; times (T); mask (T, B) or None.  As many svgp_ball_state_update calls as the route's
        frames-per-call limit asks for: (T, B) is frame-major, so a run of frames is a contiguous block."""
        T, step = int(times.numel()), STATE_UPDATE_T_MAX[self.large]
        for t0 in range(0, T, step):
            t1 = min(T, t0 + step)
            q = self._bufs(mu=[v[t0:t1] for v in mu], var=[v[t0:t1] for v in var])
            q.times, q.mask = times[t0:t1].data_ptr(), None if mask is None else mask[t0:t1].data_ptr()
            self._call("update", self._cfg(T=t1 - t0), q)
        self._dirty = True

    def _finalize(self):
        if self._dirty:
            self._call("finalize", self._cfg(), self._bufs())
            self._dirty = False

    def _new(self, *shape):
        return [torch.empty(*shape, dtype=_F64, device=self.pred.dev) for _ in range(2)]

    def _query(self, tq, eps_c, q_slices=0):
        """tq (Q) on the device; eps_c: two (Q, B) tensors or None.  Returns the p_m, p_v, z lists of (Q, B) tensors."""
        Q = int(tq.numel())
        out = {k: self._new(Q, self.B) for k in ("p_m", "p_v", "z")}
        q = self._bufs(eps=eps_c or (None, None), **out)
        q.tq = tq.data_ptr()
        self._call("query", self._cfg(Q=Q, q_slices=q_slices), q)
        return out["p_m"], out["p_v"], out["z"]

    def _query_joint(self, tq, eps_c, path_jitter, want_cov=True, want_chol=False, want_z=True):
        """dict(p_m, z: two (Q, B) tensors each; cov, chol: two (B, Q, Q) tensors each); an output that was not asked for is None."""
        B, Q = self.B, int(tq.numel())
        out = dict(p_m=self._new(Q, B), cov=self._new(B, Q, Q) if want_cov else None, chol=self._new(B, Q, Q) if want_chol else None,
                   z=self._new(Q, B) if want_z else None)
        q = self._bufs(eps=eps_c or (None, None), **{k: v or (None, None) for k, v in out.items()})
        q.tq = tq.data_ptr()
        self._call("query_joint", self._cfg(Q=Q, path_jitter=path_jitter), q)
        return out

    def route(self, op, T=None, Q=None, joint=False):
        """The GP kernels of one step, in launch order; needs no device.  op: "update" (T frames), "finalize", "query", "query_joint"
        (Q query times), or "predict": what `predict` at Q query times would launch now -- the finalize step only when frames were
        observed since the last one, then the marginal query, then with joint=True the joint one."""
        shape = (self.B, 1 if T is None else T, self.pred.m, 1 if Q is None else Q)
        if op == "predict":
            return ((state_route("finalize", shape) if self._dirty else []) + state_route("query", shape)
                    + (state_route("query_joint", shape) if joint else []))
        if op not in BALL_STATE_OPS:
            raise ValueError(f"op must be one of {', '.join(BALL_STATE_OPS)} or predict, got {op!r}")
        return state_route(op, shape)

    # ------------------------------------------------------------------ frames in
    def observe(self, videos, frame_times=None, observed=None):
        """Adds the frames videos (B, T, px, py) to the state; returns the state.  frame_times (T) defaults to n_seen + 1 .. n_seen + T,
        so feeding a video in pieces reproduces BallPredictor.predict's 1..T; observed (B, T) bool, default all."""
        pred = self.pred
        videos = pred._check_videos(videos)
        B, T = int(videos.shape[0]), int(videos.shape[1])
        if B != self.B:
            raise ValueError(f"videos must hold the state's B = {self.B} videos, got {B}")
        if T < 1:
            raise ValueError(f"need at least one video, frame and query time (B={B} T={T} Q=1)")
        observed = _check_observed(observed, B, T)
        frame_times = _check_frame_times(frame_times, T)
        if frame_times is not None and not bool(torch.isfinite(frame_times).all()):
            raise ValueError("frame_times must be finite")
        f64 = dict(dtype=_F64, device=pred.dev)
        pred.stream.wait_stream(torch.cuda.current_stream(pred.dev))
        with torch.cuda.stream(pred.stream):
            times = (torch.arange(self.n_seen + 1, self.n_seen + T + 1, **f64) if frame_times is None
                     else frame_times.to(pred.dev).contiguous())
            mask = None if observed is None else observed.to(pred.dev).to(_F64).t().contiguous()
            self._update(*pred._encode_head(videos), times, mask)
        pred.stream.synchronize()                         # the inputs of this call may go once it returns
        self.n_seen += T
        return self

    # ------------------------------------------------------------------ frames out
    def predict(self, query_times, eps=None, paths=False, return_cov=False, path_jitter=None):
        """The dict of BallPredictor.predict at query_times (Q) from what was observed so far: no encoder pass, no frame is touched.
        eps, paths, return_cov, path_jitter as there."""
        pred = self.pred
        path_jitter = pred._check_joint(paths, return_cov, eps, path_jitter)
        tq = _as_times(query_times)
        B, Q = self.B, int(tq.numel())
        if Q < 1:
            raise ValueError(f"need at least one video, frame and query time (B={B} T={max(self.n_seen, 1)} Q={Q})")
        if not bool(torch.isfinite(tq).all()):
            raise ValueError("query_times must be finite")
        eps = _check_eps(eps, B, Q)
        pred.stream.wait_stream(torch.cuda.current_stream(pred.dev))
        with torch.cuda.stream(pred.stream):
            tq = tq.to(pred.dev).contiguous()
            eps_c = None if eps is None else [eps[:, :, c].to(pred.dev).t().contiguous() for c in range(2)]
            self._finalize()
            # p_v (and, without paths, p_m and the independent draw z) from the marginal query; the path and the covariance from the
            # joint one, whose p_m the path is built on (as BallPredictor._gp_stage_joint)
            p_m, p_v, zc = self._query(tq, None if paths else eps_c)
            extra = {}
            if paths or return_cov:
                j = self._query_joint(tq, eps_c if paths else None, path_jitter, want_cov=return_cov, want_z=paths)
                if return_cov:
                    extra = dict(p_cov=torch.stack(j["cov"], 1))
                if paths:
                    p_m, zc = j["p_m"], j["z"]
            out = pred._decode_out(B, Q, p_m, p_v, zc, extra)
        pred.stream.synchronize()
        if paths:
            _check_paths_finite(out, path_jitter)
        return out

    # ------------------------------------------------------------------ housekeeping
    def reset(self):
        """Back to "nothing observed"; returns the state."""
        pred = self.pred
        pred.stream.wait_stream(torch.cuda.current_stream(pred.dev))
        with torch.cuda.stream(pred.stream):
            self.stats.zero_()
        self.n_seen, self._dirty = 0, True
        return self

    def clone(self):
        """An independent copy: observing into one leaves the other as it is."""
        pred = self.pred
        o = object.__new__(BallPosteriorState)
        o.pred, o.B, o.large, o.n_seen, o._dirty = pred, self.B, self.large, self.n_seen, self._dirty
        pred.stream.wait_stream(torch.cuda.current_stream(pred.dev))
        with torch.cuda.stream(pred.stream):
            o.stats, o.post = self.stats.clone(), self.post.clone()
        return o


class PearcePredictor(_Predictor):
    """A trained exact-GP moving-ball baseline (BALL_experiment --elbo GPVAE_Pearce | NP | VAE), forward only.  `params`: name ->
    array for every entry of pearce_param_shapes(px, py, hidden).

    The posterior of a video at the query times is build_1d_gp (GPVAE_Pearce_model.py:8-86) on its observed frames with X_test =
    the query times; `predict` additionally returns lh (B, 2), the marginal likelihood of the observed frames per coordinate.  The
    encoder head is not clamped, as in _PearceEngineBase.step.  `frame_times` defaults to 1..T like BallPredictor's; the training
    engines count 0..T-1, and since the SE kernel is stationary the posterior at a frame (and lh) is the same under either
    convention.  A checkpoint of --elbo VAE carries the length scale 0.001: a query time that is not an observed frame time gets
    the prior N(0, 1), which is the point of that baseline."""

    clip_qs = False
    # of the "meta" dict only tmax, hidden, px, py are needed
    _KIND, _SPARSE, _META_KEYS, _SHAPE_KEYS = "an exact-GP", False, PEARCE_META_KEYS, ("hidden", "px", "py")
    _REFUSAL = ("a checkpoint of a sparse-GP model (SVGPVAE_Hensman / SVGPVAE_Titsias: it has inducing points); PearcePredictor "
                "handles the exact-GP baselines GPVAE_Pearce / NP / VAE only, use BallPredictor")
    _ENTRIES = ("svgp_pearce_predict", "svgp_pearce_predict_long")
    _shapes = staticmethod(pearce_param_shapes)

    def __init__(self, params, *, tmax, hidden=500, px=32, py=32, device="cuda:0"):
        self._setup(params, pearce_param_shapes(int(px), int(py), int(hidden)), tmax=tmax, hidden=hidden, px=px, py=py,
                    device=device)

    def route(self, B, T, Q):
        return pearce_route((B, T, Q))

    # ------------------------------------------------------------------ the GP stage alone
    def _gp(self, mu, var, times, tq, mask, eps_c, q_slices=0):
        """mu, var: two (T, B) tensors each; mask (T, B) or None; eps_c: two (Q, B) tensors or None.  Returns the p_m, p_v, z lists
        and lh (2, B)."""
        T, B = mu[0].shape
        Q, p = tq.numel(), self.params
        f64 = dict(dtype=_F64, device=self.dev)
        out = {k: [torch.empty(Q, B, **f64) for _ in range(2)] for k in ("p_m", "p_v", "z")}
        lh = torch.empty(2, B, **f64)
        cfg = PearcePredictCfg(B=B, T=T, Q=Q, q_slices=int(q_slices))
        q = PearcePredictBufs()
        q.times, q.tq, q.mask, q.lh = times.data_ptr(), tq.data_ptr(), None if mask is None else mask.data_ptr(), lh.data_ptr()
        self._set_xy(q, ls=(p["l_x"], p["l_y"]), mu=mu, var=var, eps=eps_c or (None, None), **out)
        self._run_gp(T <= PEARCE_FUSED_T_MAX, cfg, q)
        return out["p_m"], out["p_v"], out["z"], lh

    def _gp_stage(self, mu, var, times, tq, mask, eps_c):
        p_m, p_v, z, lh = self._gp(mu, var, times, tq, mask, eps_c)
        return p_m, p_v, z, dict(lh=lh.t().contiguous())


def load_predictor(path, **kw):
    """BallPredictor or PearcePredictor, whichever model the checkpoint holds (told by its inducing points); the class's own load
    does the checking."""
    _, shapes = _read_checkpoint(path)
    return (BallPredictor if "ip_x" in shapes else PearcePredictor).load(path, **kw)


# ---------------------------------------------------------------------------------------------- command line
def build_parser():
    p = argparse.ArgumentParser(description="Fill dropped frames / resample in time with a trained moving-ball model.")
    p.add_argument("--checkpoint", required=True, help="RUN/model.pt of BALL_experiment --save_model")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--videos", type=str, default=None, help=".npy of videos (B, T, px, py)")
    src.add_argument("--test_batch", type=int, default=None, help="index 0..9 of the driver's fixed test batches (needs --base_dir)")
    p.add_argument("--base_dir", type=str, default=None, help="where the driver keeps Test_Batches_<vidlt>_<tmax>.pkl")
    obs = p.add_mutually_exclusive_group()
    obs.add_argument("--drop", type=float, default=None, help="fraction of frames to drop at random (with --drop_seed)")
    obs.add_argument("--observed", type=str, default=None, help=".npy of a (B, T) mask, non-zero = observed")
    p.add_argument("--drop_seed", type=int, default=0)
    qt = p.add_mutually_exclusive_group()
    qt.add_argument("--upsample", type=int, default=None, help="R: the frame times with R - 1 new times between neighbours")
    qt.add_argument("--query_times", type=float, nargs="+", default=None)
    draw = p.add_mutually_exclusive_group()
    draw.add_argument("--sample", action="store_true", help="z = p_m + eps sqrt(p_v) with eps from --seed, an independent draw per query "
                      "time; default: the posterior mean")
    # the joint arguments are absent from the namespace unless given (argparse.SUPPRESS), so that a command line without them
    # parses to the namespace it always did: read them with joint_args
    draw.add_argument("--sample_paths", action="store_true", default=argparse.SUPPRESS,
                      help="one coherent sample path per video, z = p_m + chol(C + J I) eps with eps from --seed (sparse-GP checkpoints)")
    p.add_argument("--path_jitter", type=float, default=argparse.SUPPRESS, help="J of --sample_paths; default: the model's jitter")
    p.add_argument("--save_cov", type=str, default=argparse.SUPPRESS,
                   help=".npy for the posterior covariance over the query times (B, 2, Q, Q)")
    p.add_argument("--stream_chunk", type=int, default=argparse.SUPPRESS,
                   help="K: feed the video through a BallPosteriorState in pieces of K frames, then query it (sparse-GP checkpoints)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--out", required=True)
    return p


def joint_args(args):
    """(sample_paths, path_jitter or None, save_cov or None) of a parsed command line."""
    return getattr(args, "sample_paths", False), getattr(args, "path_jitter", None), getattr(args, "save_cov", None)


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if args.test_batch is not None and args.base_dir is None:
        p.error("--test_batch needs --base_dir")
    if args.test_batch is not None and not 0 <= args.test_batch < 10:
        p.error("--test_batch must be in 0..9")
    if args.drop is not None and not 0.0 <= args.drop < 1.0:
        p.error("--drop must be in [0, 1)")
    if args.upsample is not None and args.upsample < 1:
        p.error("--upsample must be at least 1")
    sample_paths, path_jitter, save_cov = joint_args(args)
    if path_jitter is not None and not path_jitter >= 0.0:
        p.error("--path_jitter must be >= 0")
    if path_jitter is not None and not (sample_paths or save_cov):
        p.error("--path_jitter needs --sample_paths or --save_cov")
    if getattr(args, "stream_chunk", None) is not None and args.stream_chunk < 1:
        p.error("--stream_chunk must be at least 1")
    return args


def query_grid(T, upsample=None, query_times=None):
    """(query times, index of every frame time in them or None)."""
    if query_times is not None:
        return np.asarray(query_times, dtype=np.float64), None
    R = 1 if upsample is None else int(upsample)
    return np.linspace(1.0, float(T), R * (T - 1) + 1), np.arange(T) * R


def main(argv=None):
    args = parse_args(argv)
    pred = load_predictor(args.checkpoint, device=args.device)
    sample_paths, path_jitter, save_cov = joint_args(args)
    joint = sample_paths or save_cov is not None
    if joint and not isinstance(pred, BallPredictor):
        raise SystemExit(f"{args.checkpoint}: --sample_paths, --path_jitter and --save_cov need a sparse-GP checkpoint (SVGPVAE_Hensman / "
                         "SVGPVAE_Titsias, served by BallPredictor); the exact-GP baselines' joint posterior is not implemented")
    stream_chunk = getattr(args, "stream_chunk", None)
    if stream_chunk is not None and not isinstance(pred, BallPredictor):
        raise SystemExit(f"{args.checkpoint}: --stream_chunk needs a sparse-GP checkpoint (SVGPVAE_Hensman / SVGPVAE_Titsias, served by "
                         "BallPredictor): only their posterior has a streamed state; the exact-GP baselines have none")
    if args.videos is not None:
        videos = np.load(args.videos)
    else:
        from .BALL_experiment import load_or_make_test_batches
        meta = torch.load(args.checkpoint, map_location="cpu").get("meta") or {}
        if "vidlt" not in meta:
            raise SystemExit(f"{args.checkpoint}: no meta entry for vidlt; --test_batch needs it, use --videos")
        tb = load_or_make_test_batches(args.base_dir, meta["vidlt"], pred.tmax, pred.px, pred.py, 35, 3)
        videos = np.asarray(tb[args.test_batch][1], dtype=np.float64)
    B, T = videos.shape[:2]
    observed = None
    if args.observed is not None:
        observed = np.load(args.observed) != 0
    elif args.drop is not None:
        observed = np.random.RandomState(args.drop_seed).rand(B, T) >= args.drop
    tq, at_frames = query_grid(T, args.upsample, args.query_times)
    eps = np.random.RandomState(args.seed).randn(B, tq.size, 2) if args.sample or sample_paths else None
    kw = dict(paths=sample_paths, return_cov=save_cov is not None, path_jitter=path_jitter) if joint else {}
    if stream_chunk is None:
        out = pred.predict(videos, tq, observed=observed, eps=eps, **kw)
    else:
        state = pred.state(B)
        for t0 in range(0, T, stream_chunk):
            state.observe(videos[:, t0:t0 + stream_chunk], observed=None if observed is None else observed[:, t0:t0 + stream_chunk])
        state_names = [(op, state.route(op, T=min(stream_chunk, T), Q=tq.size)) for op in ("update", "finalize", "query")]
        out = state.predict(tq, eps=eps, **kw)
    frames = out["frames"].cpu().numpy()
    np.save(args.out, frames)
    if save_cov is not None:
        np.save(save_cov, out["p_cov"].cpu().numpy())
    names = pred.route(B, T, tq.size)
    print(f"{B} videos x {tq.size} query times -> {args.out}   route ({len(names)} GP launch{'es' if len(names) != 1 else ''}): "
          f"{' '.join(names)}")
    if joint:
        names = pred.route(B, T, tq.size, joint=True)
        print(f"joint route ({len(names)} GP launch{'es' if len(names) != 1 else ''}): {' '.join(names)}")
    if stream_chunk is not None:
        if joint:
            state_names.append(("query_joint", state.route("query_joint", Q=tq.size)))
        print(f"state routes (these ran; the one-shot routes above were not launched), {-(-T // stream_chunk)} piece{'s' if T > stream_chunk else ''} of at most {stream_chunk} frames: "
              + "; ".join(f"{op} ({len(n)}): {' '.join(n)}" for op, n in state_names))
    if args.test_batch is not None and observed is not None and at_frames is not None and not observed.all():
        err = (frames[:, at_frames] - videos)[~observed]
        print(f"MSE of the {int((~observed).sum())} filled-in frames against the held-back ones: {float((err ** 2).mean()):.6g}")
    return frames


if __name__ == "__main__":
    main()
