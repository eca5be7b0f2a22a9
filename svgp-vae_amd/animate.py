"""Animate a character the SPRITES SVGP-VAE has not seen, from a checkpoint and without the train set: the posterior cache.

The GP posterior of spritesSVGP.approximate_posterior_params_precomputed_GP_posterior_params (SVGPVAE_model.py:610-635) depends
on the train rows only through w_l = Sigma_l^-1 K_mn (mu_l / var_l) (L, m) and X_l = Sigma_l^-1 - K_mm^-1 (L, m, m) (DESIGN.md
section 9g).  SpritesPosteriorCache.build walks the train rows ONCE in chunks of whole character groups and forms the two;
`animate` then turns the context frames of new characters and the actions wanted of them into frames: representation network on
the context frames, kernel rows of the queries [action id, character vector], ONE call of svgp_sprites_posterior_rows for the
moments and the latent rows (one launch up to m = 256, two beyond), decode.  No train frame is touched, no random-number
state is touched.

    cache = SpritesPosteriorCache.build(vae, repr_nn, svgp, train_frames, train_action_ids, frames_per_character=50, chunk=500)
    frames = animate(cache, context_frames, target_actions)            # (C, T, 64, 64, 3): decode of the posterior mean
    frames, p_m, p_v = animate(cache, context_frames, target_actions, eps=eps, return_moments=True)
    cache.save(path); SpritesPosteriorCache.load(path)

Command line (the model's shape and flags come from the args.json the driver writes beside its checkpoints):

    python -m svgp_vae_amd.animate --checkpoint RUN/model_<k>.pt (--sprites_data_path DIR | --synthetic | --cache F)
        --characters 0 1 --N_context 36 [--actions A ..] [--sample --seed S] [--save_cache F] --out frames.npy

The posterior comes from exactly one place: a data source, whose train set the cache is built from (--sprites_data_path, or
--synthetic: the synthetic data of the run, regenerated from its args.json), or --cache, a file written by --save_cache; the test
characters are then read from the run's own data (args.json).
"""
import argparse
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

from ._lib import PosteriorRowsCfg, call, load_library

_F64 = torch.float64
CLIP_PV = (1e-4, 100.0)          # SVGPVAE_model.py:1180
NET_ROWS = 128                   # frames per network launch chain of an engine the cache builds itself
_SHAPE_KEYS = ("L", "L_action", "L_character", "m", "n_act", "K_SE", "normalize", "jitter", "N_train", "clip_qs", "net_dtype")
_FILE_KEYS = ("w", "X", "theta", "shape")


def param_shapes(shape):
    """name -> shape of the flat parameter vector, in SpritesStepEngine.shapes order."""
    from .sprites import sprites_param_shapes
    L, La, Lc = shape["L"], shape["L_action"], shape["L_character"]
    out = dict(sprites_param_shapes(L, Lc))
    out.update(inducing_index_points=(shape["m"], La + Lc), GPLVM_action=(shape["n_act"], La), se=(4,))
    return out


def theta_length(shape):
    return sum(int(np.prod(s)) for s in param_shapes(shape).values())


def _clean_shape(shape):
    if not isinstance(shape, dict) or any(k not in shape for k in _SHAPE_KEYS):
        raise ValueError(f"the shape of a SPRITES posterior cache needs the fields {', '.join(_SHAPE_KEYS)}")
    out = {k: int(shape[k]) for k in ("L", "L_action", "L_character", "m", "n_act")}
    out.update({k: bool(shape[k]) for k in ("K_SE", "normalize", "clip_qs")})
    out.update(jitter=float(shape["jitter"]), N_train=float(shape["N_train"]), net_dtype=str(shape["net_dtype"]))
    if out["net_dtype"] not in ("float64", "float32"):
        raise ValueError(f"net_dtype must be float64 or float32, got {out['net_dtype']}")
    if min(out[k] for k in ("L", "L_action", "L_character", "m", "n_act")) < 1:
        raise ValueError(f"bad shape {out}")
    return out


class SpritesPosteriorCache:
    """w (L, m), X = Sigma^-1 - K_mm^-1 (L, m, m), the flat parameter vector `theta` (SpritesStepEngine.shapes order) and the
    shape fields: the whole deployed model.  Holds tensors only; the forward-only engine for the three networks is built from
    `theta` at the first `animate` (property `engine`), unless `build` hands over the engine it walked the train set with."""

    def __init__(self, shape, theta, w, X, device="cuda:0", engine=None):
        self.shape = _clean_shape(shape)
        self.device = torch.device(device)
        L, m = self.shape["L"], self.shape["m"]
        self.theta = torch.as_tensor(theta, dtype=_F64).reshape(-1).to(self.device).contiguous()
        need = theta_length(self.shape)
        if self.theta.numel() != need:
            raise ValueError(f"theta has {self.theta.numel()} elements, the shape {self.shape} needs {need}")
        self.w = torch.as_tensor(w, dtype=_F64).to(self.device).contiguous()
        self.X = torch.as_tensor(X, dtype=_F64).to(self.device).contiguous()
        if tuple(self.w.shape) != (L, m) or tuple(self.X.shape) != (L, m, m):
            raise ValueError(f"w {tuple(self.w.shape)} / X {tuple(self.X.shape)} do not fit L={L}, m={m}: ({L}, {m}) / ({L}, {m}, {m})")
        self._engine = engine

    def params(self):
        """name -> view of theta."""
        out, off = {}, 0
        for k, s in param_shapes(self.shape).items():
            n = int(np.prod(s))
            out[k] = self.theta[off:off + n].view(s)
            off += n
        return out

    @property
    def engine(self):
        if self._engine is None:
            self._engine = engine_from_theta(self.shape, self.theta, b_max=NET_ROWS, device=self.device)
        return self._engine

    # ------------------------------------------------------------------ build
    @classmethod
    def build(cls, vae, repr_nn, svgp, train_frames, train_action_ids, frames_per_character=50, chunk=500, clip_qs=True,
              engine=None):
        """Walks the train rows once, `chunk` rows (whole character groups; the last chunk may be shorter) at a time:
        batching_encode_SVGPVAE per chunk, then precompute_GP_params_SVGPVAE (float32 streaming statistics, float64 inverse, no
        jitter) and the jitter-free K_mm^-1 of general_inverse.  X = Sigma^-1 - K_mm^-1 is formed here and nowhere else.
        `engine`: the SpritesStepEngine that owns the parameters (default: the one attached to the model objects)."""
        from . import sprites as S
        train_frames, train_action_ids = torch.as_tensor(train_frames), torch.as_tensor(train_action_ids)
        fpc, chunk, N = int(frames_per_character), int(chunk), int(train_frames.shape[0])
        if fpc < 1 or chunk < fpc or chunk % fpc:
            raise ValueError(f"chunk ({chunk}) must be a positive multiple of frames_per_character ({fpc})")
        if N < fpc or N % fpc or int(train_action_ids.shape[0]) != N:
            raise ValueError(f"{N} train frames / {int(train_action_ids.shape[0])} action ids: need the same number, a multiple "
                             f"of frames_per_character ({fpc})")
        eng = S._engine_of(svgp, vae, repr_nn, engine, min(chunk, N), clip_qs)
        if eng.clip_qs != bool(clip_qs):
            raise ValueError(f"clip_qs={bool(clip_qs)} but the engine was built with clip_qs={eng.clip_qs}")
        mu, var, aux = [], [], []
        for lo in range(0, N, chunk):
            n = min(chunk, N - lo)
            seg, rep = S.aux_data_sprites_utils(n, fpc, fpc)
            m_, v_, a_ = S.batching_encode_SVGPVAE((train_frames[lo:lo + n], train_action_ids[lo:lo + n]), vae,
                                                   clipping_qs=clip_qs, repr_nn=repr_nn, segment_ids=seg, repeats=rep, svgp=svgp,
                                                   engine=eng)
            mu.append(m_); var.append(v_); aux.append(a_)
        mu, var, aux = torch.cat(mu), torch.cat(var), torch.cat(aux)
        w, Si = S.precompute_GP_params_SVGPVAE(mu, var, aux, svgp, engine=eng)
        K_mm, _, _ = eng.kernel_matrices(aux[:1])
        X = (Si - S.general_inverse(K_mm)[None]).contiguous()
        shape = dict(L=eng.L, L_action=eng.La, L_character=eng.Lc, m=eng.m, n_act=eng.n_act, K_SE=svgp.K_SE,
                     normalize=svgp.K_obj_normalize, jitter=svgp.jitter, N_train=svgp.N_train, clip_qs=bool(clip_qs),
                     net_dtype="float32" if eng.f32 else "float64")
        eng.stream.synchronize()
        return cls(shape, eng.theta.clone(), w, X, device=eng.dev, engine=eng)

    # ------------------------------------------------------------------ files
    def save(self, path):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        torch.save({"w": self.w.cpu(), "X": self.X.cpu(), "theta": self.theta.cpu(), "shape": dict(self.shape)}, path)

    @classmethod
    def load(cls, path, device="cuda:0"):
        ck = torch.load(path, map_location="cpu")
        if not isinstance(ck, dict) or any(k not in ck for k in _FILE_KEYS) or \
                not all(torch.is_tensor(ck[k]) for k in ("w", "X", "theta")):
            raise ValueError(f"{path}: not a SPRITES posterior cache file (needs {', '.join(_FILE_KEYS)})")
        try:
            return cls(ck["shape"], ck["theta"], ck["w"], ck["X"], device=device)
        except ValueError as e:
            raise ValueError(f"{path}: {e}") from None


def engine_from_theta(shape, theta, b_max=NET_ROWS, device="cuda:0"):
    """A forward-only SpritesStepEngine whose parameters are the flat vector `theta` of a run with these shape fields."""
    from . import sprites as S
    shape = _clean_shape(shape)
    theta = torch.as_tensor(theta, dtype=_F64).reshape(-1)
    need = theta_length(shape)
    if theta.numel() != need:
        raise ValueError(f"theta has {theta.numel()} elements, the shape {shape} needs {need}")
    params, off = {}, 0
    for k, s in param_shapes(shape).items():
        n = int(np.prod(s))
        params[k] = theta[off:off + n].view(s).cpu()
        off += n
    L, La, Lc = shape["L"], shape["L_action"], shape["L_character"]
    vae, rnn = S.spritesVAE(L), S.sprites_representation_network(Lc)
    svgp = S.spritesSVGP(False, True, params["inducing_index_points"].numpy(), "main", shape["jitter"], shape["N_train"], La,
                         params["GPLVM_action"].numpy(), Lc, L, fixed_GP_params=True, fixed_GPLVM=True,
                         K_obj_normalize=shape["normalize"], K_SE=shape["K_SE"])
    eng = S.SpritesStepEngine(vae, rnn, svgp, b_max=b_max, seg_len=1, clip_qs=shape["clip_qs"], params=params, device=device,
                              net_dtype=torch.float32 if shape["net_dtype"] == "float32" else torch.float64)
    S._attach(eng, svgp, vae, rnn)
    eng.models = SimpleNamespace(vae=vae, repr_nn=rnn, svgp=svgp)
    return eng


def _target_actions(target_actions, n_act):
    t = torch.as_tensor(np.asarray(target_actions.cpu() if torch.is_tensor(target_actions) else target_actions))
    if t.dim() != 2 or t.numel() == 0:
        raise ValueError(f"target_actions must be (C, T) with C, T >= 1, got {tuple(t.shape)}")
    t64 = t.to(_F64)
    if not bool((torch.isfinite(t64) & (t64 == t64.floor()) & (t64 >= 0) & (t64 < n_act)).all()):
        raise ValueError(f"target_actions must hold integers in [0, {n_act})")
    return t64


def animate(cache, context_frames, target_actions, eps=None, return_moments=False):
    """Frames (C, T, 64, 64, 3) of C characters in the actions target_actions (C, T), each character given by its context frames
    context_frames (C, n_ctx, 64, 64, 3), n_ctx >= 1: the character vector is the mean of the representation network over them.
    decode(p_m + eps sqrt(clamp(p_v, 1e-4, 100))); eps (C T, L) None: the decode of the posterior mean.  return_moments:
    (frames, p_m, p_v), the moments (C T, L) with p_v clamped."""
    from . import sprites as S
    sh = cache.shape
    cf = torch.as_tensor(context_frames)
    if cf.dim() != 5 or tuple(cf.shape[2:]) != (64, 64, 3) or cf.shape[0] < 1 or cf.shape[1] < 1:
        raise ValueError(f"context_frames must be (C, n_ctx, 64, 64, 3) with C, n_ctx >= 1, got {tuple(cf.shape)}")
    Cn, n_ctx = int(cf.shape[0]), int(cf.shape[1])
    act = _target_actions(target_actions, sh["n_act"])
    if act.shape[0] != Cn:
        raise ValueError(f"target_actions has {act.shape[0]} rows, context_frames {Cn} characters")
    T, b, L, m = int(act.shape[1]), Cn * int(act.shape[1]), sh["L"], sh["m"]
    eng = cache.engine
    dev = eng.dev
    d_eps = None
    if eps is not None:
        d_eps = torch.as_tensor(eps, dtype=_F64).to(dev).contiguous()
        if tuple(d_eps.shape) != (b, L):
            raise ValueError(f"eps must be ({b}, {L}), got {tuple(d_eps.shape)}")
    cv = eng.character_vectors(cf.reshape(Cn * n_ctx, 64, 64, 3).to(dev, _F64))
    cv = S._segment_mean_repeat(cv, np.repeat(np.arange(Cn), n_ctx), [T] * Cn)
    aux = torch.cat([act.reshape(-1, 1).to(dev), cv], dim=1).contiguous()
    _, Kb, kbb = eng.kernel_matrices(aux)
    p_m, p_v, z = (torch.empty(b, L, dtype=_F64, device=dev) for _ in range(3))
    cfg = PosteriorRowsCfg(b=b, m=m, L=L, clip_lo=CLIP_PV[0], clip_hi=CLIP_PV[1])
    w, X = cache.w.to(dev), cache.X.to(dev)
    n_work = int(load_library().svgp_sprites_posterior_rows_workspace_elems(C.byref(cfg)))       # 0 up to m = 256
    work = torch.empty(n_work, dtype=_F64, device=dev) if n_work else None
    eng.stream.wait_stream(torch.cuda.current_stream(dev))
    call("svgp_sprites_posterior_rows", C.byref(cfg), Kb.data_ptr(), kbb.data_ptr(), w.data_ptr(), X.data_ptr(),
         None if d_eps is None else d_eps.data_ptr(), p_m.data_ptr(), p_v.data_ptr(), z.data_ptr(),
         None if work is None else work.data_ptr(), eng.stream.cuda_stream)
    frames = eng.decode(z).view(Cn, T, 64, 64, 3)
    return (frames, p_m, p_v) if return_moments else frames


def route(cache_or_shape, rows=1):
    """The kernels of the GP stage of one `animate` call of `rows` target rows, in launch order
    (svgp_sprites_posterior_rows_route: one launch up to m = 256, two beyond); needs no device."""
    sh = cache_or_shape.shape if isinstance(getattr(cache_or_shape, "shape", None), dict) else cache_or_shape
    buf = C.create_string_buffer(256)
    call("svgp_sprites_posterior_rows_route", C.byref(PosteriorRowsCfg(b=int(rows), m=int(sh["m"]), L=int(sh["L"]),
                                                                       clip_lo=CLIP_PV[0], clip_hi=CLIP_PV[1])), buf, len(buf))
    return buf.value.decode().split()


# ---------------------------------------------------------------------------------------------- command line
def run_args_of(checkpoint_path):
    with open(os.path.join(os.path.dirname(os.path.abspath(checkpoint_path)), "args.json")) as f:
        return json.load(f)


def shape_from_run(a, N_train):
    """The shape fields of the model a SPRITES_experiment run with the flags `a` (its args.json) trained; keep in step with
    run_experiment_sprites_SVGPVAE (the checkpoint format carries no shapes)."""
    if "SVGPVAE" not in str(a.get("elbo")):
        raise ValueError(f"args.json: --elbo {a.get('elbo')} is not an SVGPVAE run")
    return dict(L=int(a["L"]), L_action=int(a["L_action"]), L_character=int(a["L_character"]), m=int(a["N_actions"]) * int(a["m"]),
                n_act=int(a["N_actions"]), K_SE=bool(a.get("K_SE")), normalize=bool(a.get("object_kernel_normalize")),
                jitter=float(a["jitter"]), N_train=float(N_train), clip_qs=bool(a.get("clip_qs")), net_dtype="float64")


def theta_from_run(checkpoint_path, shape):
    """The checkpoint's flat parameter vector; a length that does not fit the shape fields is refused with both numbers."""
    ck = torch.load(checkpoint_path, map_location="cpu")
    if not isinstance(ck, dict) or "theta" not in ck:
        raise ValueError(f"{checkpoint_path}: not a checkpoint of the SPRITES driver (needs theta)")
    theta = torch.as_tensor(ck["theta"], dtype=_F64).reshape(-1).contiguous()
    need = theta_length(shape)
    if theta.numel() != need:
        raise ValueError(f"{checkpoint_path}: theta has {theta.numel()} elements but the run's args.json describes a model of "
                         f"{need} (another --L / --m / --N_actions / --L_action / --L_character?)")
    return theta


def load_run_data(a, sprites_data_path=None, need_train=True):
    """(train, test) dicts (frames, char_IDs, action_IDs) of the run's data: `sprites_data_path` if given, else the run's own (its
    synthetic spec or its path).  need_train False: train is None, and of a data directory only test_character.npz is read."""
    from .SPRITES_experiment import N_FRAMES_PER_CHARACTER_TRAIN, _load
    ns = SimpleNamespace(synthetic=None if sprites_data_path else a.get("synthetic"),
                         sprites_data_path=sprites_data_path or a.get("sprites_data_path"), seed=int(a.get("seed", 0)),
                         frames_per_character=int(a.get("frames_per_character", N_FRAMES_PER_CHARACTER_TRAIN)),
                         N_actions=int(a.get("N_actions", 72)))
    if need_train or ns.synthetic:
        train, test = _load(ns)
        return (train if need_train else None), test
    f = os.path.join(ns.sprites_data_path, "test_character.npz")
    if not os.path.exists(f):
        raise FileNotFoundError(f"{f}: expected npz with frames (N,64,64,3), char_IDs (N), action_IDs (N)")
    d = np.load(f)
    return None, {k: d[k] for k in ("frames", "char_IDs", "action_IDs")}


def cache_from_run(checkpoint_path, train, a=None, chunk=500, device="cuda:0"):
    """The posterior cache of the model in `checkpoint_path` over the train set `train` (dict frames, action_IDs)."""
    from .SPRITES_experiment import N_FRAMES_PER_CHARACTER_TRAIN
    a = a or run_args_of(checkpoint_path)
    shape = shape_from_run(a, len(train["frames"]))
    theta = theta_from_run(checkpoint_path, shape)
    fpc = int(a.get("frames_per_character", N_FRAMES_PER_CHARACTER_TRAIN))
    chunk = max(fpc, int(chunk) // fpc * fpc)
    eng = engine_from_theta(shape, theta, b_max=min(chunk, len(train["frames"])), device=device)
    t64 = lambda x: torch.as_tensor(np.asarray(x), dtype=_F64)
    return SpritesPosteriorCache.build(eng.models.vae, eng.models.repr_nn, eng.models.svgp, t64(train["frames"]),
                                       t64(train["action_IDs"]), frames_per_character=fpc, chunk=chunk, clip_qs=shape["clip_qs"],
                                       engine=eng)


def build_parser():
    p = argparse.ArgumentParser(description="Frames of test characters in unseen actions from a trained SPRITES SVGP-VAE checkpoint.")
    p.add_argument("--checkpoint", required=True, help="RUN/model_<k>.pt of SPRITES_experiment --save --save_model_weights")
    src = p.add_mutually_exclusive_group()
    src.add_argument("--sprites_data_path", type=str, default=None, help="directory with train.npz and test_character.npz")
    src.add_argument("--synthetic", action="store_true", help="the run's own synthetic data, regenerated from its args.json")
    src.add_argument("--cache", type=str, default=None, help="posterior cache file of --save_cache instead of a train set; the test "
                                                              "characters are read from the run's own data (args.json)")
    p.add_argument("--save_cache", type=str, default=None, help="write the posterior cache built from the data source here")
    p.add_argument("--characters", type=int, nargs="+", required=True, help="indices of test characters")
    p.add_argument("--N_context", type=int, default=36, help="the first N_context actions of a character are its context")
    p.add_argument("--actions", type=int, nargs="+", default=None, help="target actions; default: the remaining ones")
    p.add_argument("--sample", action="store_true", help="z = p_m + eps sqrt(p_v) with eps from --seed; default: the posterior mean")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--chunk", type=int, default=500, help="train rows per step of the cache build")
    p.add_argument("--out", required=True)
    return p


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if args.cache is None and args.sprites_data_path is None and not args.synthetic:
        p.error("give a data source (--sprites_data_path DIR or --synthetic) to build the posterior cache from, or --cache F")
    if args.cache is not None and args.save_cache is not None:
        p.error("--save_cache writes the cache built from a data source; it cannot be combined with --cache")
    return args


def main(argv=None):
    args = parse_args(argv)
    a = run_args_of(args.checkpoint)
    if args.synthetic and not a.get("synthetic"):
        raise SystemExit("--synthetic: the run's args.json has no synthetic spec; use --sprites_data_path")
    train, test = load_run_data(a, args.sprites_data_path, need_train=args.cache is None)
    na = int(a.get("N_actions", 72))
    n_char = len(test["frames"]) // na
    if not 0 < args.N_context < na:
        raise SystemExit(f"--N_context must be in (0, {na})")
    if any(c < 0 or c >= n_char for c in args.characters):
        raise SystemExit(f"--characters: the data has {n_char} test characters")
    if args.cache is not None:
        cache = SpritesPosteriorCache.load(args.cache)
        theta = theta_from_run(args.checkpoint, cache.shape)
        if not torch.equal(theta, cache.theta.cpu()):
            raise SystemExit(f"{args.cache} was built for other parameters than {args.checkpoint}")
    else:
        cache = cache_from_run(args.checkpoint, train, a, chunk=args.chunk)
        if args.save_cache:
            cache.save(args.save_cache)
    fr = np.asarray(test["frames"], dtype=np.float64).reshape(n_char, na, 64, 64, 3)
    ids = np.asarray(test["action_IDs"]).reshape(n_char, na)
    ctx = fr[args.characters, :args.N_context]
    tgt = ids[args.characters, args.N_context:] if args.actions is None else np.tile(np.asarray(args.actions), (len(args.characters), 1))
    eps = np.random.RandomState(args.seed).randn(tgt.size, cache.shape["L"]) if args.sample else None
    out = animate(cache, ctx, tgt, eps=eps)
    np.save(args.out, out.cpu().numpy())
    print(f"{len(args.characters)} characters x {tgt.shape[1]} actions -> {args.out}   route: {' '.join(route(cache, rows=tgt.size))}")
    return out


if __name__ == "__main__":
    main()
