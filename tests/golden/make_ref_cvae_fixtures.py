"""Generator of tests/golden/ref_cvae_small.npz (build container only; needs the reference checkout): executes the
REFERENCE'S OWN mnistCVAE (VAE_utils.py), forward_pass_standard_VAE_rotated_mnist and predict_CVAE (SVGPVAE_model.py) as
written, on the functional TensorFlow stand-in of make_ref_model_fixtures.py (imported, not edited), extended here by the ops
that module lacks.  Gradients come from torch autograd through the reference's forward code.  Only numeric arrays are written;
nothing of the reference's source is stored or shipped.

    python tests/golden/make_ref_cvae_fixtures.py

Problem: b = 6 train rows, L = 4, seeded glorot weights with non-zero biases, 4 test rows of which one has an id no train row
carries (the empty-group row of predict_CVAE: NaN), CVAE with and without clipping, and the plain VAE.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_ref_model_fixtures as S  # noqa: E402
from tests import cvae_cases as CC  # noqa: E402

tf, DT = S.tf, S.DT
_QUEUE = []                                 # the N(0,1) draws, in call order
ORDER = [n for n, _ in CC.param_shapes(4, True)]
B, L, T = 6, 4, 4


def _normal(shape, dtype=None, **kw):
    e = _QUEUE.pop(0)
    assert tuple(e.shape) == tuple(int(s) for s in shape)
    return e


def _repeat(x, repeats, axis=0):
    """tf.repeat with a python scalar as input (tf.repeat(w * h, b): b copies of w * h) or a tensor of per-element counts."""
    x = S._t(x, torch.int64) if not isinstance(x, torch.Tensor) else x
    r = torch.as_tensor(np.asarray(repeats.detach() if isinstance(repeats, torch.Tensor) else repeats), dtype=torch.int64)
    return torch.repeat_interleave(x.reshape(-1) if x.dim() == 0 else x, r, dim=axis)


def _extend_stand_in():
    tf.repeat = _repeat
    tf.boolean_mask = lambda x, mask: x[mask]
    tf.reduce_prod = lambda x: int(np.prod([int(v) for v in x]))
    tf.random = types.SimpleNamespace(normal=_normal)
    tf.reshape = lambda x, shape: x.reshape(tuple(int(s) for s in shape))


def _import_reference():
    torch.Tensor.get_shape = lambda self: tuple(self.shape)          # (generator process only)
    sys.modules["tensorflow"], sys.modules["tensorflow_probability"] = tf, S.tfp
    tf.__path__ = []
    for sub in ("tensorflow.python", "tensorflow.python.ops", "tensorflow.python.ops.math_ops"):
        sys.modules[sub] = types.ModuleType(sub)
    sys.modules["tensorflow.python"].ops = sys.modules["tensorflow.python.ops"]
    sys.modules["tensorflow.python.ops"].math_ops = sys.modules["tensorflow.python.ops.math_ops"]
    sys.path.insert(0, S.REF)
    for name in ("VAE_utils", "utils", "SVGPVAE_model"):
        sys.modules.pop(name, None)
    for stub in ("matplotlib", "matplotlib.pyplot", "pandas", "seaborn"):
        if stub not in sys.modules:
            try:
                importlib.import_module(stub)
            except Exception:
                sys.modules[stub] = types.ModuleType(stub)
    return importlib.import_module("SVGPVAE_model"), importlib.import_module("VAE_utils")


def problem(gin):
    """The fixture's inputs (also what tests/test_cvae_cases_cpu.py and tests/test_gpu_cvae.py rebuild from the stored arrays)."""
    rng = np.random.RandomState(91)
    out = {}
    for cvae in (True, False):
        p = CC.glorot_params(L, cvae, 9)
        p["enc_d_b"][L:] += np.array([-9.0, 0.3, 4.5, -0.2])
        out["cvae" if cvae else "vae"] = p
    ids = np.array([3.0, 5.0, 3.0, 8.0, 5.0, 3.0])
    aux = np.stack([ids, rng.uniform(0, 6.28, B)], 1)
    aux_test = np.stack([np.array([5.0, 3.0, 7.0, 8.0]), np.array([0.0, -0.3, 7.0, np.pi / 2])], 1)      # id 7: no train row
    return dict(params=out, images=gin["images"][:B], aux=aux, eps=rng.randn(B, L), images_test=gin["images"][100:100 + T],
                aux_test=aux_test, eps_predict=rng.randn(B, L))


def main():
    _extend_stand_in()
    RM, RV = _import_reference()
    gin = np.load(os.path.join(HERE, "mnist_cfg2_inputs.npz"))
    prob = problem(gin)
    out = {k: np.asarray(prob[k]) for k in ("images", "aux", "eps", "images_test", "aux_test", "eps_predict")}
    images, aux, eps = CC.t64(prob["images"]), CC.t64(prob["aux"]), CC.t64(prob["eps"])
    for tag, cvae, clip in (("cvae", True, False), ("cvae_clip", True, True), ("vae", False, False)):
        p = prob["params"]["cvae" if cvae else "vae"]
        S.VARIABLES.clear()
        vae = (RV.mnistCVAE if cvae else RV.mnistVAE)(L=L)
        seqs = [vae.encoder_first_part, vae.encoder_last_part, vae.decoder_first_part, vae.decoder_last_part] if cvae else \
            [vae.encoder, vae.decoder]
        layers = [l for s in seqs for l in s.layers if hasattr(l, "kernel")]
        leaves = {}
        for l, (kw, kb) in zip(layers, zip(ORDER[0::2], ORDER[1::2])):
            l.kernel, l.bias = CC.t64(p[kw]).clone().requires_grad_(True), CC.t64(p[kb]).clone().requires_grad_(True)
            leaves[kw], leaves[kb] = l.kernel, l.bias
            out[f"{tag}.param.{kw}"], out[f"{tag}.param.{kb}"] = p[kw], p[kb]
        assert len(layers) == 8
        _QUEUE[:] = [eps]
        tup = RM.forward_pass_standard_VAE_rotated_mnist((images, aux), vae, clipping_qs=clip, CVAE=cvae)
        names = list(leaves)
        grads = torch.autograd.grad(-tup[2], [leaves[k] for k in names])
        for k, v in zip(("recon_loss", "KL_term", "elbo", "recon", "qnet_mu", "qnet_var", "z"), tup):
            out[f"{tag}.fwd.{k}"] = v.detach().numpy()
        for k, g in zip(names, grads):
            out[f"{tag}.grad.{k}"] = g.detach().numpy()
        if cvae and not clip:
            _QUEUE[:] = [CC.t64(prob["eps_predict"])]
            aux_test = CC.t64(prob["aux_test"])
            rec, loss = RM.predict_CVAE(images, CC.t64(prob["images_test"]), aux, aux_test, vae, [float(v) for v in aux_test[:, 0]])
            out["cvae.predict.recon"], out["cvae.predict.loss"] = rec.detach().numpy(), loss.detach().numpy()
            assert np.isnan(out["cvae.predict.recon"][2]).all() and np.isfinite(out["cvae.predict.recon"][[0, 1, 3]]).all()
    path = os.path.join(HERE, "ref_cvae_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
