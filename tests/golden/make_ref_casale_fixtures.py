"""Generator of tests/golden/ref_casale_small.npz (build container only; needs the reference checkout): executes the
REFERENCE'S OWN GPVAE_Casale_model.py -- casaleGP.V_matrix, taylor_coeff, forward_pass_Casale, predict_test_set_Casale,
sort_train_data, train_angles_mask -- as written, on the functional TensorFlow stand-in of make_ref_model_fixtures.py (imported,
not edited), extended here by the ops that module lacks.  Gradients come from torch autograd through the reference's forward
code.  Only numeric arrays are written; nothing of the reference's source is stored or shipped.

    python tests/golden/make_ref_casale_fixtures.py
"""
import importlib
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_ref_model_fixtures as S  # noqa: E402
from tests import casale_cases as CC  # noqa: E402

tf, DT = S.tf, S.DT
_QUEUE = []                                 # the N(0,1) draws, in call order


def _normal(shape, dtype=None, **kw):
    e = _QUEUE.pop(0)
    assert tuple(e.shape) == tuple(int(s) for s in shape)
    return e


def _extend_stand_in():
    as_int = lambda n: int(n.item()) if isinstance(n, torch.Tensor) else int(n)
    tf.eye = lambda n, dtype=None: torch.eye(as_int(n), dtype=S._dtype(dtype))
    tf.boolean_mask = lambda x, mask: x[torch.as_tensor(np.asarray(mask, dtype=bool))]
    tf.diag_part = lambda x: torch.diagonal(x, dim1=-2, dim2=-1)
    tf.linalg.matmul = S._matmul
    tf.sort = lambda x: torch.sort(x).values
    tf.squeeze = lambda x: (torch.stack([S._t(v) for v in x]) if isinstance(x, (list, tuple)) else x).squeeze()
    tf.tile = lambda x, reps: x.repeat(*[int(r) for r in reps])
    tf.unique = lambda x: types.SimpleNamespace(y=torch.unique(x))          # only sort(unique(.).y) is used
    tf.random = types.SimpleNamespace(normal=_normal)
    # tf.shape(a)[0] * tf.shape(b)[0] and tf.cast(tf.shape(V)[0], ...) work on the tuples tf.shape returns
    tf.reshape = lambda x, shape: x.reshape(tuple(as_int(s) for s in shape))


def _import_reference():
    torch.Tensor.get_shape = lambda self: tuple(self.shape)          # (generator process only)
    sys.modules["tensorflow"], sys.modules["tensorflow_probability"] = tf, S.tfp
    sys.path.insert(0, S.REF)
    for name in ("VAE_utils", "GPVAE_Casale_model"):
        sys.modules.pop(name, None)
    return importlib.import_module("GPVAE_Casale_model"), importlib.import_module("VAE_utils")


ORDER = ["enc_c1_w", "enc_c1_b", "enc_c2_w", "enc_c2_b", "enc_c3_w", "enc_c3_b", "enc_d_w", "enc_d_b",
         "dec_d_w", "dec_d_b", "dec_c1_w", "dec_c1_b", "dec_c2_w", "dec_c2_b", "dec_c3_w", "dec_c3_b"]


def main():
    _extend_stand_in()
    RC, RV = _import_reference()
    gin = np.load(os.path.join(HERE, "mnist_cfg2_inputs.npz"))
    out = {}
    for normalize in (False, True):
        tag = "norm" if normalize else "raw"
        prob = CC.fixture_problem(gin, normalize)
        p, L = prob["params"], prob["L"]
        S.VARIABLES.clear()
        vae = RV.mnistVAE(L=L)
        vae.dtype = np.float64
        leaves = {}
        layers = [l for l in vae.encoder.layers + vae.decoder.layers if hasattr(l, "kernel")]
        for l, (kw, kb) in zip(layers, zip(ORDER[0::2], ORDER[1::2])):
            l.kernel, l.bias = p[kw].clone().requires_grad_(True), p[kb].clone().requires_grad_(True)
            leaves[kw], leaves[kb] = l.kernel, l.bias
        GP = RC.casaleGP(fixed_gp_params=False, object_vectors_init=p["object_vectors"].numpy(),
                         object_kernel_normalize=normalize, ov_joint=True)
        with torch.no_grad():       # in place: the kernel object holds these tensors
            GP.l_GP.fill_(float(p["l_GP"])); GP.amplitude.fill_(float(p["amplitude"])); GP.alpha.fill_(float(p["alpha"]))
        leaves.update(l_GP=GP.l_GP, amplitude=GP.amplitude, alpha=GP.alpha, object_vectors=GP.object_vectors)
        aux, images, lo, hi = CC.t64(prob["aux"]), prob["images"], prob["lo"], prob["hi"]
        _QUEUE[:] = [prob["eps_f"], prob["eps_b"]]
        Z = RC.encode(images, vae=vae, clipping_qs=True)
        V = GP.V_matrix(aux, train_ids_mask=prob["case"]["mask"])
        a, B, c = GP.taylor_coeff(Z=Z, V=V)
        tup = RC.forward_pass_Casale((images[lo:hi], aux[lo:hi]), vae=vae, a=a, B=B, c=c, V=V, beta=prob["beta"], GP=GP,
                                     clipping_qs=True)
        names = list(leaves)
        grads = torch.autograd.grad(tup[0], [leaves[k] for k in names], retain_graph=True)
        for k, v in zip(("V", "a", "B", "c", "Z"), (V, a, B, c, Z)):
            out[f"{tag}.{k}"] = v.detach().numpy()
        for k, v in zip(("elbo", "recon_loss", "GP_prior_term", "log_var", "qnet_mu", "qnet_var", "recon_images"), tup):
            out[f"{tag}.fwd.{k}"] = v.detach().numpy()
        for k, g in zip(names, grads):
            out[f"{tag}.grad.{k}"] = g.detach().numpy()
        for take_mean in (True, False):
            _QUEUE[:] = [prob["eps_t"]]
            rec, loss = RC.predict_test_set_Casale(prob["test_images"], prob["test_aux"], aux, vae, GP, V, Z, take_mean=take_mean)
            out[f"{tag}.predict.{'mean' if take_mean else 'sample'}.recon"] = rec.detach().numpy()
            out[f"{tag}.predict.{'mean' if take_mean else 'sample'}.loss"] = loss.detach().numpy()

    # host helpers on a shuffled copy of the 4050 real train rows (sort_train_data needs exactly 4050 rows per digit)
    rows = gin["train_aux"]
    perm = np.random.RandomState(5).permutation(len(rows))
    shuffled = rows[perm]
    srt = RC.sort_train_data(dict(images=np.arange(len(rows), dtype=np.float64), aux_data=shuffled.copy()), dataset="3")
    out["sort.order"] = srt["images"].astype(np.int32)                  # position in the shuffled input of every sorted row
    out["sort.id_column"] = srt["aux_data"][:, 0].astype(np.int32)
    assert np.array_equal(srt["aux_data"][:, 1:], shuffled[out["sort.order"]])
    with tempfile.TemporaryDirectory() as d:
        pickle.dump(dict(aux_data=shuffled), open(os.path.join(d, "t.p"), "wb"))
        RC.train_angles_mask(os.path.join(d, "t.p"), os.path.join(d, "m.p"))
        out["mask"] = np.asarray(pickle.load(open(os.path.join(d, "m.p"), "rb")), dtype=bool)
    path = os.path.join(HERE, "ref_casale_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
