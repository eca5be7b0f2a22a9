"""The rotated-MNIST data set generator (svgp_vae_amd.utils.generate_rotated_MNIST, reference utils.py:507-657) without a GPU:
the host part (sampling, PCA, row order, splits, drop, file names) against a run of the REFERENCE ITSELF, recorded by
tests/golden/make_ref_rotated_mnist_fixture.py as tests/golden/ref_rotated_mnist.npz.  The rotations go through the `rotate=` seam
to scipy.ndimage.rotate, the function the reference calls, so images and row sums are equal to the bit; the device kernel that
is the default is tested in tests/test_gpu_rotated_mnist.py.  Also: the drivers' loader and the Casale mask read what the
generator writes, and the entry point refuses bad arguments before any launch."""
import ctypes as C
import importlib
import os
import pickle

import numpy as np
import pytest
from scipy import ndimage

import svgp_vae_amd
from svgp_vae_amd import _lib
from svgp_vae_amd.utils import generate_rotated_MNIST, import_rotated_mnist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = importlib.import_module("tests.golden.make_ref_rotated_mnist_fixture")
MODES = [("shuffled", True), ("not_shuffled", False)]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_rotated_mnist.npz"))


def scipy_rotate(images, angles_deg):
    """The reference's own call (utils.py:571), image-major and angle-minor."""
    return np.stack([np.stack([ndimage.rotate(im, a, reshape=False) for a in angles_deg]) for im in images])


def _generate(fx, d, shuffle, **kw):
    np.random.seed(GEN.NP_SEED)                 # sklearn's randomized PCA draws from numpy's global generator: pinned like the fixture's run
    return generate_rotated_MNIST(str(d) + "/", shuffle_data=shuffle, mnist=(fx["x_train"], fx["y_train"]), rotate=scipy_rotate,
                                  **GEN.RUN, **kw)


def _load(path):
    with open(path, "rb") as f:
        return pickle.load(f)


@pytest.mark.parametrize("mode,shuffle", MODES, ids=[m for m, _ in MODES])
def test_generator_reproduces_the_reference_run(fx, tmp_path, capsys, mode, shuffle):
    paths = _generate(fx, tmp_path, shuffle)
    assert sorted(os.listdir(tmp_path)) == fx[mode + "_files"].tolist()                       # the reference's names
    assert sorted(os.path.basename(p) for p in paths.values()) == fx[mode + "_files"].tolist()
    splits = ["train", "eval", "test"] + ([] if shuffle else ["train_not_in_test"])
    assert set(paths) == set(splits) | {"pca"}
    assert np.array_equal(_load(paths["pca"]), fx[mode + "_pca"])
    for split in splits:
        d = _load(paths[split])
        want_aux = fx[f"{mode}_{split}_aux"]
        assert d["images"].dtype == np.float64 and d["aux_data"].dtype == np.float64
        assert d["images"].shape == tuple(fx[f"{mode}_{split}_shape"]) and d["images"].shape[1:] == (28, 28, 1)
        assert d["aux_data"].shape == want_aux.shape
        assert np.array_equal(d["aux_data"][:, :2], want_aux[:, :2])                          # ids, angles, row order
        assert np.array_equal(d["aux_data"][:, 2:], want_aux[:, 2:])                          # PCA columns
        assert np.array_equal(d["images"].reshape(len(want_aux), -1).sum(1), fx[f"{mode}_{split}_sums"])
    assert np.array_equal(_load(paths["test"])["images"], fx[mode + "_test_images"])
    # unclipped: the cubic spline overshoots [0, 1] and the generator leaves it so
    assert _load(paths["train"])["images"].min() < 0 and _load(paths["train"])["images"].max() > 1
    out = capsys.readouterr().out
    n = {s: len(fx[f"{mode}_{s}_aux"]) for s in splits}
    assert (n["train"], n["eval"], n["test"]) == ((243, 40, 15) if shuffle else (241, 40, 16))
    for line in ("Number of images with digit 3: 20", "Number of images with digit 6: 20", "Explained variance ratio PCA: [",
                 "Test angle: ", f"Size of training data: {n['train']}", f"Size of validation data: {n['eval']}",
                 f"Size of test data: {n['test']}", "36_4.p" if shuffle else "36_not_shuffled_4.p"):
        assert line in out, line
    assert ("Size of training data without test ids: 81" in out) == (not shuffle)


def test_driver_names_load_through_the_drivers_loader(fx, tmp_path):
    paths = _generate(fx, tmp_path, True, driver_names=True)
    assert sorted(os.listdir(tmp_path)) == ["eval_data36.p", "pca_ov_init36.p", "test_data36.p", "train_data36.p"]
    train, ev, te, train_batches = import_rotated_mnist(str(tmp_path) + "/", "36.p", 100)
    assert (len(train["images"]), len(ev["images"]), len(te["images"])) == (243, 40, 15)
    assert train_batches == [(0, 100), (100, 200), (200, 243)]
    assert np.array_equal(train["aux_data"], fx["shuffled_train_aux"]) and np.array_equal(te["images"], fx["shuffled_test_images"])
    assert _load(paths["pca"]).shape == (24, 4)              # MNIST_experiment.py --PCA --ov_joint reads pca_ov_init<dataset>.p
    # same content under either naming
    other = tmp_path / "ref_names"
    other.mkdir()
    ref_paths = _generate(fx, other, True)
    for k in paths:
        a, b = _load(paths[k]), _load(ref_paths[k])
        assert np.array_equal(a, b) if k == "pca" else all(np.array_equal(a[f], b[f]) for f in ("images", "aux_data")), k


def test_casale_train_angles_mask_selects_the_train_pairs(fx, tmp_path):
    from svgp_vae_amd.GPVAE_Casale_model import train_angles_mask
    paths = _generate(fx, tmp_path, True, driver_names=True)
    train_angles_mask(paths["train"], str(tmp_path / "mask.p"))
    mask = _load(tmp_path / "mask.p")
    aux = _load(paths["train"])["aux_data"]
    assert mask.dtype == bool and mask.shape == (len(np.unique(aux[:, 0])) * len(np.unique(aux[:, 1])),)
    assert int(mask.sum()) == len(aux) == 243


def test_missing_digits_raise_an_error_that_names_the_argument(tmp_path):
    with pytest.raises(ValueError, match="mnist="):
        generate_rotated_MNIST(str(tmp_path) + "/", N=2, rotate=scipy_rotate)
    assert os.listdir(tmp_path) == []


def test_rotate_entry_point_validates_its_arguments():
    """Shape and pointer checks of svgp_rotate_cubic_f64 happen before any device call (no GPU in this test)."""
    fake = C.c_void_p(4096)                                     # never dereferenced: every case fails validation first
    for H, W, message in ((65, 28, "65 x 28"), (28, 1, "28 x 1"), (1, 28, "1 x 28"), (28, 65, "28 x 65")):
        with pytest.raises(svgp_vae_amd.SvgpError, match=message + ".*2 <= H, W <= 64"):
            _lib.call("svgp_rotate_cubic_f64", 3, H, W, 16, fake, fake, fake, None)
    with pytest.raises(svgp_vae_amd.SvgpError, match="A=0"):
        _lib.call("svgp_rotate_cubic_f64", 3, 28, 28, 0, fake, fake, fake, None)
    with pytest.raises(svgp_vae_amd.SvgpError, match="n=-1"):
        _lib.call("svgp_rotate_cubic_f64", -1, 28, 28, 16, fake, fake, fake, None)
    for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        with pytest.raises(svgp_vae_amd.SvgpError, match="NULL device pointer"):
            _lib.call("svgp_rotate_cubic_f64", 3, 28, 28, 16, *args, None)
    _lib.call("svgp_rotate_cubic_f64", 0, 28, 28, 16, None, None, None, None)      # n = 0: nothing to do, OK


def test_rotate_images_refuses_to_run_without_a_gpu(monkeypatch):
    import torch
    from svgp_vae_amd.utils import rotate_images
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(svgp_vae_amd.SvgpError, match="no CPU execution path"):
        rotate_images(np.zeros((1, 28, 28)), [0.0])
