"""The rotation kernel of the rotated-MNIST data set generator (csrc/rotate.hip, svgp_rotate_cubic_f64) against
scipy.ndimage.rotate itself, the generator with the kernel as its `rotate` against the run of the reference recorded in
tests/golden/ref_rotated_mnist.npz, and a generated data set through the driver.

TOL = 1e-12 absolute, on pixel values of order 1, every pixel compared: two float64 orderings of the same sums differ by about
1e-14 here (the kernel's arithmetic run on the host against scipy: 3.3e-14 at 64 x 64, 9.3e-15 at 28 x 28); the bar leaves two
orders of magnitude above that for fused multiply-adds and sits ten orders below the effect of a wrong tap, weight or a border
pixel on the wrong side of the outside rule (the dense image's values are >= 0.2)."""
import importlib
import os
import pickle

import numpy as np
import pytest
import torch
from scipy import ndimage
from scipy.special import cosdg, sindg

from svgp_vae_amd import _lib
from svgp_vae_amd.utils import generate_rotated_MNIST, rotate_images

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = importlib.import_module("tests.golden.make_ref_rotated_mnist_fixture")
TOL = 1e-12
SHAPES = [(28, 28), (4, 4), (33, 20), (64, 64)]         # MNIST; every tap mirrors; non-square and odd; the ceiling
ANGLES = {"sixteenths": np.linspace(0, 360, 17)[:-1],    # the generator's set: the exact quarter turns are in it
          "fifths": np.linspace(0, 360, 6)[:-1],
          "odd": np.array([-33.3, 400.0, 1e-7])}


def _images(H, W):
    """Four sparse images and a dense one with non-zero borders (>= 0.2), where the outside rule shows."""
    rs = np.random.RandomState(1000 * H + W)
    x = rs.rand(5, H, W) * (rs.rand(5, H, W) < 0.25)
    x[4] = 0.2 + 0.8 * rs.rand(H, W)
    return x


@pytest.fixture(scope="module")
def scipy_reference():
    """{(H, W, angle set): (n, A, H, W)} from scipy.ndimage.rotate, once for the module."""
    return {(H, W, key): np.stack([np.stack([ndimage.rotate(im, a, reshape=False) for a in angles]) for im in _images(H, W)])
            for H, W in SHAPES for key, angles in ANGLES.items()}


@pytest.mark.parametrize("key", list(ANGLES))
@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_kernel_matches_scipy_rotate_on_every_pixel(scipy_reference, H, W, key):
    want = scipy_reference[(H, W, key)]
    got = rotate_images(_images(H, W), ANGLES[key])
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == want.shape == (5, len(ANGLES[key]), H, W)
    got = got.cpu().numpy()
    err = np.abs(got - want)
    print(f"{H}x{W} {key}: max |kernel - scipy| = {err.max():.3e}")
    assert err.max() < TOL, np.unravel_index(err.argmax(), err.shape)


def test_chunked_launches_equal_one_launch():
    x = _images(28, 28)
    a = rotate_images(x, ANGLES["fifths"], chunk=2)
    b = rotate_images(x, ANGLES["fifths"])
    assert torch.equal(a, b)


def test_no_images_is_ok_and_writes_nothing():
    out = torch.full((2, 3, 4, 4), 7.0, dtype=torch.float64, device="cuda")
    cs = torch.tensor(np.stack([cosdg(ANGLES["odd"]), sindg(ANGLES["odd"])], 1), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    _lib.call("svgp_rotate_cubic_f64", 0, 4, 4, 3, None, cs.data_ptr(), out.data_ptr(), s)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert tuple(rotate_images(np.zeros((0, 4, 4)), ANGLES["odd"]).shape) == (0, 3, 4, 4)


@pytest.mark.parametrize("mode,shuffle", [("shuffled", True), ("not_shuffled", False)], ids=["shuffled", "not_shuffled"])
def test_generator_on_the_device_reproduces_the_reference_run(tmp_path, mode, shuffle):
    """The default `rotate` (the kernel): the test split's images and the pixel sum of every row of every split."""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "ref_rotated_mnist.npz"))
    np.random.seed(GEN.NP_SEED)
    paths = generate_rotated_MNIST(str(tmp_path) + "/", shuffle_data=shuffle, mnist=(fx["x_train"], fx["y_train"]), **GEN.RUN)
    for split in ["train", "eval", "test"] + ([] if shuffle else ["train_not_in_test"]):
        with open(paths[split], "rb") as f:
            d = pickle.load(f)
        assert np.array_equal(d["aux_data"][:, :2], fx[f"{mode}_{split}_aux"][:, :2])
        assert d["images"].shape == tuple(fx[f"{mode}_{split}_shape"]) and d["images"].dtype == np.float64
        err = np.abs(d["images"].reshape(len(d["images"]), -1).sum(1) - fx[f"{mode}_{split}_sums"])
        print(f"{mode} {split}: max row-sum error {err.max():.3e}")
        assert err.max() < TOL * 28 * 28
        if split == "test":
            err = np.abs(d["images"] - fx[mode + "_test_images"])
            print(f"{mode} test images: max error {err.max():.3e}")
            assert err.max() < TOL


def test_generated_data_set_runs_through_the_driver(tmp_path):
    """450 synthetic images labelled 3 -> N = 400 at 16 angles = 6400 rotations, 5760 after the eval split, 5400 without the
    test angle, 4050 after the drop: the train set size the drivers hard-code.  One epoch of SVGPVAE_Hensman on the files as
    the generator names them for the drivers."""
    from svgp_vae_amd import MNIST_experiment
    rs = np.random.RandomState(3)
    x = (rs.randint(0, 256, (450, 28, 28)) * (rs.rand(450, 28, 28) < 0.2)).astype(np.uint8)
    d = str(tmp_path) + "/"
    paths = generate_rotated_MNIST(d, N=400, digits=[3], latent_dim_object_vector=8, mnist=(x, np.full(450, 3, dtype=np.uint8)),
                                   driver_names=True)
    assert sorted(os.path.basename(p) for p in paths.values()) == ["eval_data3.p", "pca_ov_init3.p", "test_data3.p",
                                                                    "train_data3.p"]
    with open(paths["train"], "rb") as f:
        train = pickle.load(f)
    assert train["images"].shape == (4050, 28, 28, 1) and train["aux_data"].shape == (4050, 10)
    log = MNIST_experiment.main(["--elbo", "SVGPVAE_Hensman", "--dataset", "3", "--mnist_data_path", d, "--opt_regime", "joint-1",
                                 "--eval_every", "1", "--M", "8", "--base_dir", d])
    elbos = [s["elbo"] for s in log["steps"]]
    assert len(elbos) == 16 and sum(s["rows"] for s in log["steps"]) == 4050 and all(np.isfinite(elbos))
    assert len(log["cgen_mse"]) == 1 and np.isfinite(log["cgen_mse"][0][1])
