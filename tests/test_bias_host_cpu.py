"""Host side of --bias_analysis / --save_latents: `utils.compute_bias_variance_mean_estimators` against values the reference's
own function returned (tests/golden/make_ref_bias_fixture.py -> ref_bias_fixture.npz), and the three names the reference's
driver imports for the two flags (MNIST_experiment.py:15-21) under the modules it imports them from."""
import os

import numpy as np
import pytest
import torch

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_bias_fixture.npz")
CASES = [(1, 1, 1), (3, 2, 5), (7, 16, 32)]


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FIX))


@pytest.mark.parametrize("k", range(len(CASES)), ids=[str(c) for c in CASES])
def test_bias_is_bit_equal_to_the_reference(fx, k):
    from svgp_vae_amd.utils import compute_bias_variance_mean_estimators as f
    batch, full, want = fx[f"batch_{k}"], fx[f"full_{k}"], fx[f"bias_{k}"]
    assert batch.shape == CASES[k] and full.shape == CASES[k][1:]
    B, L, m = CASES[k]
    keep = batch.copy()
    forms = {
        "arrays": (batch, full),
        "lists of arrays": ([[batch[b, l] for l in range(L)] for b in range(B)], [full[l] for l in range(L)]),
        "list of (L, m) tensors": ([torch.from_numpy(batch[b].copy()) for b in range(B)], torch.from_numpy(full.copy())),
        "tensors": (torch.from_numpy(batch.copy()), torch.from_numpy(full.copy())),
    }
    for name, (a, b) in forms.items():
        got = f(a, b)
        assert np.float64(got) == want, (name, float(got), float(want))       # to the bit
    assert np.array_equal(batch, keep), "the inputs must not be modified (the reference adds into the first step's arrays)"


def test_bias_checks_the_shapes():
    from svgp_vae_amd.utils import compute_bias_variance_mean_estimators as f
    with pytest.raises(AssertionError):
        f(np.zeros((2, 3, 4)), np.zeros((2, 4)))
    with pytest.raises(AssertionError):
        f(np.zeros((2, 3, 4)), np.zeros((3, 5)))


def test_the_reference_import_lines_of_the_two_flags_resolve():
    ns = {}
    exec("from svgp_vae_amd.utils import compute_bias_variance_mean_estimators, latent_samples_SVGPVAE", ns)   # MNIST_experiment.py:15-17
    exec("from svgp_vae_amd.SVGPVAE_model import batching_encode_SVGPVAE_full", ns)                            # :19-21
    for n in ("compute_bias_variance_mean_estimators", "latent_samples_SVGPVAE", "batching_encode_SVGPVAE_full"):
        assert callable(ns[n]), n
    import inspect
    from svgp_vae_amd import SVGPVAE_model, utils
    assert list(inspect.signature(SVGPVAE_model.batching_encode_SVGPVAE_full).parameters) == ["train_images", "vae", "clipping_qs"]
    p = list(inspect.signature(utils.latent_samples_SVGPVAE).parameters)
    assert p == ["train_images", "train_aux_data", "vae", "svgp", "clipping_qs", "epsilon"]
    assert list(inspect.signature(utils.compute_bias_variance_mean_estimators).parameters) == ["arr_batch", "arr_full"]


def test_the_plain_vae_latents_stay_absent():
    from svgp_vae_amd import utils
    with pytest.raises(ImportError):
        exec("from svgp_vae_amd.utils import latent_samples_VAE_full_train", {})
    assert not hasattr(utils, "latent_samples_VAE_full_train")


def test_save_latents_without_save_is_refused_before_any_gpu_work():
    """The refusal comes before the process group, the data files and the engine: it needs no GPU and no data."""
    from svgp_vae_amd import MNIST_experiment as E
    args = E.build_parser().parse_args(["--elbo", "SVGPVAE_Hensman", "--save_latents", "--mnist_data_path", "/nonexistent/"])
    with pytest.raises(ValueError, match="--save"):
        E.run_experiment_rotated_mnist_SVGPVAE(args)


def test_driver_docstring_names_the_flags_without_effect_and_the_deviation():
    from svgp_vae_amd import MNIST_experiment as E
    for flag in ("--test_set_metrics", "--show_pics", "--ram"):
        assert flag in E.__doc__, flag
    assert "GECO" in E.run_experiment_rotated_mnist_SVGPVAE.__doc__ and "DEVIATION" in E.run_experiment_rotated_mnist_SVGPVAE.__doc__


def test_kernel_entry_points_refuse_bad_arguments_without_a_device():
    """The argument checks of svgp_mean_vectors_accumulate / _bias come before any launch, so they answer without a GPU:
    L < 1, m < 1, a NULL pointer -> SVGP_ERR_INVALID (-1); m > 2048 -> SVGP_ERR_UNSUPPORTED (-2)."""
    import ctypes as C
    from svgp_vae_amd._lib import load_library
    lib = load_library()
    fake = C.c_void_p(4096)                                     # never dereferenced: every case fails validation first
    for (L, m), code in (((0, 5), -1), ((3, 0), -1), ((-2, 5), -1), ((3, 2049), -2)):
        assert lib.svgp_mean_vectors_accumulate(L, m, fake, fake, None) == code, (L, m)
        assert lib.svgp_mean_vectors_bias(L, m, fake, fake, fake, None) == code, (L, m)
    assert b"m <= 2048" in lib.svgp_last_error()
    assert lib.svgp_mean_vectors_accumulate(3, 5, None, fake, None) == -1
    assert lib.svgp_mean_vectors_accumulate(3, 5, fake, None, None) == -1
    for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert lib.svgp_mean_vectors_bias(3, 5, *args, None) == -1
    assert b"NULL" in lib.svgp_last_error()
