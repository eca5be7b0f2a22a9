"""BUILD CONTAINER ONLY.  Runs the reference's own `utils.generate_rotated_MNIST` (/root/reference/utils.py:507-657) on synthetic
digits and stores its inputs + outputs as tests/golden/ref_rotated_mnist.npz.

    python tests/golden/make_ref_rotated_mnist_fixture.py

The reference imports TensorFlow & co. at module level and fetches the digits with `tf.keras.datasets.mnist.load_data()`.
Both are replaced for the duration of the run: the modules by the inert stand-ins of make_ref_host_fixtures.py, the loader by
a function that returns the synthetic digits below.  Everything else (random.sample order, sklearn PCA, scipy.ndimage.rotate,
the splits, the drop, the pickles) runs as the reference wrote it.  sklearn's PCA picks its randomized solver at this shape and
draws from numpy's global generator (the reference passes no random_state): the generator is seeded with NP_SEED before every
call, and the test applies the same pin.  Nothing of the reference's source travels: only the
arrays below are committed, and tests/test_rotated_mnist_cpu.py / tests/test_gpu_rotated_mnist.py compare
`svgp_vae_amd.utils.generate_rotated_MNIST` with them.

Run: 60 sparse uint8 images (28, 28) with labels cycling 3, 6, 1; N = 12, latent_dim_object_vector = 4, digits [3, 6], seed 2,
shuffle_data True and False (the second writes the fourth file, train_not_in_test_data).  Stored per mode <m> in (shuffled,
not_shuffled) and split <s>: `<m>_files` (the names written), `<m>_pca`, `<m>_<s>_aux`, `<m>_<s>_shape`, `<m>_<s>_sums` (per-row
pixel sums), and the test split's images in full as `<m>_test_images`."""
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ref_rotated_mnist.npz")
RUN = dict(N=12, latent_dim_object_vector=4, digits=[3, 6], seed=2)
NP_SEED = 5


def synthetic_digits(seed=0, n=60):
    """(x uint8 (n, 28, 28), y (n)): about one pixel in five non-zero, labels 3, 6, 1, 3, 6, 1, ..."""
    rs = np.random.RandomState(seed)
    x = (rs.randint(0, 256, (n, 28, 28)) * (rs.rand(n, 28, 28) < 0.2)).astype(np.uint8)
    y = np.array([3, 6, 1] * (n // 3 + 1))[:n].astype(np.uint8)
    return x, y


def main():
    sys.path.insert(0, HERE)
    from make_ref_host_fixtures import import_reference          # the inert TensorFlow & co. stand-ins
    U, _ = import_reference()
    x, y = synthetic_digits()
    U.tf.keras.datasets.mnist.load_data = lambda: ((x, y), (None, None))
    fx = {"x_train": x, "y_train": y}
    for mode, shuffle in (("shuffled", True), ("not_shuffled", False)):
        with tempfile.TemporaryDirectory() as d:
            np.random.seed(NP_SEED)
            U.generate_rotated_MNIST(d + "/", shuffle_data=shuffle, **RUN)
            names = sorted(os.listdir(d))
            fx[mode + "_files"] = np.array(names)
            for name in names:
                with open(os.path.join(d, name), "rb") as f:
                    obj = pickle.load(f)
                if name.startswith("pca_ov_init"):
                    fx[mode + "_pca"] = np.asarray(obj)
                    continue
                split = name[:name.index("_data")]
                fx[f"{mode}_{split}_aux"] = obj["aux_data"]
                fx[f"{mode}_{split}_shape"] = np.array(obj["images"].shape)
                fx[f"{mode}_{split}_sums"] = obj["images"].reshape(len(obj["images"]), -1).sum(1)
                if split == "test":
                    fx[mode + "_test_images"] = obj["images"]
    np.savez_compressed(OUT, **fx)
    print("wrote", OUT, os.path.getsize(OUT), {k: np.asarray(v).shape for k, v in fx.items()})


if __name__ == "__main__":
    main()
