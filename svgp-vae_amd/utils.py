"""Host-side data utilities of the rotated-MNIST driver, mirroring the reference's `utils.py`
(names and semantics; numpy / torch instead of tf.data):

  import_rotated_mnist(MNIST_path, ending, batch_size)   utils.py:799-875
  generate_init_inducing_points(train_data_path, n, ...) utils.py:691-744
  parse_opt_regime(arr)                                  utils.py:891-899
  gauss_cross_entropy(mu1, var1, mu2, var2)              utils.py:483-504 (element-wise; inside the step it is fused
                                                         into the HIP per-sample kernel, this is the stand-alone form)
  Make_Video_batch / build_video_batch_graph / MSE_rotation   utils.py:59-121,138-192,195-245 (moving ball; ball.py)
  compute_bias_variance_mean_estimators(arr_batch, arr_full)  utils.py:922-948 (host; the driver's --bias_analysis keeps the
                                                         sum on the device: engine.mean_vectors_*)
  latent_samples_SVGPVAE(train_images, train_aux_data, vae, svgp, clipping_qs)   utils.py:975-1008
  generate_rotated_MNIST(save_path, N, nr_angles, ...)   utils.py:507-657 (the digits are an argument, not a download; the
                                                         rotations run as `svgp_rotate_cubic_f64`: rotate_images)
"""
import math
import pickle
import random

import numpy as np


def _load(path):
    with open(path, "rb") as f:
        d = pickle.load(f)
    return {"images": np.asarray(d["images"], dtype=np.float64), "aux_data": np.asarray(d["aux_data"], dtype=np.float64)}


def batches(n_rows, batch_size):
    """Un-shuffled `.batch(batch_size)` without drop_remainder (utils.py:846-848): the final short batch
    is used (4050 = 15*256 + 210)."""
    return [(lo, min(lo + batch_size, n_rows)) for lo in range(0, n_rows, batch_size)]


def import_rotated_mnist(MNIST_path, ending, batch_size, train_file=None):
    """Returns (train_data_dict, eval_data_dict, test_data_dict, train_batches).  `train_file` overrides
    `train_data<ending>` (the reference checkout ships without train_data3.p, see .MISSING_LARGE_BLOBS)."""
    train = _load(train_file or (MNIST_path + "train_data" + ending))
    ev = _load(MNIST_path + "eval_data" + ending)
    te = _load(MNIST_path + "test_data" + ending)
    return train, ev, te, batches(len(train["images"]), batch_size)


def generate_init_inducing_points(train_data_path, n=5, nr_angles=16, seed_init=0, remove_test_angle=None,
                                  PCA=False, M=8, seed=0, aux_data=None):
    """utils.py:691-744: for each of `nr_angles` angles draw n object vectors from the empirical (KDE)
    distribution of the train PCA embeddings (PCA=True) or N(0,1.5^2); rows [id, angle, vector].
    n < 1 keeps a random subset of int(n*nr_angles) angles with one vector each."""
    import scipy.stats
    random.seed(seed)
    data = aux_data if aux_data is not None else _load(train_data_path)["aux_data"]
    angles = np.linspace(0, 2 * np.pi, nr_angles + 1)[:-1]
    if n < 1:
        indices = random.sample(list(range(nr_angles)), int(n * nr_angles))
        n = 1
    else:
        indices = range(nr_angles)
    pts = []
    for i in indices:
        if i == remove_test_angle:
            continue
        s = seed_init + i
        if PCA:
            obj = [scipy.stats.gaussian_kde(data[:, ax]).resample(int(n), seed=s) for ax in range(2, 2 + M)]
            obj = np.concatenate(tuple(obj)).T
        else:
            obj = np.random.normal(0, 1.5, int(n) * M).reshape(int(n), M)
        pts.append(np.hstack((np.full((int(n), 1), angles[i]), obj)))
    pts = np.concatenate(tuple(pts))
    return np.hstack((np.array([list(range(len(pts)))]).T, pts))


def parse_opt_regime(arr):
    """utils.py:891-899: ['joint-1000'] -> (1000, ['joint']*1000)."""
    arr = list(arr)
    for i in range(len(arr)):
        regime, nr_epochs = arr[i].split("-")
        arr[i] = (regime, int(nr_epochs))
    training_regime = [r for regime in arr for r in [regime[0]] * regime[1]]
    return len(training_regime), training_regime


def gauss_cross_entropy(mu1, var1, mu2, var2):
    """utils.py:483-504: element-wise cross-entropy H[N(mu1, var1), N(mu2, var2)] =
    -1/2 (log 2 pi + log var2 + (var1 + mu1^2 - 2 mu1 mu2 + mu2^2) / var2).  Runs as `svgp_gauss_cross_entropy` on
    float64 device tensors of any (equal) shape."""
    import torch
    from ._lib import call
    mu1, var1, mu2, var2 = (t.to(torch.float64).contiguous() for t in torch.broadcast_tensors(mu1, var1, mu2, var2))
    if not mu1.is_cuda:
        from ._lib import SvgpError
        raise SvgpError("gauss_cross_entropy needs device tensors; there is no CPU execution path")
    out = torch.empty_like(mu1)
    s = torch.cuda.current_stream(mu1.device).cuda_stream
    call("svgp_gauss_cross_entropy", mu1.numel(), mu1.data_ptr(), var1.data_ptr(), mu2.data_ptr(), var2.data_ptr(),
         out.data_ptr(), s)
    return out


def _host_array(t):
    """A contiguous numpy copy of an array or a tensor (any device)."""
    return np.array(t.detach().cpu().numpy() if hasattr(t, "detach") else t)


def compute_bias_variance_mean_estimators(arr_batch, arr_full):
    """utils.py:922-948 (Supplementary C.4): arr_batch (B, L, m), the mean vectors of the B steps of an epoch, arr_full (L, m),
    the ones of the whole train set -- arrays, tensors or lists of them.  Returns mean_l sum_j |(sum_b arr_batch[b][l][j]) / B -
    arr_full[l][j]|, on the host with the reference's operation order (steps added left to right, np.sum, np.mean), so the
    result is the reference's to the bit.  The inputs are not modified (the reference adds into arr_batch[0]).  The variance
    is a TODO of the reference."""
    batch = [[_host_array(x) for x in step] for step in arr_batch]
    full = [_host_array(x) for x in arr_full]
    B, L, m = len(batch), len(batch[0]), batch[0][0].shape[0]
    assert L == len(full)
    assert m == full[0].shape[0]
    avg_arr_batch = [0] * L
    for l in range(L):
        for b in range(B):
            if b == 0:
                avg_arr_batch[l] = batch[b][l]
            else:
                avg_arr_batch[l] += batch[b][l]
    avg_arr_batch = [x / B for x in avg_arr_batch]
    bias = [np.sum(np.abs(x - y)) for x, y in zip(avg_arr_batch, full)]
    return np.mean(bias)


def latent_samples_SVGPVAE(train_images, train_aux_data, vae, svgp, clipping_qs=False, epsilon=None):
    """utils.py:975-1008: latent samples z = p_m + epsilon sqrt(p_v) (N, L) of the given rows, p_m / p_v from
    svgp.approximate_posterior_params(aux, aux, qnet_mu[:, l], qnet_var[:, l]) per channel -- here one pass over all L
    channels on the engine bound to (vae, svgp), c = N_train / N.  epsilon (N, L): the N(0,1) draw of :1005 as an input;
    None: drawn on the device by torch's generator (the engine's own counter-based generator belongs to the training
    trajectory and is left alone).  Returns a device tensor."""
    import math

    import torch
    from .SVGPVAE_model import _runtime
    N = train_images.shape[0]
    rt = svgp._rt
    if rt is None or rt.eng.b_max < N:        # as in bacthing_predict_SVGPVAE_rotated_mnist: a larger engine, same training state
        rt = _runtime(vae, svgp, clipping_qs if rt is None else rt.key[0], False if rt is None else rt.key[1],
                      math.sqrt(0.020) if rt is None else rt.key[2], N)
    eng = rt.eng
    if epsilon is None:
        epsilon = torch.randn(N, vae.L, dtype=torch.float64, device=eng.device)
    return eng.latent_samples_full(train_images, train_aux_data, epsilon, clip_qs=clipping_qs)


def rotate_images(images, angles_deg, device=None, chunk=4096):
    """images (n, H, W) rotated by every angle of angles_deg (A, degrees), as `scipy.ndimage.rotate(image, angle, reshape=False)`
    with its defaults (cubic spline, mode 'constant', cval 0, prefilter): an (n, A, H, W) float64 device tensor.  The work is
    `svgp_rotate_cubic_f64` (csrc/rotate.hip; 2 <= H, W <= 64), launched on `chunk` images at a time on the current stream;
    the cosines and sines come from scipy.special.cosdg / sindg like scipy's own, so the quarter turns are exact."""
    import torch
    from scipy.special import cosdg, sindg
    from ._lib import SvgpError, call, load_library
    load_library()
    if not torch.cuda.is_available():
        raise SvgpError("rotate_images needs a HIP device (torch.cuda.is_available() is False); there is no CPU execution path")
    if device is None:
        device = images.device if hasattr(images, "is_cuda") and images.is_cuda else "cuda"
    dev = torch.device(device)
    images = torch.as_tensor(images).to(device=dev, dtype=torch.float64).contiguous()
    if images.dim() != 3:
        raise ValueError(f"images must be (n, H, W), got {tuple(images.shape)}")
    angles = np.atleast_1d(np.asarray(angles_deg, dtype=np.float64))
    cos_sin = torch.as_tensor(np.stack([cosdg(angles), sindg(angles)], axis=1), dtype=torch.float64).to(dev).contiguous()
    n, H, W = images.shape
    A = len(angles)
    out = torch.empty((n, A, H, W), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev).cuda_stream
        for lo in range(0, n, chunk):
            hi = min(lo + chunk, n)
            call("svgp_rotate_cubic_f64", hi - lo, H, W, A, images[lo:hi].data_ptr(), cos_sin.data_ptr(), out[lo:hi].data_ptr(), s)
    return out


def _rotate_on_device(images, angles_deg, chunk=4096):
    """The default `rotate` of generate_rotated_MNIST: rotate_images on `chunk` images at a time, every chunk copied to the host
    before the next one runs, so a 60 000-digit run holds one chunk of rotations on the device, not all of them."""
    images = np.asarray(images, dtype=np.float64)
    out = np.empty((len(images), len(angles_deg)) + images.shape[1:], dtype=np.float64)
    for lo in range(0, len(images), chunk):
        out[lo:lo + chunk] = rotate_images(images[lo:lo + chunk], angles_deg).cpu().numpy()
    return out


def generate_rotated_MNIST(save_path, N=400, nr_angles=16, valid_set_size=0.1, drop_rate=0.25, digits=[3, 6],
                           latent_dim_object_vector=8, shuffle_data=True, seed=0, *, mnist=None, driver_names=False, rotate=None):
    """utils.py:507-657: the rotated-MNIST data sets of Casale's paper.  Writes the train, eval and test sets as pickles of
    {'images': (rows, 28, 28, 1) float64, unclipped, 'aux_data': (rows, 2 + latent_dim_object_vector) rows [image id, angle in
    radians, PCA embedding]} and the PCA embeddings of the N * len(digits) chosen digits (the object-vector init) as a fourth.

    Positional arguments and behaviour are the reference's: `random.seed(seed)`, N images of every digit drawn with
    random.sample, sklearn PCA over the chosen images, every image at the nr_angles angles of [0, 360) (rows image-major,
    angle-minor), per digit the last valid_set_size of the rows to the eval set (shuffled with random.sample when
    shuffle_data), one angle drawn with random.sample as the test angle, and drop_rate of the train and of the test rows dropped
    (a random subset when shuffle_data; otherwise the tail, which is then written as `train_not_in_test_data...`).

      mnist         (x_train uint8 (n, 28, 28), y_train (n)): the raw digits.  The reference downloads them through Keras
                    (:534); nothing is fetched here, None raises a ValueError.
      driver_names  False: the reference's file names `train_data<digits>_<M>.p`, `pca_ov_init<digits>_<M>.p`, ... with
                    M = latent_dim_object_vector (:561, :644; `_not_shuffled_<M>.p` without shuffle_data) -- sic: the
                    reference's own drivers never read these names.  True: the names the drivers do read,
                    `train_data<digits>.p`, `eval_data<digits>.p`, `test_data<digits>.p`, `pca_ov_init<digits>.p`
                    (MNIST_experiment.py --dataset <digits>; `<digits>_not_shuffled.p` without shuffle_data).
      rotate        callable (images (n, H, W), angles_deg (A)) -> (n, A, H, W) array standing in for the device kernel, the
                    seam for tests without a GPU.  Default: `svgp_rotate_cubic_f64` through rotate_images.  The package
                    supplies no CPU implementation.

    Returns {'train': path, 'eval': path, 'test': path, 'pca': path[, 'train_not_in_test': path]}."""
    from sklearn.decomposition import PCA
    if mnist is None:
        raise ValueError("generate_rotated_MNIST: pass the raw digits as mnist=(x_train uint8 (n, 28, 28), y_train (n)); "
                         "this build downloads nothing (the reference fetches them through tf.keras.datasets.mnist)")
    M = latent_dim_object_vector
    random.seed(seed)
    angles = np.linspace(0, 360, nr_angles + 1)[:-1]
    x_all, y_all = np.asarray(mnist[0]), np.asarray(mnist[1])
    x_all = x_all / 255.0                                   # [0, 255] -> [0, 1]

    chosen = []
    for digit in digits:
        x_digit = x_all[y_all == digit]
        print('Number of images with digit {}: {}'.format(digit, len(x_digit)))
        chosen.append(x_digit[random.sample(list(range(len(x_digit))), N)])      # (N, 28, 28)
    x = np.concatenate(chosen)
    n_obj = len(digits) * N
    assert n_obj == x.shape[0]

    pca = PCA(n_components=M)
    pca_df = pca.fit_transform(x.copy().reshape((n_obj, -1)))
    print("Explained variance ratio PCA: {}".format(pca.explained_variance_ratio_))
    digit_ending = "".join(str(d) for d in digits)
    paths = {"pca": save_path + ('pca_ov_init{}.p'.format(digit_ending) if driver_names
                                 else 'pca_ov_init{}_{}.p'.format(digit_ending, M))}
    with open(paths["pca"], 'wb') as f:
        pickle.dump(pca_df, f)

    # rows image-major, angle-minor: [id, radians(angle), pca...]
    rotated = np.asarray((rotate or _rotate_on_device)(x, angles), dtype=np.float64)
    if rotated.shape != (n_obj, nr_angles) + x.shape[1:]:
        raise ValueError(f"rotate returned {rotated.shape}, expected {(n_obj, nr_angles) + x.shape[1:]}")
    images = rotated.reshape((n_obj * nr_angles,) + x.shape[1:])[..., np.newaxis]
    aux_data = np.concatenate([np.array([tuple([i, math.radians(angle)] + list(pca_df[i])) for angle in angles])
                               for i in range(n_obj)])

    # per digit: the head of its rows stays, the tail is the eval set
    N_digit = int(len(images) / len(digits))
    N_keep = int(N_digit * (1 - valid_set_size))
    keep = np.concatenate([np.arange(d * N_digit, d * N_digit + N_keep) for d in range(len(digits))])
    held = np.concatenate([np.arange(d * N_digit + N_keep, (d + 1) * N_digit) for d in range(len(digits))])
    eval_images, eval_aux_data = images[held], aux_data[held]
    images, aux_data = images[keep], aux_data[keep]
    if shuffle_data:
        eval_idx = random.sample(list(range(len(eval_images))), len(eval_images))
        eval_images, eval_aux_data = eval_images[eval_idx], eval_aux_data[eval_idx]

    # one angle is the test set
    test_angle = random.sample(list(angles), 1)[0]
    mask = aux_data[:, 1] == math.radians(test_angle)
    train_images, train_aux_data, test_images, test_aux_data = images[~mask], aux_data[~mask], images[mask], aux_data[mask]
    print("Test angle: {}".format(test_angle))

    # drop some rows
    n_train, n_test = int(len(train_images) * (1 - drop_rate)), int(len(test_images) * (1 - drop_rate))
    if shuffle_data:
        idx_train = random.sample(list(range(len(train_images))), n_train)
        idx_test = random.sample(list(range(len(test_images))), n_test)
    else:
        idx_train, idx_test = list(range(n_train)), list(range(n_test))
        rest_images, rest_aux_data = train_images[n_train:], train_aux_data[n_train:]
    train_images, train_aux_data = train_images[idx_train], train_aux_data[idx_train]
    test_images, test_aux_data = test_images[idx_test], test_aux_data[idx_test]

    print('Size of training data: {}'.format(len(train_images)))
    print('Size of validation data: {}'.format(len(eval_images)))
    print('Size of test data: {}'.format(len(test_images)))
    if not shuffle_data:
        print('Size of training data without test ids: {}'.format(len(rest_images)))

    if driver_names:
        ending = digit_ending + ("" if shuffle_data else "_not_shuffled") + ".p"
    else:
        ending = digit_ending + ("_{}.p".format(M) if shuffle_data else "_not_shuffled_{}.p".format(M))
    print(ending)
    sets = [("train", 'train_data', train_images, train_aux_data), ("eval", 'eval_data', eval_images, eval_aux_data),
            ("test", 'test_data', test_images, test_aux_data)]
    if not shuffle_data:
        sets.append(("train_not_in_test", 'train_not_in_test_data', rest_images, rest_aux_data))
    for key, stem, im, aux in sets:
        paths[key] = save_path + stem + ending
        with open(paths[key], 'wb') as f:
            pickle.dump({'images': im, 'aux_data': aux}, f)
    return paths


def __getattr__(name):
    # the moving-ball data utilities live beside their device kernels in ball.py (BALL_experiment.py:11-12)
    if name in ("Make_path_batch", "Make_Video_batch", "MSE_rotation", "build_video_batch_graph"):
        from . import ball
        return ball.VideoBatchSource if name == "build_video_batch_graph" else getattr(ball, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
