"""Writes the rotated-MNIST data sets the drivers read (`python -m svgp_vae_amd.MNIST_experiment --dataset <digits>
--mnist_data_path <save_path>`) from the raw digits of an `mnist.npz` (arrays x_train (n, 28, 28) uint8, y_train (n)):

    python -m svgp_vae_amd.make_rotated_mnist --mnist_npz mnist.npz --save_path "MNIST data/" --digits 3

utils.generate_rotated_MNIST (utils.py:507-657) with the rotations on the device.  Nothing is downloaded."""
import argparse
import os
import pickle

import numpy as np

from .utils import generate_rotated_MNIST


def build_parser():
    p = argparse.ArgumentParser(description="Rotated-MNIST data set generator")
    p.add_argument('--mnist_npz', type=str, required=True, help="the usual mnist.npz: x_train (n, 28, 28) uint8, y_train (n)")
    p.add_argument('--save_path', type=str, default='MNIST data/', help="prefix of the written files (a directory ends with /)")
    p.add_argument('--digits', type=int, nargs="+", default=[3])
    p.add_argument('--N', type=int, default=400, help="images per digit")
    p.add_argument('--nr_angles', type=int, default=16)
    p.add_argument('--M', type=int, default=8, help="dimension of the PCA object vectors")
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--not_shuffled', action='store_true', help="shuffle_data=False: ordered rows and a fourth file")
    p.add_argument('--driver_names', action=argparse.BooleanOptionalAction, default=True,
                   help="write train_data<digits>.p ... as the drivers read them (default); --no-driver_names: the reference "
                        "generator's <digits>_<M>.p names")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    with np.load(args.mnist_npz) as f:
        mnist = (f["x_train"], f["y_train"])
    d = os.path.dirname(args.save_path)
    if d:
        os.makedirs(d, exist_ok=True)
    paths = generate_rotated_MNIST(args.save_path, N=args.N, nr_angles=args.nr_angles, digits=list(args.digits),
                                   latent_dim_object_vector=args.M, shuffle_data=not args.not_shuffled, seed=args.seed,
                                   mnist=mnist, driver_names=args.driver_names)
    sizes = {}
    for key in ("train", "eval", "test"):
        with open(paths[key], "rb") as f:
            sizes[key] = len(pickle.load(f)["aux_data"])
    print("N_train {}  N_eval {}  N_test {}".format(sizes["train"], sizes["eval"], sizes["test"]))
    if sizes["train"] != len(args.digits) * 4050:
        # the drivers take N_train = len(digits) * 4050 unless they are given the train file by name
        print("N_train is not {} = len(digits) * 4050: run the drivers with --train_file '{}'".format(
            len(args.digits) * 4050, paths["train"]))
    return paths


if __name__ == "__main__":
    main()
