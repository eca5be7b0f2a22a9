"""Records tests/golden/valu_loads_<b>_<m>_<L>.npz for tests/test_gpu_valu_loads.py: one Adam step and the outputs of every stand-alone
entry point that runs a rewritten convolution form or the riders, at each of the test's shapes, from the library built in THIS
checkout, on the GPU.

The fixtures are the results of the commit BEFORE the branch-free operand loads, so the script refuses to run in any other tree: the
native sources it stands next to (svgp-vae_amd/csrc/*.hip, *.hpp, the Makefile, include/svgpvae_hip.h) must hash to the parent's
digest -- an export of the commit has no history to ask -- and where the checkout has a history, `git rev-parse HEAD` must be that
commit too.  (Copy this file and tests/test_gpu_valu_loads.py into a checkout or export of it, build, run.)
usage: python tools/make_valu_loads_golden.py [output directory, default tests/golden]"""
import glob
import hashlib
import os
import subprocess
import sys

PARENT = "7f754c3"
PARENT_SOURCES_SHA256 = "4f8cb34cdfc7e0eb6aceda10b348735258c22213b9a4ba7baf9500a4db693a77"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sources_digest(root=ROOT):
    csrc = os.path.join(root, "svgp-vae_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp")))
    files += [os.path.join(csrc, "Makefile"), os.path.join(root, "include", "svgpvae_hip.h")]
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.relpath(f, root).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(hashlib.sha256(fh.read()).digest())
    return h.hexdigest()


def main():
    if "--digest" in sys.argv:
        print(sources_digest())
        return
    digest = sources_digest()
    if digest != PARENT_SOURCES_SHA256:
        sys.exit(f"refusing to record: the native sources of {ROOT} hash to {digest}, not to those of the parent commit {PARENT}")
    if os.path.exists(os.path.join(ROOT, ".git")):
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        if head.returncode != 0 or not head.stdout.strip().startswith(PARENT):
            sys.exit(f"refusing to record: HEAD of {ROOT} is {head.stdout.strip() or head.stderr.strip()!r}, not the parent commit {PARENT}")
    import numpy as np

    from tests import test_gpu_valu_loads as T
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else T.GOLDEN
    os.makedirs(out, exist_ok=True)
    for b, m, L in T.SHAPES:
        got = T.record(b, m, L)
        path = os.path.join(out, os.path.basename(T.golden_path(b, m, L)))
        np.savez_compressed(path, **got)
        print(f"{path}: {os.path.getsize(path)} bytes, {len(got)} arrays, elbo {float(got['sc_elbo'])!r}", flush=True)


if __name__ == "__main__":
    main()
