"""In-kernel phase timeline of the two longest launches of the config-2 step (b = 256, m = 32, L = 16): the fused decoder launch
(svgp_mnist_decoder_fwd_bwd_data_pre_tail, launch 5) and the reverse factor launch with its riders (svgp_gp_stats_factor_bwd_wgrad,
launch 6), from their probe instances (include/svgpvae_hip.h: one row of wall_clock64() stamps per workgroup, 100 MHz, one time axis).

One full step makes the inputs valid; each product launch runs a few times, then its probe instance twice, and the second (warm)
launch is printed: microseconds per phase, the `at` column is the phase's END measured from the first workgroup's entry.  A probe
launch is not a product launch (its stamps cost a store each and two barriers more): read shares, not the total.
usage: python tools/decoder_phase_probe.py"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEC_SLOTS, FB_SLOTS = 16, 8
DEC_PHASES = ["entry", "weights staged", "z", "dense", "UpC1 forward", "UpC2 forward", "UpC3 forward", "copy-outs + sq. error",
              "UpC3 data-reverse", "d2 scaled, stored", "UpC2 data-reverse", "d1 scaled, stored", "UpC1 data-reverse", "z-bar", "exit"]
FB_PHASES = ["entry", "staged", "UpC3 product", "UpC2 product", "UpC1 + dense", "partial stored", "exit"]
GROUPS = {2: "UpC2", 1: "UpC3", 4: "UpC1 + dense"}
US = 0.01           # one tick of the 100 MHz counter


def place(word):
    """last slot of a row -> (compute-unit key, role, detail)"""
    return ((word >> 32) & 15, (word >> 8) & 0xFF), (word >> 60) & 15, (word >> 56) & 15


def main():
    import torch

    import bench
    from svgp_vae_amd import _lib
    from svgp_vae_amd.engine import MnistStepEngine
    _lib.load_library()
    params, images, aux, eps = bench.synthetic_problem(0, 256, 32, 8)
    dev = torch.device("cuda:0")
    eng = MnistStepEngine(32, 16, 8, 400, geco=True, b_max=256)
    eng.load_params(params)
    t = lambda x: torch.tensor(x, dtype=torch.float64, device=dev).contiguous()
    eng.bind(t(images), t(aux), t(eps))
    eng.run(adam=False)
    eng.synchronize()
    cfg, th, ws, st = C.byref(eng.cfg), eng.theta.data_ptr(), eng.ws.data_ptr(), eng.state.data_ptr()
    img, s = eng._bound[0].data_ptr(), eng.stream.cuda_stream

    def rows(product, probe, slots):
        stamps = torch.zeros(4096 * slots, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        for _ in range(5):
            _lib.call(*product)
        for _ in range(2):
            eng.synchronize()
            stamps.zero_()
            torch.cuda.synchronize()
            _lib.call(probe[0], *probe[1], stamps.data_ptr(), stamps.numel(), s)
        eng.synchronize()
        r = stamps.cpu().view(-1, slots)
        r = r[r[:, 0] != 0]
        return [[int(v) & (2 ** 64 - 1) for v in row] for row in r.tolist()]

    # ---- launch 5
    dec = rows(("svgp_mnist_decoder_fwd_bwd_data_pre_tail", cfg, th, img, ws, st, s),
               ("svgp_mnist_decoder_fwd_bwd_data_pre_tail_probe", (cfg, th, img, ws, st)), DEC_SLOTS)
    t0 = min(r[0] for r in dec)
    image = [(i, r) for i, r in enumerate(dec) if place(r[15])[1] == 1]
    rider_cus = {place(r[15])[0] for r in dec if place(r[15])[1] == 2}
    shared = [(i, r) for i, r in image if place(r[15])[0] in rider_cus]
    picks = [("first", image[0]), ("middle", image[len(image) // 2]), ("last", image[-1])]
    if shared:
        picks.append(("beside a rider", shared[0]))
    print(f"launch 5, svgp_mnist_decoder_fwd_bwd_data_pre_tail: {len(dec)} workgroups ({len(image)} image, {len(dec) - len(image)} riders on "
          f"{len(rider_cus)} compute units; {len(shared)} image workgroups share one with a rider); first entry to last exit "
          f"{(max(r[14] for r in dec) - t0) * US:.2f} us; riders exit (thread 0) at "
          f"{min((r[14] - t0) * US for r in dec if place(r[15])[1] == 2):.2f} .. {max((r[14] - t0) * US for r in dec if place(r[15])[1] == 2):.2f} us")
    print(f"{'phase':24s}" + "".join(f"{name + ' (wg ' + str(i) + ')':>26s}" for name, (i, _) in picks) + f"{'median of all':>16s}")
    print(f"{'':24s}" + "".join(f"{'us':>14s}{'at':>12s}" for _ in picks) + f"{'us':>16s}")
    for k, name in enumerate(DEC_PHASES):
        line = f"{name:24s}"
        for _, (_, r) in picks:
            line += f"{((r[k] - r[k - 1]) * US if k else 0.0):14.2f}{(r[k] - t0) * US:12.2f}"
        d = sorted((r[k] - r[k - 1]) * US for _, r in image) if k else sorted((r[0] - t0) * US for _, r in image)
        print(line + f"{d[len(d) // 2]:16.2f}")

    # ---- launch 6
    fb = rows(("svgp_gp_stats_factor_bwd_wgrad", cfg, img, ws, st, s), ("svgp_gp_stats_factor_bwd_wgrad_probe", (cfg, img, ws, st)),
              FB_SLOTS)
    t0 = min(r[0] for r in fb)
    role = lambda r: place(r[7])[1]
    stats, chans, riders = ([r for r in fb if role(r) == k] for k in (1, 2, 3))
    print(f"\nlaunch 6, svgp_gp_stats_factor_bwd_wgrad: {len(fb)} workgroups ({len(stats)} statistics, {len(chans)} channel, {len(riders)} riders); "
          f"first entry to last exit {(max(r[6] for r in fb) - t0) * US:.2f} us")
    print(f"statistics workgroups: entries {min(r[0] - t0 for r in stats) * US:.2f} .. {max(r[0] - t0 for r in stats) * US:.2f} us, "
          f"exits {min(r[6] - t0 for r in stats) * US:.2f} .. {max(r[6] - t0 for r in stats) * US:.2f} us")
    c_first, c_last = min(chans, key=lambda r: r[6]), max(chans, key=lambda r: r[6])
    print(f"channel workgroups: first to finish {(c_first[0] - t0) * US:.2f} -> {(c_first[6] - t0) * US:.2f} us, last to finish "
          f"{(c_last[0] - t0) * US:.2f} -> {(c_last[6] - t0) * US:.2f} us")
    print(f"{'rider':34s}{'entry at':>10s}{'staged':>10s}{'product':>10s}{'stored':>10s}{'exit at':>10s}")
    for mask, name in GROUPS.items():
        grp = sorted((r for r in riders if place(r[7])[2] == mask), key=lambda r: r[0])
        if not grp:
            continue
        k = {1: 2, 2: 3, 4: 4}[mask]            # the slot that closes this group's product
        for label, r in (("first", grp[0]), ("last", grp[-1])):
            print(f"{name + ', ' + label + ' of ' + str(len(grp)):34s}{(r[0] - t0) * US:10.2f}{(r[1] - r[0]) * US:10.2f}"
                  f"{(r[k] - r[1]) * US:10.2f}{(r[5] - r[4]) * US:10.2f}{(r[6] - t0) * US:10.2f}")
        med = lambda f: sorted(f(r) for r in grp)[len(grp) // 2] * US
        print(f"{name + ', median':34s}{med(lambda r: r[0] - t0):10.2f}{med(lambda r: r[1] - r[0]):10.2f}{med(lambda r: r[k] - r[1]):10.2f}"
              f"{med(lambda r: r[5] - r[4]):10.2f}{med(lambda r: r[6] - t0):10.2f}")
    print(f"last rider exit {(max(r[6] for r in riders) - t0) * US:.2f} us; last channel exit {(c_last[6] - t0) * US:.2f} us")


if __name__ == "__main__":
    main()
