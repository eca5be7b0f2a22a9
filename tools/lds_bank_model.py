"""LDS bank model of an image workgroup of the fused decoder launch (k_decoder_fwd_bwd_data, csrc/vae_dev.hpp:
decoder_fwd_bwd_data_images): for every group of LDS accesses of one image, how many passes the LDS needs per service group.

The rules are those of the MI355X LDS:
  - a 64-bit access (ds_read_b64 / ds_write_b64) is serviced as 2 groups of 32 lanes, a 128-bit access as 4 groups of 16 lanes;
  - the bank of byte address a is (a / 4) mod 64;
  - lanes of a group that read the same dword are served together (broadcast);
  - the DEGREE of a service group is the number of distinct dwords on its busiest bank: 1 is conflict-free, d costs d passes.
The layout (offset and pixel stride of each array, the index map of the effective-weight image) is read from the library's host entries
svgp_mnist_decoder_fused_lds_array / _fused_lds_index, which evaluate the constexpr functions the kernel uses; `packed_layout` is the
map before the activations were padded (8 doubles per pixel, no aliases), for comparison.

This is a model of the source, not of the compiled code: thread -> item maps, tap order and the clamped address (element 0) of a tap
outside the tile are those of vae_dev.hpp; the access WIDTH is known for the gathers this file was written for (ds_read_b64 in
gg_fwd, ds_read_b128 in tap_operand_group) and ASSUMED 64-bit per element everywhere else (a pair of neighbouring doubles may compile
to one ds_read2_b64 / ds_write2_b64, which is serviced per element the same way).  No counter is expected to move by exactly the
difference of two tables: waves of other phases and of the other workgroup on the compute unit share the LDS.

usage: python tools/lds_bank_model.py [L]      (prints the table for the packed and for the library's layout)"""
import ctypes as C
import os
import sys

NT, WAVE, BANKS = 512, 64, 64
ARRAYS = ["dense", "weff", "z", "h0", "a1", "a2", "d3", "d2", "d1", "dh0", "red"]


class Layout:
    """offset (doubles) and pixel stride of each array, and the place of a packed weight element in the block"""

    def __init__(self, L, offset, stride, weff_index):
        self.L, self.offset, self.stride, self._weff = L, dict(offset), dict(stride), weff_index

    def at(self, name, pixel, ch=0):
        """byte address of channel `ch` of pixel `pixel` of an activation array"""
        s = self.stride[name] or 1
        return (self.offset[name] + pixel * s + ch) * 8

    def weff(self, layer, cls, tap, ci, co, cin=8, cout=8):
        base = {1: 0, 2: 1024, 3: 2048}[layer]
        return (self.offset["weff"] + self._weff(base + ((cls * 4 + tap) * cin + ci) * cout + co)) * 8


def library_layout(lib, L=16):
    off, st = {}, {}
    for which, name in enumerate(ARRAYS):
        o, s, f, l = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        assert lib.svgp_mnist_decoder_fused_lds_array(L, which, C.byref(o), C.byref(s), C.byref(f), C.byref(l)) > 0, name
        off[name], st[name] = o.value, s.value
    return Layout(L, off, st, lambda e: int(lib.svgp_mnist_decoder_fused_lds_index(1, e)))


def packed_layout(lib, L=16):
    """the map of the launch before the pixel strides were padded: 8 doubles per pixel, every array a block of its own"""
    lay = library_layout(lib, L)
    o = lay.offset["z"]
    for name, n in (("z", 64), ("h0", 128), ("a1", 512), ("a2", 1568), ("d3", 784), ("d2", 1568), ("d1", 512), ("dh0", 128), ("red", 16)):
        lay.offset[name] = o
        o += n
    for name in ("a2", "d2", "d1"):
        lay.stride[name] = 8
    return lay


def with_strides(lay, **strides):
    """a copy of `lay` with other pixel strides (the offsets are kept: a gather's degree does not depend on where its array starts
    as long as that is a multiple of 16 bytes, which every map here keeps for a2 and which does not matter for 64-bit reads)"""
    out = Layout(lay.L, lay.offset, lay.stride, lay._weff)
    out.stride.update(strides)
    return out


def degree(addresses, width):
    """passes for one service group: distinct dwords on the busiest bank"""
    banks = {}
    for a in set(addresses):
        for w in range(0, width, 4):
            banks.setdefault(((a + w) // 4) % BANKS, set()).add((a + w) // 4)
    return max(len(v) for v in banks.values())


def service(lane_addr, width, threads=range(NT)):
    """degrees of the service groups of ONE instruction executed by `threads` (a range): lane_addr(thread) -> byte address, or None
    for a lane that is switched off; a group with no live lane is not issued"""
    per = 32 if width == 8 else 16
    out = []
    for g0 in range(0, NT, per):
        ad = [lane_addr(t) for t in range(g0, g0 + per) if t in threads]
        ad = [a for a in ad if a is not None]
        if ad:
            out.append(degree(ad, width))
    return out


# ------------------------------------------------------------------------------------------ the MFMA gather-GEMMs (gg_fwd, 16 taps)
def _gg_taps(pad):
    for t in range(16):
        py, ty, px, tx = (t >> 3) & 1, (t >> 2) & 1, (t >> 1) & 1, t & 1
        yield (py * 2 + px), (ty * 2 + tx), py + pad - 2 * ty, px + pad - 2 * tx


def gg_gather(lay, src, hs, hout, pad):
    """A operands of UpConv3::bwd_data_mfma: wave `grp` owns pixels grp * 16 .. + 15 of the hs x hs grid; per (tap, kq) one ds_read_b64
    at src[(iy * hout + ix)][kq * 4 + q], iy = 2 ya + oy, element 0 of the tile for a tap outside it"""
    out = []
    np_, ngrp = hs * hs, (hs * hs + 15) // 16
    for grp in range(ngrp):
        for _, _, oy, ox in _gg_taps(pad):
            for kq in range(2):
                def addr(t, grp=grp, oy=oy, ox=ox, kq=kq):
                    lane = t & 63
                    r, q = lane & 15, lane >> 4
                    pa = grp * 16 + r
                    pv = pa < np_
                    ya, xa = (pa // hs, pa % hs) if pv else (0, 0)
                    iy, ix = 2 * ya + oy, 2 * xa + ox
                    valid = pv and 0 <= iy < hout and 0 <= ix < hout
                    return lay.at(src, iy * hout + ix if valid else 0, kq * 4 + q)
                out += service(addr, 8, range(grp * 64, grp * 64 + 64))
    return out


def gg_weights(lay, layer, pad):
    """B operands: every wave, per (tap, kq) one ds_read_b64 at We[class][tap][r][kq * 4 + q] (weights read transposed; r < 8 clamped)"""
    out = []
    for cls, tap, _, _ in _gg_taps(pad):
        for kq in range(2):
            def addr(t, cls=cls, tap=tap, kq=kq):
                lane = t & 63
                return lay.weff(layer, cls, tap, min(lane & 15, 7), kq * 4 + (lane >> 4))
            out += service(addr, 8)
    return out


def gg_store(lay, dst, hs):
    """results: lane (r, q) stores channel r < 8 of pixels grp * 16 + q + 4 e, e = 0..3"""
    out = []
    np_, ngrp = hs * hs, (hs * hs + 15) // 16
    for grp in range(ngrp):
        for e in range(4):
            def addr(t, grp=grp, e=e):
                lane = t & 63
                r, po = lane & 15, grp * 16 + (lane >> 4) + 4 * e
                return lay.at(dst, po, r) if po < np_ and r < 8 else None
            out += service(addr, 8, range(grp * 64, grp * 64 + 64))
    return out


# ------------------------------------------------------------------------------------------ the rolled VALU forward (fwd_valu<true, true>)
def _fwd_items(hs, pad, cout):
    hout, ncg = 2 * hs - 2 + 2 * pad, max(cout // 2, 1)
    return hout, ncg, hout * hout * ncg


def fwd_gather(lay, src, hs, pad, cout):
    """activations of a tap: 4 ds_read_b128 (channel pairs 0..3) at src[(sy * hs + sx)], element 0 for a tap outside the tile"""
    hout, ncg, n = _fwd_items(hs, pad, cout)
    out = []
    for it0 in range(0, n, NT):
        for ty in range(2):
            for tx in range(2):
                for v in range(4):
                    def addr(t, it0=it0, ty=ty, tx=tx, v=v):
                        it = it0 + t
                        if it >= n:
                            return None
                        p = it // ncg
                        x, y = p % hout, p // hout
                        sy, sx = ((y - pad) >> 1) + ty, ((x - pad) >> 1) + tx
                        valid = 0 <= sy < hs and 0 <= sx < hs
                        return lay.at(src, sy * hs + sx if valid else 0, 2 * v)
                    out += service(addr, 16)
    return out


def fwd_weights(lay, layer, hs, pad, cout):
    """weights of a tap: ds_read_b128 at We[class][tap][ci][2 cg .. + 1] (8 per tap), or [ci, ci + 1][0] for one output channel (4)"""
    hout, ncg, n = _fwd_items(hs, pad, cout)
    out = []
    for it0 in range(0, n, NT):
        for tap in range(4):
            for ci in (range(8) if cout > 1 else range(0, 8, 2)):
                def addr(t, it0=it0, tap=tap, ci=ci):
                    it = it0 + t
                    if it >= n:
                        return None
                    cg, p = it % ncg, it // ncg
                    x, y = p % hout, p // hout
                    cls = ((y - pad) & 1) * 2 + ((x - pad) & 1)
                    return lay.weff(layer, cls, tap, ci, 2 * cg if cout > 1 else 0, 8, cout)
                out += service(addr, 16)
    return out


def fwd_store(lay, dst, hs, pad, cout):
    hout, ncg, n = _fwd_items(hs, pad, cout)
    out = []
    for it0 in range(0, n, NT):
        for g in range(2 if cout > 1 else 1):
            def addr(t, it0=it0, g=g):
                it = it0 + t
                return lay.at(dst, it // ncg, (it % ncg) * 2 + g) if it < n else None
            out += service(addr, 8)
    return out


# ------------------------------------------------------------------------------------------ the VALU data reverse of UpC3 (bwd_data_valu)
def valu_rev(lay, what):
    """item = (stored pixel of the 14 x 14 grid, channel pair ig): 16 (class, tap) reads of d3 (one channel) and of the pair's two weights"""
    hs, hout, pad, n = 14, 28, 1, 14 * 14 * 4
    out = []
    for it0 in range(0, n, NT):
        if what == "store":
            for g in range(2):
                def addr(t, it0=it0, g=g):
                    it = it0 + t
                    return lay.at("d2", it // 4, (it % 4) * 2 + g) if it < n else None
                out += service(addr, 8)
            continue
        for cy in range(4):
            for cx in range(4):
                py, ty, px, tx = cy >> 1, cy & 1, cx >> 1, cx & 1
                for g in range(1 if what == "d3" else 2):
                    def addr(t, it0=it0, py=py, ty=ty, px=px, tx=tx, g=g):
                        it = it0 + t
                        if it >= n:
                            return None
                        ig, ps = it % 4, it // 4
                        if what == "weights":
                            return lay.weff(3, py * 2 + px, ty * 2 + tx, ig * 2 + g, 0, 8, 1)
                        y, x = 2 * (ps // hs - ty) + py + pad, 2 * (ps % hs - tx) + px + pad
                        valid = 0 <= y < hout and 0 <= x < hout
                        return lay.at("d3", y * hout + x if valid else 0)
                    out += service(addr, 8)
    return out


# ------------------------------------------------------------------------------------------ element-wise passes, dense, z-bar
def elementwise(lay, name, n):
    """thread t touches packed elements t, t + 512, ... (copy-outs, the elu' passes, the squared-error pass)"""
    out = []
    for i0 in range(0, n, NT):
        def addr(t, i0=i0):
            i = i0 + t
            return lay.at(name, i >> 3, i & 7) if i < n and lay.stride[name] >= 8 else (lay.at(name, i) if i < n else None)
        out += service(addr, 8)
    return out


def dense(lay, what):
    out = []
    for i in range(lay.L):
        def addr(t, i=i):
            if t >= 128:
                return None
            return (lay.offset["z"] + i) * 8 if what == "z" else (lay.offset["dense"] + i * 128 + t) * 8
        out += service(addr, 8)
    return out


def zbar(lay, what):
    out = []
    for k in range(16):
        def addr(t, k=k):
            i, j = t >> 3, (t & 7) + 8 * k
            if i >= lay.L:
                return None
            return (lay.offset["dh0"] + j) * 8 if what == "dh0" else (lay.offset["dense"] + i * 128 + j) * 8
        out += service(addr, 8)
    return out


# the three gathers the padded strides are for; (name, function of the layout)
PADDED = [("UpC2 data reverse: gathers of d2 (b64)", lambda l: gg_gather(l, "d2", 8, 14, 0)),
          ("UpC1 data reverse: gathers of d1 (b64)", lambda l: gg_gather(l, "d1", 4, 8, 1)),
          ("UpC3 forward: gathers of a2 (b128)", lambda l: fwd_gather(l, "a2", 14, 1, 1))]
OTHERS = [("dense: z (broadcast)", lambda l: dense(l, "z")),
          ("dense: weights", lambda l: dense(l, "w")),
          ("UpC1 forward: gathers of h0 (b128)", lambda l: fwd_gather(l, "h0", 4, 1, 8)),
          ("UpC1 forward: weights (b128)", lambda l: fwd_weights(l, 1, 4, 1, 8)),
          ("UpC1 forward: stores of a1", lambda l: fwd_store(l, "a1", 4, 1, 8)),
          ("UpC2 forward: gathers of a1 (b128)", lambda l: fwd_gather(l, "a1", 8, 0, 8)),
          ("UpC2 forward: weights (b128)", lambda l: fwd_weights(l, 2, 8, 0, 8)),
          ("UpC2 forward: stores of a2", lambda l: fwd_store(l, "a2", 8, 0, 8)),
          ("UpC3 forward: weights (b128)", lambda l: fwd_weights(l, 3, 14, 1, 1)),
          ("UpC3 forward: stores of recon", lambda l: fwd_store(l, "d3", 14, 1, 1)),
          ("copy-outs: h0, a1", lambda l: elementwise(l, "h0", 128) + elementwise(l, "a1", 512)),
          ("copy-out: a2", lambda l: elementwise(l, "a2", 1568)),
          ("squared error, d3 in place (read + write)", lambda l: 2 * elementwise(l, "d3", 784)),
          ("UpC3 data reverse (bwd_data_valu): reads of d3", lambda l: valu_rev(l, "d3")),
          ("UpC3 data reverse (bwd_data_valu): weights", lambda l: valu_rev(l, "weights")),
          ("UpC3 data reverse (bwd_data_valu): stores of d2", lambda l: valu_rev(l, "store")),
          ("d2 elu' pass: d2 (read + write), a2", lambda l: 2 * elementwise(l, "d2", 1568) + elementwise(l, "a2", 1568)),
          ("UpC2 data reverse: B operands (weights)", lambda l: gg_weights(l, 2, 0)),
          ("UpC2 data reverse: stores of d1", lambda l: gg_store(l, "d1", 8)),
          ("d1 elu' pass: d1 (read + write), a1", lambda l: 2 * elementwise(l, "d1", 512) + elementwise(l, "a1", 512)),
          ("UpC1 data reverse: B operands (weights)", lambda l: gg_weights(l, 1, 1)),
          ("UpC1 data reverse: stores of dh0", lambda l: gg_store(l, "dh0", 4)),
          ("z-bar: dh0", lambda l: zbar(l, "dh0")),
          ("z-bar: dense weights", lambda l: zbar(l, "w"))]


def summary(degrees):
    """(service groups, mean degree, maximum degree, passes beyond one per group)"""
    n = len(degrees)
    return n, sum(degrees) / n, max(degrees), sum(degrees) - n


def table(lay, accesses=None):
    return [(name,) + summary(fn(lay)) for name, fn in (accesses or PADDED + OTHERS)]


def render(title, rows):
    lines = [title, f"{'access group (one image)':56s}{'groups':>8s}{'mean':>8s}{'max':>6s}{'extra passes':>14s}"]
    for name, n, mean, mx, extra in rows:
        lines.append(f"{name:56s}{n:8d}{mean:8.2f}{mx:6d}{extra:14d}")
    lines.append(f"{'all':56s}{sum(r[1] for r in rows):8d}{'':8s}{'':6s}{sum(r[4] for r in rows):14d}")
    return "\n".join(lines)


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import svgp_vae_amd
    lib = svgp_vae_amd.load_library()
    L = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    print(render(f"packed activations (8 doubles per pixel), L = {L}", table(packed_layout(lib, L))))
    lay = library_layout(lib, L)
    print()
    print(render(f"the library's layout: pixel strides d2 {lay.stride['d2']}, d1 {lay.stride['d1']}, a2 {lay.stride['a2']}, L = {L}", table(lay)))


if __name__ == "__main__":
    main()
