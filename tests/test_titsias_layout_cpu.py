"""ws.Knbar_part under cfg.titsias: the Titsias reverse stage (svgp_gp_titsias_bwd) keeps W | cA | cB, b m + 2 b L elements, in that
field, which every other stage needs L b m of.  The layout gives it the larger of the two at the row capacity, so the stage's own
guard (a field too small is SVGP_ERR_INVALID) is reached by no shape svgp_check_cfg accepts -- L = 1, m <= 2 and (m = 3, L = 2) were
once refused there; without cfg.titsias the field is L b m as before; and with it the workspace grows only at those shapes."""
import ctypes as C
import itertools

from svgp_vae_amd import _lib

UP16 = lambda n: (n + 15) // 16 * 16


def _layout(**kw):
    wl = _lib.WsLayout()
    _lib.call("svgp_mnist_ws_layout_get", C.byref(_lib.MnistCfg(M=3, n_obj=0, N_train=4050.0, jitter=1e-4, **kw)), C.byref(wl))
    return wl


def test_knbar_part_holds_the_reverse_stage_at_every_accepted_shape():
    seen_small = 0
    for m, L, cap in itertools.product((1, 2, 3, 4, 5, 16, 32, 64, 65, 72, 520, 2048), (1, 2, 3, 4, 16, 63, 64), (1, 3, 60, 128, 257)):
        if m > 72 and cap > 60:
            continue
        for b in sorted({1, cap}):
            plain = _layout(b=b, b_global=b, b_cap=cap, m=m, L=L)
            tit = _layout(b=b, b_global=b, b_cap=cap, m=m, L=L, titsias=1)
            need = cap * m + 2 * cap * L
            assert plain.scr_bm - plain.Knbar_part == UP16(L * cap * m), (m, L, cap)
            assert tit.scr_bm - tit.Knbar_part == UP16(max(L * cap * m, need)), (m, L, cap)
            assert tit.scr_bm - tit.Knbar_part >= b * m + 2 * b * L
            small = (L - 1) * m < 2 * L
            assert small == (need > L * cap * m)
            seen_small += small
            # with cfg.titsias the field, and behind it the workspace, grows only at the shapes once refused
            grow = (tit.scr_bm - tit.Knbar_part) - (plain.scr_bm - plain.Knbar_part)
            assert grow >= 0 and (grow > 0) <= small, (m, L, cap)
            assert tit.total - tit.scr_bm == plain.total - plain.scr_bm + UP16(L * m * m) + UP16(L * m) + UP16(2 * L + 1)
    assert seen_small >= 20      # L = 1 at every m; m = 1, 2 at every L; (m 3, L 2)
