"""The small glue kernels behind the ball and SPRITES drivers (ball.hip, gp_sprites.hip, optim.hip, ...), each called through the C
ABI on its own and compared with a plain float64 restatement on the CPU (numpy longdouble for sums), at the sizes where their
loops and tiles end: one element, one short of / exactly / one past a 256-thread workgroup or a 16-wide tile, more than one
workgroup, and sizes the drivers never reach.

Every output buffer is NaN before the call (an element the kernel does not write fails the comparison) and carries GUARD
elements of a known pattern behind it, which must come back untouched.

Bounds (none of them measured):
  copies, layouts, single IEEE operations, act = 0 paths     bit-equal
  element-wise exp / tanh / log / log1p / sigmoid            8 ulp of the reference value (device and host libm may round differently)
  a sum of n terms                                           2^-52 (n + 8) sum |term|, the absolute terms summed in longdouble: holds
                                                             for any summation order (which costs (n - 1) / 2 of it) and leaves the
                                                             rest to the rounding of the terms themselves
  float32 variants                                           the same with 2^-23
A result that is a function of a sum (softmax: the log of one, a quotient by one) takes these rules stage by stage.  Two bounds are
wider, because no correct implementation can meet the plain ones: the SE kernel (the rounding of the exponent, which exp magnifies
by |exponent|) and the Adam update (the rounding of b^t, which 1 - b^t magnifies by b^t / (1 - b^t)); both are derived at the test.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
GUARD = 64
EPS = {F64: 2.0 ** -52, F32: 2.0 ** -23}
LD = np.longdouble


_LIVE = []          # device copies made by dev() for the call being assembled: kept alive until it has run


def _call(name, *args):
    from svgp_vae_amd._lib import call
    try:
        call(name, *args, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        _LIVE.clear()


def _guard(dtype):
    return torch.arange(1, GUARD + 1, dtype=dtype) * -3.25


class Buf:
    """n elements on the device followed by GUARD elements of a known pattern.  Buf(n) is an output (NaN before the call);
    Buf(data=t) holds t (an input, or an in-place operand)."""

    def __init__(self, n=None, dtype=F64, data=None):
        if data is not None:
            data = data.contiguous().reshape(-1)
            n, dtype = data.numel(), data.dtype
        else:
            data = torch.full((n,), float("nan"), dtype=dtype)
        self.n, self.dtype = n, dtype
        self.t = torch.cat([data, _guard(dtype)]).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self, *shape):
        h = self.t.cpu()
        assert torch.equal(h[self.n:], _guard(self.dtype)), "the kernel wrote behind its output"
        return h[:self.n].reshape(*shape) if shape else h[:self.n]


def dev(t):
    _LIVE.append(t.contiguous().cuda())
    return _LIVE[-1]


def ulps(got, ref):
    """|got - ref| in units of the spacing of the reference value; an exact match (infinities included) is 0."""
    got, ref = np.asarray(got), np.asarray(ref)
    with np.errstate(invalid="ignore"):
        d = np.abs(got.astype(LD) - ref.astype(LD)) / np.spacing(np.abs(ref)).astype(LD)
    return np.where(got == ref, 0.0, d).astype(np.float64)


def assert_ulps(got, ref, n, what):
    u = ulps(got.numpy(), ref.numpy())
    worst = float(np.nanmax(u)) if u.size else 0.0
    print(f"{what}: worst {worst:.2f} ulp (bound {n})")
    assert not np.isnan(u).any() and worst <= n, f"{what}: {worst} ulp"


def assert_within(got, ref, bound, what):
    """|got - ref| <= bound element-wise; ref and bound may be longdouble arrays."""
    got = np.asarray(got, dtype=LD)
    err = np.abs(got - np.asarray(ref, dtype=LD))
    bound = np.asarray(bound, dtype=LD)
    ratio = float(np.max(err / np.maximum(bound, np.finfo(LD).tiny))) if err.size else 0.0
    print(f"{what}: worst error / bound {ratio:.3f}")
    assert not np.isnan(err).any(), f"{what}: NaN"
    assert np.all(err <= bound), f"{what}: error / bound up to {ratio}"


def rnd(gen, *shape, dtype=F64):
    return torch.randn(*shape, dtype=dtype, generator=gen)


# ---------------------------------------------------------------------------------------------------------
# dense-layer glue
# ---------------------------------------------------------------------------------------------------------
ROWS, COLS = (1, 15, 16, 17, 1000), (1, 4, 15, 16, 17, 33, 500)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("rows", ROWS)
def test_bias_act_fwd(rows, act):
    g = torch.Generator().manual_seed(rows * 2 + act)
    for Cc in COLS:
        x, bias = rnd(g, rows, Cc) * 1.5, rnd(g, Cc)
        b = Buf(data=x)
        _call("svgp_bias_act_fwd", rows, Cc, act, dev(bias).data_ptr(), b.ptr)
        pre = x + bias
        if act == 0:
            assert torch.equal(b.get(rows, Cc), pre), (rows, Cc)
        else:
            assert_ulps(b.get(rows, Cc), torch.tanh(pre), 8, f"tanh rows {rows} C {Cc}")


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("rows", ROWS)
def test_act_bwd_bias(rows, act):
    """dpre = dout * (1 - out^2) in place for tanh, dout untouched for act = 0 (out may be NULL): a sum of the two terms dout and
    -dout out^2.  db = the column sums of dpre as stored: rows terms each, compared with the longdouble sums of the stored values."""
    g = torch.Generator().manual_seed(100 + rows * 2 + act)
    for Cc in COLS:
        out, dout = torch.tanh(rnd(g, rows, Cc) * 2), rnd(g, rows, Cc)
        d, db = Buf(data=dout), Buf(Cc)
        _call("svgp_act_bwd_bias", rows, Cc, act, dev(out).data_ptr() if act else None, d.ptr, None, db.ptr)
        if act == 0:
            assert torch.equal(d.get(rows, Cc), dout), (rows, Cc)
            terms = dout.numpy().astype(LD)
        else:
            want = dout * (1 - out * out)
            tol = (2 + 8) * EPS[F64] * (dout.abs() + (dout * out * out).abs())
            dpre = d.get(rows, Cc)
            assert_within(dpre.numpy(), want.numpy(), tol.numpy(), f"dpre rows {rows} C {Cc}")
            terms = dpre.numpy().astype(LD)
        bound = EPS[F64] * (rows + 8) * np.abs(terms).sum(0)
        assert_within(db.get().numpy(), terms.sum(0), bound, f"db rows {rows} C {Cc} act {act}")


# ---------------------------------------------------------------------------------------------------------
# encoder heads: mu, var_raw = exp, var = clip(var_raw); reverse with the tf.clip_by_value mask (bounds included)
# ---------------------------------------------------------------------------------------------------------
def _var_raw_with_edges(gen, shape, lo, hi):
    """Values below, inside and above [lo, hi], some equal to a bound to the bit and some one spacing outside it."""
    v = torch.exp(torch.empty(shape, dtype=F64).uniform_(math.log(lo) - 5, math.log(hi) + 5, generator=gen))
    flat = v.reshape(-1)
    edge = [lo, hi, float(np.nextafter(lo, 0)), float(np.nextafter(hi, np.inf)), float(np.nextafter(lo, 1)),
            float(np.nextafter(hi, 0))]
    for k in range(flat.numel()):
        if k % 3 == 0:
            flat[k] = edge[(k // 3) % len(edge)]
    return v


@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("B,T", [(1, 1), (5, 12), (64, 64)])
def test_ball_head_fwd_bwd(B, T, clip):
    lo, hi = 1e-6, 1e3
    g = torch.Generator().manual_seed(B * T + clip)
    h = torch.cat([rnd(g, B * T, 2), torch.empty(B * T, 2, dtype=F64).uniform_(-20, 10, generator=g)], 1)   # exp: 2e-9 .. 2e4
    bias = rnd(g, 4) * 0.1
    o = [Buf(B * T) for _ in range(6)]                  # mu_x, var_raw_x, var_x, mu_y, var_raw_y, var_y, each (T, B)
    _call("svgp_ball_head_fwd", B, T, clip, dev(bias).data_ptr(), dev(h).data_ptr(), *[b.ptr for b in o])
    pre = (h + bias).reshape(B, T, 4)
    for c in range(2):
        mu, var_raw, var = (o[3 * c + k].get(T, B) for k in range(3))
        assert torch.equal(mu, pre[:, :, c].t())                                      # the transposed (T, B) channel layout
        assert_ulps(var_raw, torch.exp(pre[:, :, 2 + c]).t(), 8, f"ball head var_raw {c}")
        assert torch.equal(var, torch.clamp(var_raw, lo, hi) if clip else var_raw)
        if clip and B * T > 1:
            assert (var_raw < lo).any() and (var_raw > hi).any() and ((var_raw > lo) & (var_raw < hi)).any()
    # reverse: var_raw is an input here, so the bounds themselves can be hit to the bit
    vr = [_var_raw_with_edges(g, (T, B), lo, hi) for _ in range(2)]
    yb, sb = [rnd(g, T, B) for _ in range(2)], [rnd(g, T, B) for _ in range(2)]
    dh = Buf(B * T * 4)
    _call("svgp_ball_head_bwd", B, T, clip, dev(vr[0]).data_ptr(), dev(yb[0]).data_ptr(), dev(sb[0]).data_ptr(),
          dev(vr[1]).data_ptr(), dev(yb[1]).data_ptr(), dev(sb[1]).data_ptr(), dh.ptr)
    got = dh.get(B, T, 4)
    for c in range(2):
        mask = ((vr[c] >= lo) & (vr[c] <= hi)) if clip else torch.ones_like(vr[c], dtype=torch.bool)
        assert torch.equal(got[:, :, c], yb[c].t())
        assert torch.equal(got[:, :, 2 + c], torch.where(mask, sb[c] * vr[c], torch.zeros_like(sb[c])).t())


@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("b,L", [(1, 1), (7, 3), (300, 64)])
def test_enc_head_fwd_bwd(b, L, clip):
    lo, hi = 1e-3, 10.0
    g = torch.Generator().manual_seed(b * L + clip)
    enc = torch.cat([rnd(g, b, L), torch.empty(b, L, dtype=F64).uniform_(-12, 7, generator=g)], 1)          # exp: 6e-6 .. 1e3
    bias = rnd(g, 2 * L) * 0.1
    e, mu, var_raw, var = Buf(data=enc), Buf(b * L), Buf(b * L), Buf(b * L)
    _call("svgp_enc_head_fwd", b, L, clip, dev(bias).data_ptr(), e.ptr, mu.ptr, var_raw.ptr, var.ptr)
    pre = enc + bias
    assert torch.equal(e.get(b, 2 * L), pre)                                          # the bias add happens in place
    assert torch.equal(mu.get(b, L), pre[:, :L])
    vr = var_raw.get(b, L)
    assert_ulps(vr, torch.exp(pre[:, L:]), 8, "enc head var_raw")
    assert torch.equal(var.get(b, L), torch.clamp(vr, lo, hi) if clip else vr)
    if clip and b * L > 1:
        assert (vr < lo).any() and (vr > hi).any() and ((vr > lo) & (vr < hi)).any()
    vr, yb, sb = _var_raw_with_edges(g, (b, L), lo, hi), rnd(g, b, L), rnd(g, b, L)
    d = Buf(b * 2 * L)
    _call("svgp_enc_head_bwd", b, L, clip, dev(vr).data_ptr(), dev(yb).data_ptr(), dev(sb).data_ptr(), d.ptr)
    mask = ((vr >= lo) & (vr <= hi)) if clip else torch.ones_like(vr, dtype=torch.bool)
    assert torch.equal(d.get(b, 2 * L), torch.cat([yb, torch.where(mask, sb * vr, torch.zeros_like(sb))], 1))


# ---------------------------------------------------------------------------------------------------------
# copies and single operations: bit-equal
# ---------------------------------------------------------------------------------------------------------
SIZES = (1, 255, 256, 257, 65541)


# pack / unpack move 2 B T elements, so the odd sizes 1, 255, 257 of the other copies cannot occur: 2, 510, 256, 514 and 65 538
# elements end at the same workgroup edges (one thread per element, 256 per workgroup)
@pytest.mark.parametrize("B,T", [(1, 1), (5, 51), (2, 64), (257, 1), (3, 10923)])
def test_ball_pack_unpack(B, T):
    g = torch.Generator().manual_seed(B + T)
    zx, zy = rnd(g, T, B), rnd(g, T, B)
    z = Buf(B * T * 2)
    _call("svgp_ball_pack_z", B, T, dev(zx).data_ptr(), dev(zy).data_ptr(), z.ptr)
    assert torch.equal(z.get(B, T, 2), torch.stack([zx.t(), zy.t()], 2))
    dz = rnd(g, B, T, 2)
    bx, by = Buf(B * T), Buf(B * T)
    _call("svgp_ball_unpack_zbar", B, T, dev(dz).data_ptr(), bx.ptr, by.ptr)
    assert torch.equal(bx.get(T, B), dz[:, :, 0].t()) and torch.equal(by.get(T, B), dz[:, :, 1].t())


@pytest.mark.parametrize("rows,Cc", [(1, 1), (5, 51), (16, 16), (257, 1), (1, 257), (7, 9363)])
def test_scale_rows_and_bias_add(rows, Cc):
    g = torch.Generator().manual_seed(rows + Cc)
    x, w, bias = rnd(g, rows, Cc), rnd(g, rows), rnd(g, Cc)
    b = Buf(data=x)
    _call("svgp_scale_rows", rows, Cc, dev(w).data_ptr(), b.ptr)
    assert torch.equal(b.get(rows, Cc), x * w[:, None])
    b = Buf(data=x)
    _call("svgp_bias_add", rows, Cc, dev(bias).data_ptr(), b.ptr)
    assert torch.equal(b.get(rows, Cc), x + bias)
    x32, bias32 = x.to(F32), bias.to(F32)
    b = Buf(data=x32)
    _call("svgp_bias_add_f32", rows, Cc, dev(bias32).data_ptr(), b.ptr)
    assert torch.equal(b.get(rows, Cc), x32 + bias32)


@pytest.mark.parametrize("n", SIZES)
def test_scale_by_device_scalar_and_casts(n):
    g = torch.Generator().manual_seed(n)
    x, f = rnd(g, n) * 1e3, rnd(g, 1)
    b = Buf(data=x)
    _call("svgp_scale_by_device_scalar", n, dev(f).data_ptr(), b.ptr)
    assert torch.equal(b.get(), x * f)
    y32 = Buf(n, F32)
    _call("svgp_cast_f64_f32", n, dev(x).data_ptr(), y32.ptr)
    assert torch.equal(y32.get(), x.to(F32))
    y64 = Buf(n, F64)
    _call("svgp_cast_f32_f64", n, dev(x.to(F32)).data_ptr(), y64.ptr)
    assert torch.equal(y64.get(), x.to(F32).to(F64))


def test_state_add():
    from svgp_vae_amd._lib import STATE, STATE_LEN, SvgpError
    st0 = torch.arange(STATE_LEN, dtype=F64) * 1.5 + 0.25
    st = Buf(data=st0)
    _call("svgp_state_add", st.ptr, STATE["RNG_CTR"], 3.0)
    _call("svgp_state_add", st.ptr, 0, -0.125)
    want = st0.clone()
    want[STATE["RNG_CTR"]] += 3.0
    want[0] += -0.125
    assert torch.equal(st.get(), want)
    for slot in (-1, STATE_LEN):
        with pytest.raises(SvgpError):
            _call("svgp_state_add", st.ptr, slot, 1.0)
    assert torch.equal(st.get(), want)


# ---------------------------------------------------------------------------------------------------------
# Bernoulli and softmax cross-entropies
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["all", "no_pred", "no_dlogits"])
@pytest.mark.parametrize("rows", [1, 7])
def test_sigmoid_xent(rows, form):
    """Per row -sum_pix [max(x,0) - x z + log1p(exp(-|x|))]: a sum of 3 P terms.  sigmoid: an element-wise function, 8 ulp.
    dlogits = scale (sigmoid - z): a sum of two terms."""
    scale = 1.0 / 7
    special = torch.tensor([0.0, 1e-300, -1e-300, 40.0, -40.0, 800.0, -800.0], dtype=F64)
    for P in (1, 255, 256, 257, 1024):
        g = torch.Generator().manual_seed(rows * 2000 + P)
        x = rnd(g, rows, P) * 4
        z = torch.randint(0, 2, (rows, P), generator=g).to(F64)
        z[:, 1::3] = torch.rand(rows, len(range(1, P, 3)), dtype=F64, generator=g)             # fractional labels too
        k = torch.arange(rows * P).reshape(rows, P)
        x = torch.where(k % 5 == 0, special[(k // 5) % 7], x) if P > 1 else special[:rows].reshape(rows, 1).clone()
        pred, rr, dl = Buf(rows * P), Buf(rows), Buf(rows * P)
        _call("svgp_sigmoid_xent", rows, P, scale, dev(x).data_ptr(), dev(z).data_ptr(),
              None if form == "no_pred" else pred.ptr, rr.ptr, None if form == "no_dlogits" else dl.ptr)
        xl, zl = x.numpy().astype(LD), z.numpy().astype(LD)
        t1, t2, t3 = np.maximum(xl, 0), -xl * zl, np.log1p(np.exp(-np.abs(xl)))
        want = -(t1 + t2 + t3).sum(1)
        bound = EPS[F64] * (3 * P + 8) * (np.abs(t1) + np.abs(t2) + np.abs(t3)).sum(1)
        got = rr.get()
        assert torch.isfinite(got).all()
        assert_within(got.numpy(), want, bound, f"row_recon rows {rows} P {P}")
        sg = torch.sigmoid(x)
        if form == "no_pred":
            assert torch.isnan(pred.get()).all()
        else:
            assert_ulps(pred.get(rows, P), sg, 8, f"sigmoid rows {rows} P {P}")
        if form == "no_dlogits":
            assert torch.isnan(dl.get()).all()
        else:
            tol = scale * EPS[F64] * (2 + 8) * (sg + z)
            assert_within(dl.get(rows, P).numpy(), (scale * (sg - z)).numpy(), tol.numpy(), f"dlogits rows {rows} P {P}")


@pytest.mark.parametrize("n,Cc", [(1, 1), (3, 2), (5, 255), (5, 257), (4, 1000)])
def test_softmax_xent(n, Cc):
    """No output is a plain sum, so the rules of the header apply stage by stage.  se = sum_c exp(z_c - mx), a sum of C terms, is good
    to a relative 2^-52 (C + 8), which is also the absolute error it leaves in log(se); log adds 8 ulp of its value; row_loss =
    log(se) + mx - z[label] is a sum of three terms.  softmax_c = exp(z_c - mx) / se: 8 ulp of exp and the relative error of se;
    dlogits = (softmax - onehot) / n is a sum of two terms.  loss: the mean of the n row losses as stored."""
    g = torch.Generator().manual_seed(n * 1000 + Cc)
    z = rnd(g, n, Cc) * 3
    z += torch.tensor([0.0, 700.0, -700.0, 30.0, -5.0], dtype=F64)[:n, None]            # rows shifted by +-700
    lab = torch.randint(0, Cc, (n,), generator=g)
    lab[0] = Cc - 1                                                                     # the last class
    if n > 1:
        lab[1] = 0                                                                      # the first
    row, loss, dl = Buf(n), Buf(1), Buf(n * Cc)
    _call("svgp_softmax_xent", n, Cc, dev(z).data_ptr(), dev(lab.to(F64)).data_ptr(), row.ptr, loss.ptr, dl.ptr)
    zl = z.numpy().astype(LD)
    mx = zl.max(1, keepdims=True)
    ex = np.exp(zl - mx)
    se = ex.sum(1)
    zlab = zl[np.arange(n), lab.numpy()]
    want_row = np.log(se) + mx[:, 0] - zlab
    row_bound = EPS[F64] * ((Cc + 8) + 8 * np.abs(np.log(se)) + (3 + 8) * (np.abs(np.log(se)) + np.abs(mx[:, 0]) + np.abs(zlab)))
    got_row = row.get().numpy().astype(LD)
    assert_within(got_row, want_row, row_bound, f"row_loss n {n} C {Cc}")
    assert_within(loss.get().numpy(), got_row.sum(keepdims=True) / n, EPS[F64] * (n + 8) * np.abs(got_row).sum() / n,
                  f"loss n {n} C {Cc}")
    sm = ex / se[:, None]
    onehot = np.zeros((n, Cc), dtype=LD)
    onehot[np.arange(n), lab.numpy()] = 1
    d_bound = EPS[F64] * ((8 + Cc + 8) * sm + (2 + 8) * (sm + onehot)) / n
    assert_within(dl.get(n, Cc).numpy(), (sm - onehot) / n, d_bound, f"dlogits n {n} C {Cc}")


# ---------------------------------------------------------------------------------------------------------
# Gaussian cross-entropy, squared error
# ---------------------------------------------------------------------------------------------------------
PART_CASES = [(n_part, tot) for n_part in (1, 3, 256) for tot in (256 * n_part - 1, 256 * n_part, 256 * n_part + 1)] + \
             [(1, 1), (3, 70001), (256, 5)]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_gauss_cross_entropy(n):
    """-1/2 (log 2pi + log v2 + (v1 + a^2 - 2ab + b^2) / v2): a sum of six terms."""
    g = torch.Generator().manual_seed(n)
    a, b = rnd(g, n), rnd(g, n)
    v1, v2 = torch.exp(rnd(g, n)), torch.exp(rnd(g, n) * 2)
    out = Buf(n)
    _call("svgp_gauss_cross_entropy", n, *(dev(t).data_ptr() for t in (a, v1, b, v2)), out.ptr)
    al, bl, v1l, v2l = (t.numpy().astype(LD) for t in (a, b, v1, v2))
    terms = [np.full(n, math.log(2 * math.pi), dtype=LD), np.log(v2l), v1l / v2l, al * al / v2l, -2 * al * bl / v2l, bl * bl / v2l]
    want = -0.5 * sum(terms)
    bound = 0.5 * EPS[F64] * (6 + 8) * sum(np.abs(t) for t in terms)
    assert_within(out.get().numpy(), want, bound, f"gauss ce n {n}")


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n_part,tot", PART_CASES)
def test_sqerr_fwd(n_part, tot, dtype):
    """n_part workgroups stride over tot elements and leave their partial sums of (x - xhat)^2 in part_sums[blk * 4 + 2]; no
    other slot of the partial-sum area may change.  The float32 variant forms the differences and their squares in float64
    (x is large against xhat, so a float32 difference would be off by 2^-24 relative: far outside the bound).  The total is a sum of
    tot terms."""
    g = torch.Generator().manual_seed(n_part * 100000 + tot)
    x, xh = (rnd(g, tot) * 1000).to(dtype), rnd(g, tot).to(dtype)
    before = rnd(g, n_part, 4)
    before[:, 2] = float("nan")
    ps = Buf(data=before)
    _call("svgp_sqerr_fwd" + ("_f32" if dtype == F32 else ""), tot, n_part, dev(x).data_ptr(), dev(xh).data_ptr(), ps.ptr)
    after = ps.get(n_part, 4)
    keep = [0, 1, 3]
    assert torch.equal(after[:, keep], before[:, keep])
    part = after[:, 2]
    assert torch.isfinite(part).all() and (part >= 0).all()
    assert (part[(tot + 255) // 256:] == 0).all()                       # a workgroup with no element writes 0
    d2 = (x.numpy().astype(LD) - xh.numpy().astype(LD)) ** 2
    total = part.numpy().astype(LD).sum()                               # n_part more additions, in longdouble
    assert_within(total, d2.sum(), EPS[F64] * (tot + 8) * d2.sum(), f"sqerr n_part {n_part} tot {tot}")


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("geco", [0, 1])
@pytest.mark.parametrize("tot", [1, 255, 256, 257, 70001])
def test_sqerr_bwd(tot, geco, dtype):
    """dxhat = 2 gscale (xhat - x), gscale = (geco ? lagrange / b_global : 1) / n_pix, evaluated in float64 through the
    reciprocals 1 / b_global and 1 / n_pix: up to seven roundings -> 8 ulp (float32 variant: rounded once more, to float32)."""
    from svgp_vae_amd._lib import STATE, STATE_LEN
    g = torch.Generator().manual_seed(tot * 2 + geco)
    x, xh = (rnd(g, tot) * 1000).to(dtype), rnd(g, tot).to(dtype)
    st = torch.arange(STATE_LEN, dtype=F64) + 0.5
    st[STATE["LAGRANGE"]] = 2.7
    b_global, n_pix = 37, 12288
    out = Buf(tot, dtype)
    _call("svgp_sqerr_bwd" + ("_f32" if dtype == F32 else ""), tot, geco, b_global, n_pix, dev(st).data_ptr(),
          dev(x).data_ptr(), dev(xh).data_ptr(), out.ptr)
    want = 2.0 * ((2.7 / b_global) if geco else 1.0) / n_pix * (xh.to(F64) - x.to(F64))
    if dtype == F64:
        assert_ulps(out.get(), want, 8, f"sqerr bwd tot {tot}")
    else:
        assert_ulps(out.get(), want.to(F32), 1, f"sqerr bwd f32 tot {tot}")


# ---------------------------------------------------------------------------------------------------------
# average pooling, SPRITES auxiliary data (segment means)
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,HW,Cc", [(1, 1, 1), (3, 64, 16), (5, 49, 7), (2, 100, 33)])
def test_avgpool(n, HW, Cc, dtype):
    g = torch.Generator().manual_seed(n * HW * Cc)
    sfx = "_f32" if dtype == F32 else ""
    x = rnd(g, n, HW, Cc).to(dtype)
    y = Buf(n * Cc, dtype)
    _call("svgp_avgpool_fwd" + sfx, n, HW, Cc, dev(x).data_ptr(), y.ptr)
    xl = x.numpy().astype(LD)
    assert_within(y.get(n, Cc).numpy(), xl.sum(1) / HW, EPS[dtype] * (HW + 8) * np.abs(xl).sum(1) / HW, f"avgpool {n} {HW} {Cc}")
    dy = rnd(g, n, Cc).to(dtype)
    dx = Buf(n * HW * Cc, dtype)
    _call("svgp_avgpool_bwd" + sfx, n, HW, Cc, dev(dy).data_ptr(), dx.ptr)
    assert torch.equal(dx.get(n, HW, Cc), (dy / HW)[:, None, :].expand(n, HW, Cc))    # one division: bit-equal


@pytest.mark.parametrize("b,seg_len,Lc", [(4, 1, 3), (8, 8, 16), (24, 8, 5), (30, 3, 64)])
def test_sprites_aux(b, seg_len, Lc):
    g = torch.Generator().manual_seed(b * seg_len * Lc)
    rep, ids = rnd(g, b, Lc), torch.randint(0, 9, (b,), generator=g).to(F64)
    aux = Buf(b * (1 + Lc))
    _call("svgp_sprites_aux_fwd", b, seg_len, Lc, dev(rep).data_ptr(), dev(ids).data_ptr(), aux.ptr)
    got = aux.get(b, 1 + Lc)
    assert torch.equal(got[:, 0], ids)

    def seg_mean(t):
        tl = t.numpy().astype(LD).reshape(b // seg_len, seg_len, Lc)
        mean = np.repeat(tl.sum(1) / seg_len, seg_len, axis=0)
        return mean, EPS[F64] * (seg_len + 8) * np.repeat(np.abs(tl).sum(1) / seg_len, seg_len, axis=0)

    assert_within(got[:, 1:].numpy(), *seg_mean(rep), f"sprites aux fwd {b} {seg_len} {Lc}")
    d_char = rnd(g, b, Lc)
    d_rep = Buf(b * Lc)
    _call("svgp_sprites_aux_bwd", b, seg_len, Lc, dev(d_char).data_ptr(), d_rep.ptr)
    assert_within(d_rep.get(b, Lc).numpy(), *seg_mean(d_char), f"sprites aux bwd {b} {seg_len} {Lc}")


def test_sprites_aux_rejects_a_batch_that_is_no_multiple_of_the_segment():
    from svgp_vae_amd._lib import SvgpError
    x = torch.zeros(64, dtype=F64).cuda()
    for fn, args in (("svgp_sprites_aux_fwd", (x.data_ptr(), x.data_ptr(), x.data_ptr())),
                     ("svgp_sprites_aux_bwd", (x.data_ptr(), x.data_ptr()))):
        with pytest.raises(SvgpError):
            _call(fn, 10, 4, 2, *args)


# ---------------------------------------------------------------------------------------------------------
# SE kernel on scalar times and its reverse
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,m", [(1, 1), (30, 15), (257, 64), (5, 300)])
def test_se1d_kernel_matrix(T, m):
    """K = exp(-(x - z)^2 / (2 l^2)).  The kernels evaluate the exponent as d d (-0.5 / l^2), the reference as -d^2 / (2 l^2):
    up to four roundings apart, which exp turns into a relative 4 ulp |exponent|, on top of its own 8 ulp.
    Reverse against autograd with random (non-symmetric) Kbar and Knbar: d_z[i] is a sum of 2 m + T terms, d_l of m m + T m, and
    each term holds that exp -> 2^-52 (n + 8 + 4 |exponent|) |term|, summed in longdouble."""
    g = torch.Generator().manual_seed(T * 1000 + m)
    x = torch.arange(1, T + 1, dtype=F64)
    z = torch.linspace(1, max(T, 2), m, dtype=F64) + 0.1 * rnd(g, m)
    ls = torch.tensor([1.7], dtype=F64)
    K, Kn, knn = Buf(m * m), Buf(T * m), Buf(T)
    _call("svgp_se1d_kernel_matrix_fwd", T, m, dev(x).data_ptr(), dev(z).data_ptr(), dev(ls).data_ptr(), K.ptr, Kn.ptr, knn.ptr)
    zr, lr = z.clone().requires_grad_(True), ls.clone().requires_grad_(True)
    se = lambda a, b: torch.exp(-(a[:, None] - b[None, :]) ** 2 / (2 * lr * lr))
    Kw, Knw = se(zr, zr), se(x, zr)
    for got, want, a, b in ((K.get(m, m), Kw, z, z), (Kn.get(T, m), Knw, x, z)):
        want = want.detach()
        arg = (a[:, None] - b[None, :]) ** 2 / (2 * ls * ls)
        tol = (8 + 4 * arg) * torch.from_numpy(np.spacing(want.numpy()))
        assert_within(got.numpy(), want.numpy(), tol.numpy(), f"se1d fwd T {T} m {m}")
    assert torch.equal(knn.get(), torch.ones(T, dtype=F64))
    Kbar, Knbar = rnd(g, m, m), rnd(g, T, m)
    gz, gl = torch.autograd.grad((Kw * Kbar).sum() + (Knw * Knbar).sum(), [zr, lr])
    d_z, d_l = Buf(m), Buf(1)
    _call("svgp_se1d_kernel_matrix_bwd", T, m, dev(x).data_ptr(), dev(z).data_ptr(), dev(ls).data_ptr(), dev(Kbar).data_ptr(),
          dev(Knbar).data_ptr(), d_z.ptr, d_l.ptr)
    zl, xl, l = z.numpy().astype(LD), x.numpy().astype(LD), LD(1.7)
    dzz, dxz = zl[:, None] - zl[None, :], xl[:, None] - zl[None, :]
    azz, axz = dzz ** 2 / (2 * l * l), dxz ** 2 / (2 * l * l)
    Kb, Knb = Kbar.numpy().astype(LD), Knbar.numpy().astype(LD)
    tzz, txz = np.abs(Kb * np.exp(-azz) * dzz), np.abs(Knb * np.exp(-axz) * dxz)      # |term| l^2 of d_z, |term| l^3 / |d| of d_l
    n_z, n_l = 2 * m + T, m * m + T * m
    bz = ((tzz * (n_z + 8 + 4 * azz)).sum(1) + (tzz * (n_z + 8 + 4 * azz)).sum(0) + (txz * (n_z + 8 + 4 * axz)).sum(0)) / (l * l)
    bl = ((tzz * np.abs(dzz) * (n_l + 8 + 4 * azz)).sum() + (txz * np.abs(dxz) * (n_l + 8 + 4 * axz)).sum()) / l ** 3
    assert_within(d_z.get().numpy(), gz.numpy(), EPS[F64] * bz, f"se1d d_z T {T} m {m}")
    assert_within(d_l.get().numpy(), gl.numpy(), EPS[F64] * bl, f"se1d d_l T {T} m {m}")


# ---------------------------------------------------------------------------------------------------------
# ball frames
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("px,py", [(8, 8), (5, 9), (9, 5)])
def test_ball_rasterize(px, py):
    """frame[i][j] = (i - x)^2 + (j - y)^2 < r^2 with i along px and j along py.  Centres are multiples of 1/8 and r of 1/2, so
    every square and sum is exact and the comparison cannot depend on how the sum is rounded or fused."""
    g = torch.Generator().manual_seed(px * 10 + py)
    fixed = torch.tensor([[2.0, 3.0], [0.0, 0.0], [px - 1.0, py - 1.0],               # on pixel centres (corners included)
                          [2.5, 3.5], [1.5, 2.0], [0.125, 4.875],                    # between pixels
                          [-3.0, 2.0], [px + 1.5, py + 2.0], [-0.5, -0.5], [2.0, py + 0.5], [-40.0, 100.0]], dtype=F64)
    paths = torch.cat([fixed, torch.randint(-16, 8 * max(px, py) + 16, (40, 2), generator=g).to(F64) / 8])
    frames = paths.shape[0]
    for r in (2.0, 2.5, 0.5):
        vid = Buf(frames * px * py)
        _call("svgp_ball_rasterize", frames, px, py, r, dev(paths).data_ptr(), vid.ptr)
        pn = paths.numpy()
        i, j = np.arange(px).reshape(1, px, 1), np.arange(py).reshape(1, 1, py)
        want = ((i - pn[:, 0, None, None]) ** 2 + (j - pn[:, 1, None, None]) ** 2 < r * r).astype(np.float64)
        got = vid.get(frames, px, py).numpy()
        assert np.array_equal(got, want), (px, py, r)
        assert want[:3].sum() > 0 and want[10].sum() == 0


# ---------------------------------------------------------------------------------------------------------
# gradient clip and TF1 Adam
# ---------------------------------------------------------------------------------------------------------
ADAM_N = (0, 1, 255, 257, 70001)


def _grad_with_edges(gen, n, thr):
    gr = rnd(gen, n) * thr * 2
    edge = [thr, -thr, float(np.nextafter(thr, np.inf)), float(np.nextafter(-thr, -np.inf)), float(np.nextafter(thr, 0)), 0.0, -0.0]
    for k in range(0, n, 3):
        gr[k] = edge[(k // 3) % len(edge)]
    return gr


@pytest.mark.parametrize("n", ADAM_N)
def test_clip_by_value(n):
    thr = 100000.0
    g = torch.Generator().manual_seed(n)
    gr = _grad_with_edges(g, n, thr)
    b = Buf(data=gr)
    _call("svgp_clip_by_value", n, thr, b.ptr)
    got = b.get()
    assert torch.equal(got, torch.clamp(gr, -thr, thr))
    if n > 100:
        assert (gr > thr).any() and (gr < -thr).any() and (gr.abs() < thr).any() and (gr == thr).any()


@pytest.mark.parametrize("n", ADAM_N)
def test_adam_tf1_three_steps(n):
    """tf.train.AdamOptimizer (TF 1.15): lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), m and v moments, theta -= lr_t m / (sqrt(v) + eps)
    with eps outside the square root; t = state[ADAM_T] + 1, and the counter is advanced by hand between the steps, as the drivers'
    finalize kernels do.  Each step is compared from the state the device itself left, so nothing compounds:
      m, v         two-term sums: 2^-52 (2 + 8) sum |term|
      the update   u = lr_t m / (sqrt(v) + eps) from the moments as stored: an element-wise expression, 8 ulp -- but for b^t: pow is
                   good to 16 ulp (the OpenCL bound the device libm follows; the host's own adds one), and 1 - b^t magnifies that by
                   q = b^t / (1 - b^t) (999 at b2 = 0.999, t = 1; halved by the square root), which no implementation can avoid
                   -> relative (8 + 17 (q1 + q2 / 2)) 2^-52
      theta        theta - u, a two-term sum, on top of the error of u."""
    from svgp_vae_amd._lib import STATE, STATE_LEN
    b1, b2, eps, lr, thr = 0.9, 0.999, 1e-8, 1e-3, 100000.0
    g = torch.Generator().manual_seed(n + 7)
    theta, mo, vo = Buf(data=rnd(g, n)), Buf(data=torch.zeros(n, dtype=F64)), Buf(data=torch.zeros(n, dtype=F64))
    st = torch.zeros(STATE_LEN, dtype=F64)
    st[STATE["LR"]] = lr
    for t in range(1, 4):
        st[STATE["ADAM_T"]] = t - 1.0
        state = Buf(data=st)
        gr = torch.clamp(_grad_with_edges(g, n, thr), -thr, thr) * (1e-5 if t == 2 else 1.0)
        th0, m0, v0 = theta.get().clone(), mo.get().clone(), vo.get().clone()
        grad = Buf(data=gr)
        _call("svgp_adam_tf1_step", n, theta.ptr, grad.ptr, mo.ptr, vo.ptr, state.ptr, b1, b2, eps)
        assert torch.equal(grad.get(), gr)                                   # ... and the gradient
        assert torch.equal(state.get(), st)                                  # the step reads the state and leaves it alone
        if n == 0:
            continue
        m1, v1 = b1 * m0 + (1 - b1) * gr, b2 * v0 + (1 - b2) * gr * gr
        assert_within(mo.get().numpy(), m1.numpy(), (10 * EPS[F64] * ((b1 * m0).abs() + ((1 - b1) * gr).abs())).numpy(), f"m t {t}")
        assert_within(vo.get().numpy(), v1.numpy(), (10 * EPS[F64] * v1).numpy(), f"v t {t}")
        lr_t = lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
        upd = lr_t * mo.get() / (torch.sqrt(vo.get()) + eps)
        q1, q2 = b1 ** t / (1 - b1 ** t), b2 ** t / (1 - b2 ** t)
        tol = EPS[F64] * ((8 + 17 * (q1 + q2 / 2)) * upd.abs() + (2 + 8) * (th0.abs() + upd.abs()))
        assert_within(theta.get().numpy(), (th0 - upd).numpy(), tol.numpy(), f"theta t {t}")


# ---------------------------------------------------------------------------------------------------------
# NaN and infinity through the clips: ordinary data, nothing faults; torch.clamp / tf.clip_by_value semantics
# ---------------------------------------------------------------------------------------------------------
def test_clip_by_value_keeps_nan_and_clips_infinities():
    thr = 100000.0
    gr = torch.tensor([float("nan"), float("inf"), -float("inf"), 1.0, -2e5, 3e5, float("nan")] * 41, dtype=F64)
    b = Buf(data=gr)
    _call("svgp_clip_by_value", gr.numel(), thr, b.ptr)
    got, want = b.get(), torch.clamp(gr, -thr, thr)
    assert torch.isnan(want[0]) and want[1] == thr and want[2] == -thr
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))


def test_enc_head_clip_keeps_nan_and_clips_infinities():
    b, L, lo, hi = 3, 2, 1e-3, 10.0
    nan, inf = float("nan"), float("inf")
    # variance pre-activations: exp(NaN) = NaN, exp(+inf) = +inf, exp(-inf) = 0, exp(800) = +inf
    enc = torch.tensor([[0.5, nan, nan, inf], [nan, 0.25, -inf, 800.0], [1.0, 2.0, 0.0, nan]], dtype=F64)
    e, mu, var_raw, var = Buf(data=enc), Buf(b * L), Buf(b * L), Buf(b * L)
    _call("svgp_enc_head_fwd", b, L, 1, dev(torch.zeros(2 * L, dtype=F64)).data_ptr(), e.ptr, mu.ptr, var_raw.ptr, var.ptr)
    want_raw = torch.exp(enc[:, L:])
    want = torch.clamp(want_raw, lo, hi)
    assert want.tolist()[1] == [lo, hi] and math.isnan(want[0, 0]) and want[0, 1] == hi and math.isnan(want[2, 1])
    for got, ref in ((mu.get(b, L), enc[:, :L]), (var_raw.get(b, L), want_raw), (var.get(b, L), want)):
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), (got, ref)
        assert torch.equal(torch.nan_to_num(got, nan=0.0, posinf=1e308, neginf=-1e308),
                           torch.nan_to_num(ref, nan=0.0, posinf=1e308, neginf=-1e308)), (got, ref)


def test_ball_head_clip_keeps_nan_and_clips_infinities():
    B, T, lo, hi = 2, 3, 1e-6, 1e3
    nan, inf = float("nan"), float("inf")
    h = torch.zeros(B * T, 4, dtype=F64)
    h[:, 2] = torch.tensor([nan, inf, -inf, 800.0, 0.0, nan], dtype=F64)
    h[:, 3] = torch.tensor([-800.0, nan, 1.0, nan, inf, -inf], dtype=F64)
    h[0, 0] = nan
    o = [Buf(B * T) for _ in range(6)]
    _call("svgp_ball_head_fwd", B, T, 1, dev(torch.zeros(4, dtype=F64)).data_ptr(), dev(h).data_ptr(), *[b.ptr for b in o])
    hh = h.reshape(B, T, 4)
    for c in range(2):
        want_raw = torch.exp(hh[:, :, 2 + c]).t()
        want = torch.clamp(want_raw, lo, hi)
        assert torch.isnan(want).sum() == 2 and (want == hi).sum() >= 1 and (want == lo).sum() >= 1
        for got, ref in ((o[3 * c].get(T, B), hh[:, :, c].t()), (o[3 * c + 1].get(T, B), want_raw), (o[3 * c + 2].get(T, B), want)):
            assert torch.equal(torch.isnan(got), torch.isnan(ref)), (got, ref)
            assert torch.equal(torch.nan_to_num(got, nan=0.0, posinf=1e308, neginf=-1e308),
                               torch.nan_to_num(ref, nan=0.0, posinf=1e308, neginf=-1e308)), (got, ref)
