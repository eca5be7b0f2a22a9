"""Case tables, input builders and float64 references of the float32 streaming statistics (csrc/gp_stream_f32.hip:
svgp_stream_features_f32, svgp_stream_knm_f32, svgp_stream_stats_f32).  numpy only; tests/test_stream_cases_cpu.py guards the tables
without a GPU, tests/test_gpu_stream_f32_envelope.py runs them.

Two kinds of comparison, neither a relative limit against the largest element:

EXACT.  Inputs on which every float32 operation of the kernels is exact, so the result equals the float64 reference bit for bit
and a lost, doubled or misplaced row or element cannot hide.
  statistics: K in {-2..2}, var in {0, 1/4, 1/2, 1, 2, 4} (0 -> weight 0, reciprocal_no_nan; the other reciprocals are powers of
    two), mean in {-3..3}.  Every product k p k' and k p mean and every partial sum of them is a multiple of 1/4 of magnitude at
    most 16 n (S) or 24 n (v); multiples of 1/4 below 2^22 are float32 numbers, so with 96 n <= 2^24 every sum is exact in any
    order, on the matrix cores and on the vector ALU.
  K_nm: linear x linear without normalisation on integers in {-3..3}: both dot products (at most 9 d) and their product (at most
    81 d1 d2 = 10 368) are integers far below 2^24.
  statistics of one random row: every sum has one term, so each element is a correctly rounded float32 product in any order of
    summation; k_i (p k_j) and k_j (p k_i) differ in the last bit often enough to tell a computed element from a mirrored one.

BOUNDED.  Random data against the float64 reference evaluated on the float32-rounded inputs (kernel parameters included: the
descriptor carries them as float32), with a bound per element from rounding analysis; u = 2^-24 is the unit round-off, u2 = 2 u =
2^-23 one ulp.  None of the constants is measured.
  statistics: S_lij = sum_r k_ri p_rl k_rj is an n-term float32 inner product.  In any summation order (chunks of 32 rows on the
    matrix cores, row slices summed by the reduction) its error is at most gamma_n sum_r |k_ri| p_rl |k_rj|, gamma_n ~ n u
    (Higham, Accuracy and Stability of Numerical Algorithms, 3.1).  The weight p = 1 / var and the scaling p k add one rounding
    each, and the second-order terms stay below two more u for n < 2^20:
        |S - S64|_lij <= (n + 4) u sum_r |k_ri| p_rl |k_rj|
    and the same for v with |p_rl mean_rl| in the sum (p, then p mean, then the n-term sum).
  K_nm.  One rounding is u = u2 / 2 relative; a D-term dot product is within D u = D u2 / 2 of its sum of magnitudes; cosf, sinf
  and rsqrtf are taken at 2 ulp, the hardware exp2 behind the fast exponential at 1 ulp.
    periodic x linear, K = amp^2 exp(s1 (c - 1)) <o_x, o_y>, s1 = 1 / l^2, c = cos a cos b + sin a sin b.
      Let E = amp^2 exp(s1 (c - 1)) and A = E sum_k |o_x,k| |o_y,k| (o normalised when asked).  In ulp of A:
        <o_x, o_y>: the M-term dot product M / 2; per normalised operand the M-term norm M / 4 (halved by the square root),
           rsqrtf 2 and the scaling product 1 / 2                                                        -> M + 5
        c: four function values at 2 ulp, two products, one sum, on magnitudes |cos cos| + |sin sin| <= 1: an absolute error
           of up to 5 ulp, multiplied by s1 in the exponent                                              -> 5 s1
        the exponent arg = s1 (c - 1): s1 (a product and a quotient on the host), the difference, the product and the one
           rounding of arg log2 e inside the fast exponential, 4.5 roundings relative to |arg|            -> 2.25 |arg|
        exp2 1, amp^2 1 / 2, the two closing products 1                                                  -> 2.5
      Sum: M + 7.5 + 2.25 |arg| + 5 s1.  The bound below spends 12 on the constant and 1 on |arg| and 4 on s1; with |arg| <= 2 s1
      the difference 4.5 - 3.5 s1 is positive for s1 <= 1.28, i.e. for every length scale l >= 0.89 (the cases use l = 1.3):
      |err| <= (M + 12 + s1 |c - 1| + 4 s1) u2 A
    SE x SE, K = c0 exp(arg), arg = <a, b> / l1^2 + <c, d> / l2^2 - r_a - r_b.  The four terms of arg cancel, so its absolute
      error is relative to mag = sum |a| |b| / l1^2 + sum |c| |d| / l2^2 + r_a + r_b.  In ulp of mag: the dot products and the
      squared norms inside r, (d1 + d2) / 2; s1 and s2 (two roundings each on the host) 1; the divisions and the sum inside r 1.5;
      the two fused multiply-adds and the sum r_a + r_b 1.5: within d1 + d2 + 8.  The fast exponential adds |arg| / 2 (the rounding
      of arg log2 e) and 1; c0 = sigma1^2 sigma2^2 three roundings; the closing product one: within |arg| + 8 ulp of K:
      |err| <= ((d1 + d2 + 8) mag + |arg| + 8) u2 K64
    linear x linear, K = <a^, b^> <c^, d^> (normalised when asked).  In ulp of A = (sum |a^| |b^|)(sum |c^| |d^|): the two dot
      products (d1 + d2) / 2; the four norms d / 4 each, (d1 + d2) / 2; rsqrtf 2 and the scaling product 1 / 2 per operand, 10;
      the closing product 1 / 2:
      |err| <= (d1 + d2 + 12) u2 A
A plain numpy float32 evaluation of the same formulas stays below a quarter of these bounds at these draws (the CPU guard asserts
half)."""
import functools

import numpy as np

U = 2.0 ** -24
U2 = 2.0 ** -23
PERIODIC_LINEAR, LINEAR_LINEAR, SE_SE = 0, 1, 2
# the instantiations of k_knm_f32 (KNM_CASE in svgp_stream_knm_f32): (kind, d1, d2)
KNM_INSTANCES = ((0, 2, 4), (0, 2, 8), (0, 2, 16), (0, 2, 32), (1, 8, 16), (2, 8, 16), (1, 4, 6), (2, 4, 6))
KNM_ROW_BLOCK = {(1, 4, 6): 32, (1, 8, 16): 128}     # rows per workgroup: 32, 128 when d1 + d2 > 12
KNM_PANEL = 1024                                      # columns per workgroup


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


# ---- statistics -------------------------------------------------------------------------------------------------------------------
# (n, m, L, nsplit, nsplit_v, there for); nsplit / nsplit_v: the row slices of k_stats_mfma_f32 / k_stats_v_f32 that stats_plan gives
STATS_EXACT = [
    (1, 1, 1, 1, 1, "one row, one column: scalar loads, no 4-row loop"),
    (31, 3, 1, 1, 1, "one row short of a 32-row chunk; m % 4 != 0"),
    (32, 4, 2, 1, 1, "exactly one chunk; m % 4 == 0: vector loads"),
    (33, 5, 2, 1, 1, "one row into the second chunk"),
    (65, 31, 1, 1, 1, "one column short of a 32 x 32 block of the diagonal tile"),
    (65, 32, 1, 1, 1, "exactly one block"),
    (65, 33, 1, 1, 1, "one column into the second block: blocks (0, 0), (0, 1), (1, 1) and the mirrored (1, 0)"),
    (100, 255, 2, 1, 1, "one column short of a full tile, scalar path"),
    (100, 256, 2, 1, 1, "a full tile: the branch-free fetch for 3 chunks, the guarded one for the last 4 rows, in one workgroup"),
    (100, 257, 2, 1, 1, "scalar path with a second tile one column wide"),
    (96, 260, 1, 1, 1, "vector path with a second tile four columns wide, every chunk full"),
    (70, 512, 1, 1, 1, "2 full tiles per side"),
    (40, 516, 1, 1, 1, "3 tiles per side, the last one partial"),
    (64, 1028, 1, 1, 1, "5 tiles per side: 10 off-diagonal pairs through the pair decode"),
    (32, 2048, 1, 1, 1, "8 tiles per side, 28 off-diagonal pairs: the config-5 tiling"),
    (300, 36, 16, 1, 1, "one channel pass of k_stats_v_f32 (SV_LC = 16)"),
    (300, 36, 17, 1, 1, "two channel passes, the second with one channel"),
    (300, 36, 33, 1, 1, "three channel passes"),
    (4097, 64, 3, 2, 16, "two row slices (2080 + 2017 rows); v: 16 slices of 257 rows: the 4-row loop, then one scalar row"),
    (131073, 64, 1, 64, 512, "64 row slices, the last one 33 rows; v: 512 slices, the last ones empty"),
]
# (n, m, L, nsplit, nsplit_v): the four shapes of tests/test_gpu_stream_f32.py::test_stats and two more
STATS_RANDOM = [
    (1000, 64, 3, 1, 3),
    (5000, 300, 5, 2, 19),
    (4100, 516, 2, 2, 16),
    (40, 30, 17, 1, 1),
    (100, 256, 2, 1, 1),
    (4097, 64, 3, 2, 16),
]


def round_up(x, q):
    return (x + q - 1) // q * q


def stats_workspace_layout(n, m, L, nsplit, nsplit_v):
    """The workspace of svgp_stream_stats_f32 as stats_plan lays it out, in float32 elements: weights 1 / var and mean / var
    transposed (L, n) each, the partial tiles (nsplit, L, m, m), the partial vectors (nsplit_v, L, m).  A row slice of the tile
    kernel is a whole number of 32-row chunks, so that only the last slice has a ragged chunk."""
    off_part = round_up(2 * L * n, 4)
    off_partv = off_part + nsplit * L * m * m
    return dict(part=off_part, partv=off_partv, total=off_partv + nsplit_v * L * m,
                rows_per_split=round_up(-(-n // nsplit), 32))


def stats64(K, means, vars_):
    """S_l = K^T diag(p_l) K and v_l = K^T (p_l mean_l) in float64, p = reciprocal_no_nan(var): the rule of _stats64 in
    tests/test_gpu_stream_f32.py, one matrix product per channel."""
    K, means, vars_ = (np.asarray(a, np.float64) for a in (K, means, vars_))
    p = np.where(vars_ == 0, 0.0, 1.0 / np.where(vars_ == 0, 1.0, vars_))
    S = np.stack([(K * p[:, l:l + 1]).T @ K for l in range(p.shape[1])])
    v = (K.T @ (p * means)).T
    return S, v


@functools.lru_cache(maxsize=None)
def stats_exact_inputs(n, m, L):
    """K (n, m), means (n, L), vars (n, L) float32 on which the statistics are exact, and their reference (S, v) in float64."""
    rng = np.random.default_rng([n, m, L])
    K = rng.integers(-2, 3, (n, m)).astype(np.float32)
    means = rng.integers(-3, 4, (n, L)).astype(np.float32)
    vars_ = rng.choice(np.array([0, 0.25, 0.5, 1, 2, 4], np.float32), (n, L))
    S, v = stats64(K, means, vars_)
    return _frozen(K, means, vars_, S, v)


@functools.lru_cache(maxsize=None)
def stats_random_inputs(n, m, L):
    """The draws of tests/test_gpu_stream_f32.py::test_stats; returns K, means, vars (float32), the float64 reference (S, v) of
    the float32-rounded inputs and the per-element bounds (bS, bv) of the module docstring."""
    rng = np.random.default_rng(n)
    K = rng.normal(0, 1, (n, m)).astype(np.float32)
    means = rng.normal(0, 1, (n, L)).astype(np.float32)
    vars_ = rng.uniform(1e-3, 10, (n, L)).astype(np.float32)
    vars_[::7, 0] = 0.0                                       # reciprocal_no_nan rows
    S, v = stats64(K, means, vars_)
    bS, bv = stats64(np.abs(K), np.abs(means), vars_)
    return _frozen(K, means, vars_, S, v, (n + 4) * U * bS, (n + 4) * U * bv)


# (m, L): one row of random data.  Every sum has one term, so each element is a correctly rounded float32 product whatever the
# order of summation, and which of the two products an element is tells whether it was computed or mirrored.
STATS_ONE_ROW = [(65, 2), (300, 1)]


@functools.lru_cache(maxsize=None)
def stats_one_row_inputs(m, L):
    """K (1, m), means (1, L), vars (1, L) float32 and the statistics bit for bit (float32): the tile kernel multiplies the
    column i of K with the weighted column j, S_lij = fl(k_i fl(p_l k_j)), for the tile pairs ti <= tj and, inside a diagonal
    tile, the 32 x 32 blocks bi <= bj; the rest is the mirror S_lji.  v_li = fl(k_i fl(p_l mean_l)).  p_l = fl(1 / var_l)."""
    rng = np.random.default_rng([m, L])
    K = rng.normal(0, 1, (1, m)).astype(np.float32)
    means = rng.normal(0, 1, (1, L)).astype(np.float32)
    vars_ = rng.uniform(0.5, 3, (1, L)).astype(np.float32)
    p = np.float32(1) / vars_[0]
    E = K[0][None, :, None] * (p[:, None, None] * K[0][None, None, :])
    blk = np.arange(m) >> 5
    S = np.where(blk[:, None] <= blk[None, :], E, E.transpose(0, 2, 1))
    v = K[0][None, :] * (p * means[0])[:, None]
    assert S.dtype == np.float32 and v.dtype == np.float32
    return _frozen(K, means, vars_, S, v)


def stats_f32_numpy(K, means, vars_):
    """The statistics in numpy float32 (the CPU guard's stand-in for the kernels)."""
    one = np.float32(1)
    p = np.where(vars_ == 0, np.float32(0), one / np.where(vars_ == 0, one, vars_)).astype(np.float32)
    S = np.stack([(K * p[:, l:l + 1]).T @ K for l in range(p.shape[1])])
    v = (K.T @ (p * means)).T
    assert S.dtype == np.float32 and v.dtype == np.float32
    return S, v


# ---- K_nm -------------------------------------------------------------------------------------------------------------------------
N_OBJ, N_ACT = 40, 72                                 # rows of the gather tables (objects; the 72 SPRITES actions)
PERIODIC_PARAMS = (1.3, 0.9)                          # (l_GP, amplitude) of tests/test_gpu_stream_f32.py
SE_PARAMS = {(8, 16): (5.0, 1.4, 7.0, 1.2), (4, 6): (2.0, 1.0, 2.5, 1.0)}      # (l1, sigma1, l2, sigma2); (4, 6): unit-variance features
# (kind, d1, d2, n, m): linear x linear on integers, around the rows per workgroup and the 1024-column panel
KNM_EXACT = [(1, d1, d2, n, m) for (d1, d2), ns in (((4, 6), (1, 31, 32, 33)), ((8, 16), (127, 128, 129)))
             for n in ns for m in (1, 3, 4, 1023, 1024, 1025, 1028)]
# the same with a row stride of need + 3: the rows are the leading columns of a wider matrix padded with NaN
KNM_EXACT_WIDE = [(1, 4, 6, 33, 1025), (1, 8, 16, 129, 1028)]
# (kind, d1, d2, normalize, table, n, m)
KNM_BOUNDED = [(0, 2, M, nz, tab, 300, 257) for M in (4, 8, 16, 32) for nz in (False, True) for tab in (True, False)] + \
              [(0, 2, 32, True, True, 300, 1100)] + \
              [(1, d1, d2, nz, True, 300, 257) for d1, d2 in ((8, 16), (4, 6)) for nz in (False, True)] + \
              [(2, d1, d2, False, True, 300, 257) for d1, d2 in ((8, 16), (4, 6))]


def knm_params(kind, d1, d2):
    """The kernel parameters as the descriptor holds them: float32 values, returned as Python floats."""
    p = PERIODIC_PARAMS if kind == 0 else SE_PARAMS[(d1, d2)] if kind == 2 else ()
    return tuple(float(np.float32(v)) for v in p)


def mnist_kernel64(x, y, l_gp, amp, table, normalize, x_inducing):
    """float64 restatement of mnistSVGP.kernel_matrix (SVGPVAE_model.py:427-476), y always inducing; as _mnist_kernel64 of
    tests/test_gpu_stream_f32.py."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ox = x[:, 2:] if (x_inducing or table is None) else np.asarray(table, np.float64)[x[:, 0].astype(int)]
    oy = y[:, 2:]
    d = x[:, 1][:, None] - y[:, 1][None, :]
    per = amp ** 2 * np.exp(-2.0 * np.sin(d / 2.0) ** 2 / l_gp ** 2)
    lin = ox @ oy.T
    if normalize:
        lin = lin / (np.linalg.norm(ox, axis=1)[:, None] * np.linalg.norm(oy, axis=1)[None, :])
    return per * lin


def sprites_kernel64(x, y, table, normalize, se, x_inducing, La):
    """float64 restatement of spritesSVGP.kernel_matrix (:550-600), y always inducing; as _sprites_kernel64 of
    tests/test_gpu_stream_f32.py."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if x_inducing:
        ax, cx = x[:, :La], x[:, La:]
    else:
        ax, cx = np.asarray(table, np.float64)[x[:, 0].astype(int)], x[:, 1:]
    ay, cy = y[:, :La], y[:, La:]
    if se is not None:
        l1, s1, l2, s2 = se
        d1 = ((ax[:, None, :] - ay[None, :, :]) ** 2).sum(-1)
        d2 = ((cx[:, None, :] - cy[None, :, :]) ** 2).sum(-1)
        return s1 ** 2 * np.exp(-d1 / (2 * l1 ** 2)) * s2 ** 2 * np.exp(-d2 / (2 * l2 ** 2))
    k1, k2 = ax @ ay.T, cx @ cy.T
    if normalize:
        k1 = k1 / (np.linalg.norm(ax, axis=1)[:, None] * np.linalg.norm(ay, axis=1)[None, :])
        k2 = k2 / (np.linalg.norm(cx, axis=1)[:, None] * np.linalg.norm(cy, axis=1)[None, :])
    return k1 * k2


@functools.lru_cache(maxsize=None)
def knm_exact_inputs(kind, d1, d2, n, m):
    """Integer batch rows x (n, 1 + d2), inducing rows z (m, d1 + d2) and action table (N_ACT, d1) in float32, the float64
    K_nm (n, m) and K_mm (m, m)."""
    assert kind == LINEAR_LINEAR
    rng = np.random.default_rng([d1, d2, n, m])
    tab = rng.integers(-3, 4, (N_ACT, d1)).astype(np.float32)
    x = np.concatenate([rng.integers(0, N_ACT, (n, 1)), rng.integers(-3, 4, (n, d2))], 1).astype(np.float32)
    z = rng.integers(-3, 4, (m, d1 + d2)).astype(np.float32)
    return _frozen(x, z, tab, sprites_kernel64(x, z, tab, False, None, False, d1), sprites_kernel64(z, z, None, False, None, True, d1))


def _knm_draw(kind, d1, d2, table, n, m):
    rng = np.random.default_rng([kind, d1, d2, int(table), n, m])
    if kind == PERIODIC_LINEAR:
        tab = rng.normal(0, 1.5, (N_OBJ, d2)) if table else None
        x = np.concatenate([rng.integers(0, N_OBJ, (n, 1)).astype(float), rng.uniform(0, 2 * np.pi, (n, 1)),
                            rng.normal(0, 1.5, (n, d2))], 1)
        z = np.concatenate([np.zeros((m, 1)), rng.uniform(0, 2 * np.pi, (m, 1)), rng.normal(0, 1.5, (m, d2))], 1)
    else:
        sd = 1.0 if (d1, d2) == (4, 6) else 1.5
        tab = rng.normal(0, sd, (N_ACT, d1))
        x = np.concatenate([rng.integers(0, N_ACT, (n, 1)).astype(float), rng.normal(0, sd, (n, d2))], 1)
        z = rng.normal(0, sd, (m, d1 + d2))
    return x.astype(np.float32), z.astype(np.float32), None if tab is None else tab.astype(np.float32)


def knm_ref_bound(kind, d1, d2, normalize, x, z, tab, x_inducing):
    """float64 K (rows x against inducing rows z) of the float32-rounded inputs and parameters, and the per-element bound of the
    module docstring."""
    p = knm_params(kind, d1, d2)
    x64, z64 = x.astype(np.float64), z.astype(np.float64)
    t64 = None if tab is None else tab.astype(np.float64)
    unit = lambda a: a / np.linalg.norm(a, axis=1)[:, None] if normalize else a
    if kind == PERIODIC_LINEAR:
        l_gp, amp = p
        ref = mnist_kernel64(x64, z64, l_gp, amp, t64, normalize, x_inducing)
        ox = x64[:, 2:] if (x_inducing or t64 is None) else t64[x64[:, 0].astype(int)]
        s1 = 1.0 / l_gp ** 2
        c = np.cos(x64[:, 1][:, None] - z64[:, 1][None, :])
        A = amp ** 2 * np.exp(s1 * (c - 1.0)) * (np.abs(unit(ox)) @ np.abs(unit(z64[:, 2:])).T)
        return ref, (d2 + 12 + s1 * np.abs(c - 1.0) + 4 * s1) * U2 * A
    if x_inducing:
        ax, cx = x64[:, :d1], x64[:, d1:]
    else:
        ax, cx = t64[x64[:, 0].astype(int)], x64[:, 1:]
    ay, cy = z64[:, :d1], z64[:, d1:]
    if kind == LINEAR_LINEAR:
        ref = sprites_kernel64(x64, z64, t64, normalize, None, x_inducing, d1)
        A = (np.abs(unit(ax)) @ np.abs(unit(ay)).T) * (np.abs(unit(cx)) @ np.abs(unit(cy)).T)
        return ref, (d1 + d2 + 12) * U2 * A
    l1, _, l2, _ = p
    ref = sprites_kernel64(x64, z64, t64, False, p, x_inducing, d1)
    r = lambda a, c: (a ** 2).sum(1) / (2 * l1 ** 2) + (c ** 2).sum(1) / (2 * l2 ** 2)
    ra, rb = r(ax, cx)[:, None], r(ay, cy)[None, :]
    mag = np.abs(ax) @ np.abs(ay).T / l1 ** 2 + np.abs(cx) @ np.abs(cy).T / l2 ** 2 + ra + rb
    arg = ax @ ay.T / l1 ** 2 + cx @ cy.T / l2 ** 2 - ra - rb
    return ref, ((d1 + d2 + 8) * mag + np.abs(arg) + 8) * U2 * ref


@functools.lru_cache(maxsize=None)
def knm_bounded_inputs(kind, d1, d2, normalize, table, n, m):
    """x, z, table (float32; table None for periodic rows that carry their own object vector), then (K_nm, its bound) and
    (K_mm, its bound) in float64."""
    x, z, tab = _knm_draw(kind, d1, d2, table, n, m)
    knm, b_nm = knm_ref_bound(kind, d1, d2, normalize, x, z, tab, False)
    kmm, b_mm = knm_ref_bound(kind, d1, d2, normalize, z, z, None, True)
    return _frozen(x, z, tab, knm, b_nm, kmm, b_mm)


def knm_f32_numpy(kind, d1, d2, normalize, x, z, tab, x_inducing):
    """k_features_f32 and k_knm_f32 restated in numpy float32, operation by operation (the CPU guard's stand-in for the kernels)."""
    f32, one = np.float32, np.float32(1)
    p = [f32(v) for v in knm_params(kind, d1, d2)]
    sq = lambda a: (a * a).sum(1, dtype=f32)
    unit = lambda a: a * (one / np.sqrt(sq(a)))[:, None] if normalize else a

    def feats(a, inducing):
        if kind == PERIODIC_LINEAR:
            o = a[:, 2:] if (inducing or tab is None) else tab[a[:, 0].astype(int)]
            return np.stack([np.cos(a[:, 1]), np.sin(a[:, 1])], 1).astype(f32), unit(o)
        act, chr_ = (a[:, :d1], a[:, d1:]) if inducing else (tab[a[:, 0].astype(int)], a[:, 1:])
        return (unit(act), unit(chr_)) if kind == LINEAR_LINEAR else (act, chr_)

    (a1, a2), (b1, b2) = feats(x, x_inducing), feats(z, True)
    dot1, dot2 = a1 @ b1.T, a2 @ b2.T
    assert dot1.dtype == f32 and dot2.dtype == f32
    if kind == PERIODIC_LINEAR:
        out = (p[1] * p[1]) * np.exp((one / (p[0] * p[0])) * (dot1 - one)) * dot2
    elif kind == LINEAR_LINEAR:
        out = dot1 * dot2
    else:
        r = lambda a, c: sq(a) / (f32(2) * p[0] * p[0]) + sq(c) / (f32(2) * p[2] * p[2])
        s1, s2 = one / (p[0] * p[0]), one / (p[2] * p[2])
        out = (p[1] * p[1] * p[3] * p[3]) * np.exp(s1 * dot1 + (s2 * dot2 + (-r(a1, a2)[:, None] - r(b1, b2)[None, :])))
    assert out.dtype == f32
    return out
