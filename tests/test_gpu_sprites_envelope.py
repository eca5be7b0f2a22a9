"""The SPRITES step (SpritesStepEngine) over the shape range it accepts, against the float64 oracle (oracle/sprites_oracle.py), at
the shapes where its kernels change form, inside the step, where each stage's output feeds the next.  Case table, problems,
tolerances: tests/sprites_cases.py; that the oracle itself is well conditioned at every case: tests/test_sprites_envelope_oracle_cpu.py.

What changes with the shape (svgp-vae_amd/csrc):
  * m: m <= 32 the five-LDS-matrix form of the factor kernels, m == 32 its own instance, 33 <= m <= 64 the four-matrix form
    (gp_kernels.hip), m > 64 the global-memory path (gp_large.hip) with its side-stream branches (sprites.py) and, with Titsias,
    gp_titsias.hip; m = 130 is no multiple of the 64-wide tiles.  m = 1, 2 are the widest rows-per-workgroup forms.
  * L: channels of the GP block and the dense layers' width (1 <= L <= 64); L >= 22 at m > 64 is the range the MNIST step needed a
    fix for.
  * (L_action, L_character): the tiled kernel-matrix VJP (gp_sprites.hip: sprites_bwd_bucket) has the template buckets (8,16) and
    (16,32); outside both (L_action > 16) the per-target kernels k_sprites_kernel_bwd_cols / _rows with (La + Lc) | 1 doubles of
    dynamic LDS per thread; SP_MAXD = 32 is the limit.  L_character != 16 takes the representation network off the direct
    16-channel convolution kernels onto the tap-table ones (conv_taps.hip: Lc -> Lc, k = 2, stride 2; Lc <= 16: check_desc), and
    svgp_sprites_aux_* / svgp_avgpool_* run at that width.
  * seg_len: the segment mean of svgp_sprites_aux_fwd / _bwd (1: every frame its own character); n_act = 1: every row of the
    batch scatters into GPLVM row 0 (k_sprites_kernel_bwd_scatter).
  * b: the row statistics are summed in partials sized from the capacity b_max, not from b (common.hpp svgp_stat_parts: one below
    128 rows of capacity, four from 128); min(b, 256) partial sums of the reconstruction error (SVGP_MAX_PART); the kernel-matrix
    VJP scratch need is not monotone in b (sprites_bwd_splits).  The driver builds its engine with b_max above the training batch,
    so the engine is also stepped below capacity here, and with a small batch after a full one.
"""
import pytest
import torch

from tests import sprites_cases as SC
from tests.sprites_cases import DT

pytestmark = pytest.mark.gpu


def _step_and_compare(eng, case, rows=None, label=None):
    cs = SC.CASES[case]
    _, _, images, ids, eps, want, wgrads = SC.reference(case, rows)
    got = SC.step(eng, images, ids, eps)
    assert eng.cfg.b == images.shape[0]
    return SC.compare(eng, got, want, wgrads, cs["kernel"] == "se", label or case)


@pytest.mark.parametrize("case", SC.ENVELOPE_CASES)
def test_sprites_step_matches_oracle_across_the_shape_range(case):
    cs = SC.CASES[case]
    params, gp = SC.reference(case)[:2]
    eng = SC.engine(case, params, gp)
    assert eng.wl.stat_parts == (4 if cs["b_max"] >= 128 else 1)
    bad, _, _ = _step_and_compare(eng, case)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", list(SC.CAPACITY_BATCHES))
def test_batches_below_capacity_on_one_engine(case):
    """One engine of the case's capacity (the buffers sized from it: statistics partials, kernel-matrix VJP scratch, the layers'
    partial-sum regions) stepped with fewer rows, then the full batch, then a small batch again -- rows or partials left over from
    the full batch must not reach it.  Each step against the oracle for exactly those rows."""
    cs = SC.CASES[case]
    params, gp = SC.reference(case)[:2]
    eng = SC.engine(case, params, gp)
    assert eng.b_max == cs["b"] == max(SC.CAPACITY_BATCHES[case])
    bad = []
    for i, rows in enumerate(SC.CAPACITY_BATCHES[case]):
        bad += [f"step {i}, {rows} rows of {cs['b']}: {t}"
                for t in _step_and_compare(eng, case, rows, label=f"{case} step {i} rows {rows}")[0]]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", SC.SIDE_STREAM_CASES)
def test_side_streams_equal_one_stream_at_ragged_shapes(case):
    """tests/test_gpu_sprites.py::test_sprites_side_streams_equal_one_stream at m = 65 and m = 130 (no multiple of the tile): three
    Adam steps with the side branches and three with every launch on one stream give the same bits."""
    params, gp, images, ids, eps, _, _ = SC.reference(case)
    out = []
    for one_stream in (False, True):
        eng = SC.engine(case, params, gp, lr=3e-3)
        assert eng.side is not None and eng.scratch2 is not None
        if one_stream:
            eng.side = eng.side2 = None
        dev = eng.dev
        di, da, de = images.to(dev), ids.to(dev, DT), eps.to(dev)
        for _ in range(3):
            eng.step(di, da, de, adam=True)
        assert eng.scalars()["adam_t"] == 3.0
        out.append((eng.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.state.clone()))
    for name, x, y in zip(("theta", "adam_m", "adam_v", "state"), *out):
        assert bool(torch.isfinite(x).all()), name
        assert torch.equal(x, y), name


@pytest.mark.parametrize("case", SC.F32_CASES)
def test_float32_networks_at_envelope_shapes(case):
    """float32 networks with the float64 GP block (net_dtype = float32, gemm_f32 = 0) on the generic representation-network
    kernels (L_character = 11) and at L = 33, at the bars of tests/test_gpu_f32.py::test_sprites_step_float32."""
    params, gp, images, ids, eps, want, wgrads = SC.reference(case)
    eng = SC.engine(case, params, gp, net_dtype=torch.float32, gemm_f32=0)
    got = SC.step(eng, images, ids, eps)
    gr = eng.grads
    bars = [(SC.TUPLE_NAMES[i], got[i], want[i], tol) for i, tol in
            ((7, SC.F32_ENC_TOL), (8, SC.F32_ENC_TOL), (0, SC.F32_ELBO_TOL), (1, SC.F32_ELBO_TOL), (2, SC.F32_ELBO_TOL),
             (9, SC.F32_ELBO_TOL), (5, SC.F32_POST_TOL), (6, SC.F32_POST_TOL))]
    bars += [(f"grad {k}", gr[k], wgrads[k], SC.F32_WGRAD_TOL) for k in SC.F32_WGRADS]
    bad = []
    for name, have, w, tol in bars:
        e = SC.rel(have, w)
        print(f"{case} f32 {name}: {e:.2e} (bar {tol:.0e})")
        if not e < tol:
            bad.append(f"{name}: {e:.3e} (bar {tol:.0e})")
    assert all(bool(torch.isfinite(torch.as_tensor(t)).all()) for t in got)
    assert bool(torch.isfinite(eng.grad).all())
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("La,Lc", [(8, 17), (33, 16)])
def test_unsupported_feature_widths_are_refused(La, Lc):
    """L_character = 17 is past the 16 channels of the convolution kernels (conv_taps.hip check_desc), L_action = 33 past SP_MAXD
    (gp_sprites.hip): SvgpError no later than the first step, and a valid engine in the same process still matches the oracle."""
    from svgp_vae_amd import _lib
    from svgp_vae_amd import sprites as S
    b, seg, L, m, n_act = 8, 4, 6, 12, 9
    params, gp, images, ids, eps, _, _ = SC.problem(b, seg, L, La, Lc, m, n_act, seed=300 + La + Lc)
    with pytest.raises(_lib.SvgpError):
        svgp = S.spritesSVGP(False, False, gp["inducing_index_points"].numpy(), 'main', SC.JITTER, SC.N_TRAIN, La,
                             gp["GPLVM_action"].numpy(), Lc, L, K_obj_normalize=True)
        eng = S.SpritesStepEngine(S.spritesVAE(L), S.sprites_representation_network(Lc), svgp, b_max=b, seg_len=seg, geco=True,
                                  params=params)
        dev = eng.dev
        eng.step(images.to(dev), ids.to(dev, DT), eps.to(dev), adam=False)
    torch.cuda.synchronize()
    params, gp = SC.reference("nact1")[:2]
    bad, _, _ = _step_and_compare(SC.engine("nact1", params, gp), "nact1", label=f"nact1 after La {La} Lc {Lc}")
    assert not bad, "\n".join(bad)
