"""`GPVAE_Pearce_model.py` of the reference (`build_pearce_elbo_graphs`, GPVAE_Pearce_model.py:89; imported by
BALL_experiment.py:15).  The exact per-video GP (`build_1d_gp`, :8-86) runs as `k_pearce_fwd / k_pearce_bwd` of the HIP
library up to 64 frames and on the global-memory kernels of pearce_long.hip up to 2048; the host side lives with the other
moving-ball engines in ball.py."""
from .ball import PearceLongStepEngine, PearceStepEngine, build_pearce_elbo_graphs  # noqa: F401
