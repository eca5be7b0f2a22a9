// The two size thresholds between the forms of the m x m stages, and the pieces of the large-m factor stages (gp_large.hip).
// Host-only constants: shared by the kernels' translation units (common.hpp) and the step planner (step_plan.hpp).
#pragma once

#define SVGP_M_MAX 64          // up to here the m x m stages stay LDS-resident (gp_kernels.hip)
#define SVGP_CHOL_INVERSE_MIN_M 512   // spd inverse: fused 32-block Gauss-Jordan sweep below, potrf + potri from here on

// The pieces of the two large-m factor stages (gp_large.hip): what a caller may issue on its own (on another stream, before or after
// a join).  A call runs the pieces of its set in the order listed here; the data dependencies between pieces of different calls are
// the caller's business (gp_large.hip has them at the two functions).
enum : unsigned {
    SVGP_FWD_K = 1,         // channel-independent block: (K + jI)^-1, log det, Kn Ki, q, W, P^T -- needs the kernel matrices only
    SVGP_FWD_SIG = 2,       // channel block up to mu: Sigma^-1, t, G, A_hat (+ A_hat + jI), mu
    SVGP_FWD_KL = 4,        // u = Ki mu and the trace partials: needs K and SIG
    SVGP_FWD_TAIL = 8,      // (A_hat + jI)^-1, its log det, KL_l: only the reverse factor stage and the final ELBO need it
    SVGP_FWD_HEAD = SVGP_FWD_K | SVGP_FWD_SIG | SVGP_FWD_KL,
    SVGP_FWD_ALL = SVGP_FWD_HEAD | SVGP_FWD_TAIL,
};
enum : unsigned {
    SVGP_BWD_SW = 1,        // T = S P, SW = P^T T (only when SW is not formed over the rows by the reverse statistics)
    SVGP_BWD_EARLY_B = 2,   // H, HG, the three channel sums: needs (A_hat + jI)^-1
    SVGP_BWD_LATE_A = 4,    // the vector chain; + the X block when it reads nothing EARLY_B writes (SW from the rows, or no SW)
    SVGP_BWD_CHANNELS = 8,  // the X block otherwise; Ssym; the channel sum Sgs
    SVGP_BWD_KBAR = 16,     // the single-matrix chain of the gradient of Ki (five launches that read nothing of CHANNELS)
    SVGP_BWD_FINAL = 32,    // the closing assembly of Kbar
    SVGP_BWD_EARLY = SVGP_BWD_SW | SVGP_BWD_EARLY_B,
    SVGP_BWD_LATE_B = SVGP_BWD_CHANNELS | SVGP_BWD_KBAR | SVGP_BWD_FINAL,
    SVGP_BWD_LATE = SVGP_BWD_LATE_A | SVGP_BWD_LATE_B,
    SVGP_BWD_ALL = SVGP_BWD_EARLY | SVGP_BWD_LATE,
};
