// The launch schedule of the MNIST step as data.  step_plan() is the ONE place that decides, for every form of the step
// (svgp_mnist_step_phase, svgp_mnist_train_step, svgp_mnist_train_step_dp), which stage entry runs on which lane, where a side
// branch is forked and joined and where a collective is issued.  Pure host arithmetic: no HIP call, no allocation, no text.
// api.hip executes a plan (svgp_step_run), svgp_mnist_step_route prints one; tests/test_step_route_cpu.py pins the routes.
// Why an order is what it is (DESIGN.md 6 has the measurements) is written at the line that fixes it, below.
#pragma once
#include "../../include/svgpvae_hip.h"
#include "gp_pieces.hpp"
#include "sched.hpp"

// (measured with a 1-rank communicator at m = 256, L = 16: the pack / unpack launches cost ~100 us per step, the 44 % of 8.4 MB
// they take off each of the four points is worth ~15 us apiece on xGMI; at m = 800, L = 64 a point is 328 MB)
inline bool svgp_dp_pack_rule(int m) { return m >= 512; }

// Every stage entry the step calls: enumerator, entry point.  The svgp_big_* two are the channel-window forms (gp_large.hip) of
// the sharded step; the others are the entry points of include/svgpvae_hip.h (svgp_gp_factor_fwd_pieces: common.hpp).
#define SVGP_STEP_STAGES(X)                                              \
    X(ENC_KM_FWD, svgp_mnist_encoder_kernel_matrix_fwd)                  \
    X(STATS_FWD, svgp_gp_stats_fwd)                                      \
    X(TIT_STATS, svgp_gp_titsias_stats)                                  \
    X(FACTOR_FWD_PIECES, svgp_gp_factor_fwd_pieces)                      \
    X(FACTOR_FWD_DEFER_AJI, svgp_gp_factor_fwd_defer_aji)                \
    X(FACTOR_FWD_AJI_TAIL, svgp_gp_factor_fwd_aji_tail)                  \
    X(BIG_FACTOR_FWD, svgp_big_factor_fwd)                               \
    X(POST_FWD, svgp_gp_posterior_fwd)                                   \
    X(POST_FWD_AJI, svgp_gp_posterior_fwd_with_aji)                      \
    X(TIT_FWD, svgp_gp_titsias_fwd)                                      \
    X(DEC_FUSED_AJI, svgp_mnist_decoder_fwd_bwd_data_pre_aji)            \
    X(DEC_FUSED, svgp_mnist_decoder_fwd_bwd_data_pre)                    \
    X(DEC_FWD_PRE, svgp_mnist_decoder_fwd_pre)                           \
    X(DEC_BWD_DATA_PRE_AJI, svgp_mnist_decoder_bwd_data_pre_aji)         \
    X(DEC_BWD_DATA_PRE, svgp_mnist_decoder_bwd_data_pre)                 \
    X(DEC_FWD, svgp_mnist_decoder_fwd)                                   \
    X(DEC_BWD, svgp_mnist_decoder_bwd)                                   \
    X(STATS_BWD, svgp_gp_stats_bwd)                                      \
    X(FACTOR_BWD_EARLY, svgp_gp_factor_bwd_early)                        \
    X(FACTOR_BWD_LATE_A, svgp_gp_factor_bwd_late_a)                      \
    X(FACTOR_BWD_LATE_B, svgp_gp_factor_bwd_late_b)                      \
    X(FACTOR_BWD_LATE_B_KBAR, svgp_gp_factor_bwd_late_b_kbar)            \
    X(FACTOR_BWD_LATE_B_CHANNELS, svgp_gp_factor_bwd_late_b_channels)    \
    X(FACTOR_BWD_LATE_B_FINAL, svgp_gp_factor_bwd_late_b_final)          \
    X(BIG_FACTOR_BWD, svgp_big_factor_bwd)                               \
    X(STATS_FACTOR_BWD_WGRAD, svgp_gp_stats_factor_bwd_wgrad)            \
    X(FACTOR_BWD_NOFINAL_WGRAD, svgp_gp_factor_bwd_nofinal_wgrad)        \
    X(FACTOR_BWD_NOFINAL, svgp_gp_factor_bwd_nofinal)                    \
    X(POST_BWD_ROWS, svgp_gp_posterior_bwd_rows)                         \
    X(POST_BWD_FINAL, svgp_gp_posterior_bwd_with_final)                  \
    X(POST_BWD, svgp_gp_posterior_bwd)                                   \
    X(TIT_BWD, svgp_gp_titsias_bwd)                                      \
    X(KM_BWD_PARTIALS, svgp_kernel_matrix_bwd_partials)                  \
    X(ENC_BWD, svgp_mnist_encoder_bwd)                                   \
    X(ENC_BWD_KM, svgp_mnist_encoder_bwd_km)                             \
    X(ENC_BWD_KM_SUM, svgp_mnist_encoder_bwd_km_sum)                     \
    X(GRAD_REDUCE_ALL, svgp_mnist_grad_reduce_all)                       \
    X(GRAD_REDUCE_PART, svgp_mnist_grad_reduce_part)                     \
    X(ADAM_FINALIZE, svgp_adam_tf1_finalize)                             \
    X(FINALIZE_NOADAM, svgp_elbo_finalize_noadam)

enum StepStage : unsigned char {
#define X(id, fn) STEP_ST_##id,
    SVGP_STEP_STAGES(X)
#undef X
    STEP_ST_COUNT
};

// What an exchange op moves: the three blocks of the all-reduce forms (gradC also as its two halves, cfg.split_grad_exchange) and
// the members of the four points of the channel-sharded form.  S, Si, A2, Ssym are the symmetric (L, m, m) blocks that may travel
// tile-packed (STEP_PART_PACKED); the others are (L, m) vectors, KL is (L).
#define SVGP_STEP_BLOCKS(X) \
    X(statA) X(statB) X(gradC) X(gradC_hi) X(gradC_lo) X(S) X(v) X(Si) X(t) X(u) X(A2) X(ud) X(td) X(Ssym) X(vbar) X(KL)
enum StepBlock : unsigned char {
#define X(id) STEP_BLK_##id,
    SVGP_STEP_BLOCKS(X)
#undef X
    STEP_BLK_COUNT
};

enum StepKind : unsigned char {
    STEP_STAGE,             // stage `stage` on `lane`; arg: a piece set (SVGP_FWD_* / SVGP_BWD_*) or the part of svgp_mnist_grad_reduce_part
    STEP_FORK,              // side branch `lane` continues after everything issued on the caller's stream so far
    STEP_JOIN,              // the caller's stream continues after everything issued on side branch `lane` (no-op when it is not open)
    STEP_ALLREDUCE,         // block `arg`, summed over the ranks, on `lane`: an exchange point of its own
    STEP_POINT_BEGIN,       // exchange point `arg` (1..4) of the channel-sharded form opens: the optional timing event
    STEP_POINT_END,
    STEP_PACK,              // symmetric block `arg`, `part` of its channels, to the wire buffer
    STEP_UNPACK,
    STEP_GROUP_BEGIN,       // the collectives up to STEP_GROUP_END are one RCCL launch
    STEP_GROUP_END,
    STEP_REDUCE_SCATTER,    // block `arg` over the channels (part STEP_PART_PACKED: its wire buffer)
    STEP_ALLGATHER,
};
enum StepLane : unsigned char { STEP_MAIN, STEP_SIDE0, STEP_SIDE1 };
enum StepPart : unsigned char { STEP_PART_ALL, STEP_PART_WINDOW /* the rank's channels */, STEP_PART_OTHERS, STEP_PART_PACKED };
enum StepForm { STEP_FORM_PHASE = 0, STEP_FORM_STEP = 1, STEP_FORM_DP = 2 };

struct StepOp { unsigned char kind, lane, stage, part; unsigned arg; };
#define SVGP_STEP_MAX_OPS 96
struct StepPlan {
    int n = 0;
    bool side = false;      // the call looks up (the first time: creates) the side branches of the caller's stream
    // m <= 32 (SVGP_FWD_SPLIT): four launch slots run another form of their entry -- the forward factor stage its head form (Si, t,
    // mu_hat, u, q), the forward row stage its z form (no d, no L3 partial), the fused decoder launch the riders that finish the
    // factor stage (G, A, M2, Aji, KL), pass 1 of the reverse row stage its d form (d, L3 partial).  The slots and their names in the
    // route text stay; svgp_mnist_step_route_forms prints the forms.
    bool fwd_split = false;
    bool early = false;     // the plan issues the early reverse factor half on branch 1: the late half alone may follow
    bool sharded = false;   // the channel-sharded form: stages run on a copy of cfg with rep_weight 1
    bool pack = false;      // ... whose symmetric blocks travel tile-packed: the workspace must carry the wire buffer
    StepOp op[SVGP_STEP_MAX_OPS];
};

// form STEP_FORM_PHASE: stand-alone phase `phase` (0..5), which joins what it forks before it returns (each phase may be captured
// into its own graph, with a collective in between); early_issued: phase 1 of this library issued the early reverse factor half
// on this workspace.  STEP_FORM_STEP: the four phases back to back with NOTHING exchanged in between, so a stage may move across
// a phase boundary.  STEP_FORM_DP: the step on `nranks` ranks -- phases with an all-reduce behind each of the first three, a
// branch forked in one phase may be joined in a later one; the split-gradient form; or the channel-sharded form.
// SVGP_OK, or SVGP_ERR_INVALID (form / phase / rank out of range; more ops than the plan holds).
inline int step_plan(const svgp_mnist_cfg* c, int form, int phase, int nranks, int rank, bool adam, bool early_issued,
                     const SvgpSched& sc, StepPlan& P) {
    P = StepPlan();
    if (form < STEP_FORM_PHASE || form > STEP_FORM_DP || (form == STEP_FORM_PHASE && (phase < 0 || phase > 5))) return SVGP_ERR_INVALID;
    if (form == STEP_FORM_DP && (nranks < 1 || rank < 0 || rank >= nranks)) return SVGP_ERR_INVALID;
    auto push = [&](StepKind kind, StepLane lane, unsigned char stage, unsigned arg, StepPart part) {
        if (P.n < SVGP_STEP_MAX_OPS) P.op[P.n] = StepOp{kind, lane, stage, part, arg};
        ++P.n;
    };
    auto run = [&](StepStage st, StepLane lane = STEP_MAIN, unsigned arg = 0) { push(STEP_STAGE, lane, st, arg, STEP_PART_ALL); };
    auto fork = [&](StepLane lane) { push(STEP_FORK, lane, 0, 0, STEP_PART_ALL); };
    auto join = [&](StepLane lane) { push(STEP_JOIN, lane, 0, 0, STEP_PART_ALL); };
    auto xop = [&](StepKind kind, unsigned arg = 0, StepPart part = STEP_PART_ALL, StepLane lane = STEP_MAIN) { push(kind, lane, 0, arg, part); };

    const int defer = form == STEP_FORM_PHASE ? 0 : form == STEP_FORM_STEP ? 2 : 1;
    const bool large = c->m > SVGP_M_MAX;
    // Measured on MI355X (tools/fork_probe.py): a fork + join costs ~10 us of cross-stream signalling.  The kernel-matrix reverse
    // pass || encoder reverse pass branch hides ~20 us, which pays only in the per-phase-graph replay form (phase 2: 110 -> 100 us)
    // and loses in the eager in-order form (261 -> 283 us per step), so it is opt-in: SVGP_SIDE_STREAMS=1.
    const bool fork2 = sc.side_small_m;
    // Large-m path: the tail of the forward factor stage ((A_hat + jI)^-1, its log det, KL: a whole batched inverse that only
    // the reverse factor stage and the final ELBO need) runs on side branch 1, beside the row stage, the decoder and the
    // reverse statistics.  That hides ~140 us at config 3 for ~10 us of signalling, so it is on unless SVGP_SIDE_STREAMS=0.
    // Not with cfg.titsias: svgp_gp_titsias_fwd inverts its own batch through the SAME inverse scratch (ws.scr_inv) on the
    // caller's stream, and the early reverse half would only multiply zero seeds.
    const bool fork1 = large && !c->titsias && !sc.side_off;
    // 64 < m < 512, phases issued back to back (round 5): everything of the forward factor stage that is a function of the KERNEL
    // MATRICES alone -- (K + jI)^-1 and its log det, Kn Ki, q, W = (Kn Ki) K, P^T = K Ki: one single-matrix blocked inverse (a chain
    // of 8 block steps, as long as the channel batch's) and three products -- goes to side branch 1 right behind the kernel
    // matrices, beside the forward statistics (the sharded form: and exchange point 1) and the channel inverses, instead of behind
    // them on the caller's stream.  Joined where u = Ki mu needs it.  SVGP_KONLY_BRANCH=0: the in-line order.
    const bool ksplit = fork1 && defer && c->m < SVGP_CHOL_INVERSE_MIN_M && sc.konly_branch;
    // m <= 64 (round 6): pass 2 of the reverse row stage (the sums over channels, consumed by the kernel-matrix VJP only) rides in the
    // encoder's reverse launch in front of the VJP workgroups.  Not with cfg.titsias (its reverse stage adds to Kbar / Knbar in
    // between), the split gradient exchange (phase 4) or SVGP_ENC_KM_MERGE=0.
    const bool sum_rides = !large && !fork2 && !c->titsias && sc.enc_km_merge && sc.sum_merge;
    const bool aji_in_dec = c->m <= 32 && !c->titsias && sc.dec_split && sc.aji_dec;
    // Everything of the forward factor stage behind Si, t, u, and the d / L3 half of the forward row stage, is first read BEHIND the
    // decoder launch: it rides there (the riders that already finish (A_hat + jI)^-1) and in pass 1 of the reverse row stage.  Only
    // where the step is issued whole (a stand-alone phase 1 must leave d, M2 and KL behind) and the fused decoder launch has riders.
    P.fwd_split = (form == STEP_FORM_STEP || form == STEP_FORM_DP) && aji_in_dec && sc.dec_fuse && sc.fwd_split;
    // the reverse statistics at the head of the reverse factor launch: only where nothing is exchanged between the two
    const bool stat_rides = defer == 2 && !large && !c->titsias && c->L <= 56 && sc.dec_split && sc.stat_merge;
    // The late reverse half alone is valid only if the early half was issued on this workspace: a whole-step form knows, the
    // stand-alone phase is told (a caller that ran the phase-1 stages through the individual entry points, or changed
    // SVGP_SIDE_STREAMS in between, gets the full reverse factor stage).
    const bool early = form == STEP_FORM_PHASE ? large && early_issued : fork1;
    const bool sharded = form == STEP_FORM_DP && large && c->L % nranks == 0 && !c->titsias && !c->kl_form;
    const bool split = form == STEP_FORM_DP && !sharded && c->split_grad_exchange;
    const bool pack = sharded && (sc.dp_pack < 0 ? svgp_dp_pack_rule(c->m) : sc.dp_pack != 0);

    auto phase0 = [&] {
        run(STEP_ST_ENC_KM_FWD);                                // one launch for the encoder and the kernel matrices
        // (The K-only branch is FORKED here but its launches are ISSUED behind the statistics': the host -- and a replayed graph,
        // which submits its nodes in capture order -- takes ~2.5 us per launch, and the branch's 15 launches in front of the
        // statistics' first kernel left the caller's stream idle for 36 us in the kernel trace.)
        if (ksplit) fork(STEP_SIDE1);
        run(STEP_ST_STATS_FWD);
        if (ksplit) run(STEP_ST_FACTOR_FWD_PIECES, STEP_SIDE1, SVGP_FWD_K);
        if (c->titsias) run(STEP_ST_TIT_STATS);
    };
    // the decoder pair; m <= 64 with the split on: the `_pre` forms read the effective up-convolution weights phase 0 of this step
    // left in ws.dec_weff
    auto decoder = [&](bool pre) {
        if (pre && sc.dec_fuse) {
            // SVGP_DEC_FUSE: the two launches of the branch below as one (same grid, workgroup n consumes only its own data; same bits)
            run(aji_in_dec ? STEP_ST_DEC_FUSED_AJI : STEP_ST_DEC_FUSED);
        } else if (pre) {
            run(STEP_ST_DEC_FWD_PRE);
            run(aji_in_dec ? STEP_ST_DEC_BWD_DATA_PRE_AJI : STEP_ST_DEC_BWD_DATA_PRE);
        } else {
            run(STEP_ST_DEC_FWD);
            run(STEP_ST_DEC_BWD);
        }
    };
    auto phase1 = [&] {
        if (ksplit) {                                           // the channel block; then what needs the branch's (K + jI)^-1 too
            run(STEP_ST_FACTOR_FWD_PIECES, STEP_MAIN, SVGP_FWD_SIG);
            join(STEP_SIDE1);
            run(STEP_ST_FACTOR_FWD_PIECES, STEP_MAIN, SVGP_FWD_KL);
        } else {
            run(STEP_ST_FACTOR_FWD_DEFER_AJI);                  // m <= 64: (A_hat + jI)^-1 finishes inside a later launch
        }
        // m > 64: the tail of the stage and the early half of the REVERSE factor stage (no reverse statistic needed; phase 2 then
        // runs the late half only) go to the side branch.  The branch is FORKED here but ISSUED behind the row stage: its ~25
        // launches take the host ~100 us to enqueue, during which the caller's stream had nothing to run (config 3, kernel trace of
        // round 4: a 101 us hole in front of the row stage's product) -- the branch has that much slack, the caller's stream none.
        if (fork1) fork(STEP_SIDE1);
        run(aji_in_dec ? STEP_ST_POST_FWD : STEP_ST_POST_FWD_AJI);
        if (large) {
            run(STEP_ST_FACTOR_FWD_AJI_TAIL, fork1 ? STEP_SIDE1 : STEP_MAIN);
            if (fork1) { run(STEP_ST_FACTOR_BWD_EARLY, STEP_SIDE1); P.early = true; }
        }
        if (c->titsias) run(STEP_ST_TIT_FWD);
        decoder(!large && sc.dec_split);
        if (!stat_rides) run(STEP_ST_STATS_BWD);                // (else: at the head of phase 2's first launch)
        if (fork1 && !defer) join(STEP_SIDE1);                  // phase-at-a-time callers: joined before the phase returns
    };
    // ph 2; 4: up to and including the kernel-matrix reverse pass + gradient reduction part 1 (cfg.split_grad_exchange); 5: the
    // encoder's reverse pass + gradient reduction part 2
    auto phase2 = [&](int ph) {
        if (ph == 5) {
            run(STEP_ST_ENC_BWD);
            run(STEP_ST_GRAD_REDUCE_PART, STEP_MAIN, 2);
            return;
        }
        if (early) {
            run(STEP_ST_FACTOR_BWD_LATE_A);                     // what does not read the branch's results: before the join
            join(STEP_SIDE1);                                   // (a no-op unless phase 1 left the branch open)
            // round 6: the single-matrix chain of the gradient of Ki (five ~9 us launches) on the branch that has just been joined,
            // beside the channel block on the caller's stream; SVGP_KBAR_BRANCH=0: one after the other
            if (sc.kbar_branch) {
                fork(STEP_SIDE1);
                run(STEP_ST_FACTOR_BWD_LATE_B_KBAR, STEP_SIDE1);
                run(STEP_ST_FACTOR_BWD_LATE_B_CHANNELS);
                join(STEP_SIDE1);
                run(STEP_ST_FACTOR_BWD_LATE_B_FINAL);
            } else {
                run(STEP_ST_FACTOR_BWD_LATE_B);
            }
        } else {
            // channel sum Kbar: inside the next launch; m <= 64: + the decoder's weight gradients as riders (phase 1 ran the data half)
            run(stat_rides ? STEP_ST_STATS_FACTOR_BWD_WGRAD
                           : !large && sc.dec_split ? STEP_ST_FACTOR_BWD_NOFINAL_WGRAD : STEP_ST_FACTOR_BWD_NOFINAL);
        }
        const bool sums = ph == 2 && sum_rides;
        run(sums ? STEP_ST_POST_BWD_ROWS : STEP_ST_POST_BWD_FINAL);
        if (c->titsias) run(STEP_ST_TIT_BWD);
        // (m > 64, measured round 5: the kernel-matrix reverse pass on side branch 0 beside the encoder's does NOT overlap -- 68 KB +
        // 104 KB of LDS per workgroup do not fit one CU; the kernel-matrix launch stretched from 49 to 103 us and the step was unchanged)
        if (ph == 4) {
            run(STEP_ST_KM_BWD_PARTIALS);
            run(STEP_ST_GRAD_REDUCE_PART, STEP_MAIN, 1);
            return;
        }
        if (sums) {
            run(STEP_ST_ENC_BWD_KM_SUM);
        } else if (!large && !fork2 && sc.enc_km_merge) {
            run(STEP_ST_ENC_BWD_KM);
        } else {
            if (fork2) fork(STEP_SIDE0);
            run(STEP_ST_KM_BWD_PARTIALS, fork2 ? STEP_SIDE0 : STEP_MAIN);
            run(STEP_ST_ENC_BWD);
            if (fork2) join(STEP_SIDE0);
        }
        run(STEP_ST_GRAD_REDUCE_ALL);
    };
    auto phase3 = [&] { run(adam ? STEP_ST_ADAM_FINALIZE : STEP_ST_FINALIZE_NOADAM); };
    // one of points 1..4 of the sharded form: [pack |] one grouped collective over a symmetric block and two more members [| unpack].
    // fork_between: branch 1 is forked behind the pack, in front of the collective.
    auto point = [&](int idx, StepKind coll, StepBlock sym, StepBlock b1, StepBlock b2, StepPart packed, StepPart unpacked, bool fork_between) {
        xop(STEP_POINT_BEGIN, idx);
        if (pack) xop(STEP_PACK, sym, packed);
        if (fork_between) fork(STEP_SIDE1);
        xop(STEP_GROUP_BEGIN);
        xop(coll, sym, pack ? STEP_PART_PACKED : STEP_PART_ALL);
        xop(coll, b1);
        if (b2 != STEP_BLK_COUNT) xop(coll, b2);
        xop(STEP_GROUP_END);
        if (pack) xop(STEP_UNPACK, sym, unpacked);
        xop(STEP_POINT_END, idx);
    };

    P.side = fork2 || large;
    if (form == STEP_FORM_PHASE) {
        if (phase == 0) phase0();
        else if (phase == 1) phase1();
        else if (phase == 3) phase3();
        else phase2(phase);
    } else if (form == STEP_FORM_STEP) {
        phase0(); phase1(); phase2(2); phase3();
    } else if (!sharded) {
        phase0();
        xop(STEP_ALLREDUCE, STEP_BLK_statA);
        phase1();
        xop(STEP_ALLREDUCE, STEP_BLK_statB);
        if (split) {
            // The closing all-reduce in two parts (round 6; prepared for small-message all-reduce latencies above ~20 us on 8 ranks,
            // where three of them per 165 us step would cap weak scaling below 6x): gradC[n_enc:] -- decoder + GP parameters + scalar
            // sums -- is complete once the kernel-matrix reverse pass and reduction part 1 are done and travels on the side branch WHILE
            // the encoder's reverse pass runs on the caller's stream; gradC[:n_enc] follows it.  Same sums, same order on every rank.
            P.side = true;
            phase2(4);
            fork(STEP_SIDE1);
            xop(STEP_ALLREDUCE, STEP_BLK_gradC_hi, STEP_PART_ALL, STEP_SIDE1);
            phase2(5);
            xop(STEP_ALLREDUCE, STEP_BLK_gradC_lo);
            join(STEP_SIDE1);
        } else {
            phase2(2);
            xop(STEP_ALLREDUCE, STEP_BLK_gradC);
        }
        phase3();
    } else {
        // Channel-sharded form: the (L,m,m) statistics are reduce-SCATTERED over the channels, every rank factors its L / G channels
        // and what the row stages need is all-gathered (comm.hip has the exchange).  Here fork1 == !SVGP_SIDE_STREAMS=0.
        P.sharded = true; P.pack = pack; P.side = fork1;
        run(STEP_ST_ENC_KM_FWD);
        // the channel-independent block -- every rank computes it, and with L / G channels per rank it is most of the stage
        if (ksplit) fork(STEP_SIDE1);
        run(STEP_ST_STATS_FWD);                  // (issued first: the branch's 15 launches would hold the caller's stream back)
        if (ksplit) run(STEP_ST_BIG_FACTOR_FWD, STEP_SIDE1, SVGP_FWD_K);
        point(1, STEP_REDUCE_SCATTER, STEP_BLK_S, STEP_BLK_v, STEP_BLK_COUNT, STEP_PART_ALL, STEP_PART_WINDOW, false);
        if (ksplit) {                            // window factor stage without its tail
            run(STEP_ST_BIG_FACTOR_FWD, STEP_MAIN, SVGP_FWD_SIG);
            join(STEP_SIDE1);
            run(STEP_ST_BIG_FACTOR_FWD, STEP_MAIN, SVGP_FWD_KL);
        } else {
            run(STEP_ST_BIG_FACTOR_FWD, STEP_MAIN, SVGP_FWD_HEAD);
        }
        // Point 2.  The window goes to the wire format first, so that the side branch never reads a block that is being rewritten
        // (Sigma^-1 is exactly symmetric in memory: its lower tiles ARE the matrix and the owner keeps its own window as it is; the
        // unpack behind the collective writes the other ranks' windows only).  The tail and the early half of the reverse factor
        // stage go to the side branch, beside the all-gather, the row stage, the networks and the reverse statistics: FORKED behind
        // the pack (the branch depends on the window stage only), ISSUED behind the collective -- enqueued first, the branch's GEMMs
        // fill every CU and the collective's kernel waits for a slot: with a 1-rank communicator the point measured 245 us at
        // config 3 for a no-op gather (round 3: 260 us), and the row stage on the caller's stream waits behind it.
        point(2, STEP_ALLGATHER, STEP_BLK_Si, STEP_BLK_t, STEP_BLK_u, STEP_PART_WINDOW, STEP_PART_OTHERS, fork1);
        // (the row stage is issued first: the branch's ~25 launches take the host ~100 us to enqueue, during which the caller's
        // stream would have nothing to run; the branch has that much slack)
        run(STEP_ST_POST_FWD);
        run(STEP_ST_BIG_FACTOR_FWD, fork1 ? STEP_SIDE1 : STEP_MAIN, SVGP_FWD_TAIL);
        if (fork1) run(STEP_ST_BIG_FACTOR_BWD, STEP_SIDE1, SVGP_BWD_EARLY);
        decoder(false);
        run(STEP_ST_STATS_BWD);
        point(3, STEP_REDUCE_SCATTER, STEP_BLK_A2, STEP_BLK_ud, STEP_BLK_td, STEP_PART_ALL, STEP_PART_WINDOW, false);
        if (fork1) {
            join(STEP_SIDE1);
            // round 6 (as on one GPU): the single-matrix chain of the gradient of Ki -- five small launches that every rank runs in full,
            // while the channel block covers its L / G channels only -- on the branch that has just been joined, beside the channel
            // block.  SVGP_KBAR_BRANCH=0: one launch after the other.
            if (sc.kbar_branch) {
                run(STEP_ST_BIG_FACTOR_BWD, STEP_MAIN, SVGP_BWD_LATE_A);
                fork(STEP_SIDE1);
                run(STEP_ST_BIG_FACTOR_BWD, STEP_SIDE1, SVGP_BWD_KBAR);
                run(STEP_ST_BIG_FACTOR_BWD, STEP_MAIN, SVGP_BWD_CHANNELS);
                join(STEP_SIDE1);
                run(STEP_ST_BIG_FACTOR_BWD, STEP_MAIN, SVGP_BWD_FINAL);
            } else {
                run(STEP_ST_BIG_FACTOR_BWD, STEP_MAIN, SVGP_BWD_LATE);
            }
        } else {
            run(STEP_ST_BIG_FACTOR_BWD, STEP_MAIN, SVGP_BWD_ALL);
        }
        point(4, STEP_ALLGATHER, STEP_BLK_Ssym, STEP_BLK_vbar, STEP_BLK_KL, STEP_PART_WINDOW, STEP_PART_ALL, false);
        run(STEP_ST_POST_BWD);
        run(STEP_ST_KM_BWD_PARTIALS);
        run(STEP_ST_ENC_BWD);
        run(STEP_ST_GRAD_REDUCE_ALL);
        xop(STEP_ALLREDUCE, STEP_BLK_gradC);     // point 5: gradients + scalar sums
        phase3();
    }
    return P.n <= SVGP_STEP_MAX_OPS ? SVGP_OK : SVGP_ERR_INVALID;
}
