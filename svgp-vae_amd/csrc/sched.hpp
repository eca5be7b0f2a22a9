// The library's schedule switches: environment variables that choose between launch orders / merged and un-merged launch forms
// that compute the same bits (DESIGN.md "Schedule switches" has the table: values, defaults, the test that compares the settings).
// This is the only reader.  An exported entry point that consults a switch calls sched_read() once per call and passes the struct
// down, so that a test may flip a variable between two calls of one process and no call sees two values of one switch.
// (The one other getenv of csrc/ is the SVGP_CONV_ROWS test hook in conv_taps.hip.)
#pragma once
#include <cstdlib>

struct SvgpSched {
    bool dec_split;       // SVGP_DEC_SPLIT     m <= 64: decoder reverse pass as data half (phase 1) + weight riders (phase 2); 0: one kernel
    bool enc_km_merge;    // SVGP_ENC_KM_MERGE  m <= 64: kernel-matrix VJP + encoder reverse pass in one launch; 0: two launches
    bool sum_merge;       // SVGP_SUM_MERGE     m <= 64: pass 2 of the reverse row stage rides in that launch too; 0: its own launch
    bool stat_merge;      // SVGP_STAT_MERGE    m <= 64, single GPU: reverse statistics ride in the reverse factor launch; 0: their own
    bool aji_dec;         // SVGP_AJI_DEC       m <= 32: deferred (A_hat + jI)^-1 rides in the decoder's data-reverse launch; 0: row stage
    bool dec_fuse;        // SVGP_DEC_FUSE      m <= 64, split on: decoder forward + data-reverse launches as ONE launch; 0: two launches
    bool fwd_split;       // SVGP_FWD_SPLIT     m <= 32, decoder riders + fused decoder on: only Si, t, u ahead of the decoder (step_plan.hpp); 0: full forms
    bool stat_four;       // SVGP_STAT_FOUR     set (any value): the four-matrix form of the merged statistics launch also where five fit
    bool konly_branch;    // SVGP_KONLY_BRANCH  64 < m < 512: the kernel-matrix-only block of the forward factor stage on side branch 1; 0: in line
    bool kbar_branch;     // SVGP_KBAR_BRANCH   m > 64: the single-matrix chain of the gradient of Ki beside the channel block; 0: in line
    bool stream_probe;    // SVGP_STREAM_PROBE  side streams picked by the concurrency probe; 0: the first two created
    // SVGP_SIDE_STREAMS, first character: '0' no side branch anywhere; '1' additionally opts in to the m <= 64 fork (kernel-matrix
    // reverse pass beside the encoder's; pays only under per-phase graph replay); '2' is a SPRITES-only host mode (sprites.py) and
    // means "unset" here; unset: the large-m branches on, the m <= 64 fork off.
    bool side_off;        //   '0'
    bool side_small_m;    //   '1'
    int dp_pack;          // SVGP_DP_PACK       channel-sharded step: tile-packed symmetric exchange 1 / 0; -1 (unset): svgp_dp_pack_default(m)
};

inline SvgpSched sched_read() {
    auto on = [](const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); };
    SvgpSched s;
    s.dec_split = on("SVGP_DEC_SPLIT");
    s.enc_km_merge = on("SVGP_ENC_KM_MERGE");
    s.sum_merge = on("SVGP_SUM_MERGE");
    s.stat_merge = on("SVGP_STAT_MERGE");
    s.aji_dec = on("SVGP_AJI_DEC");
    s.dec_fuse = on("SVGP_DEC_FUSE");
    s.fwd_split = on("SVGP_FWD_SPLIT");
    s.stat_four = getenv("SVGP_STAT_FOUR") != nullptr;
    s.konly_branch = on("SVGP_KONLY_BRANCH");
    s.kbar_branch = on("SVGP_KBAR_BRANCH");
    s.stream_probe = on("SVGP_STREAM_PROBE");
    const char* side = getenv("SVGP_SIDE_STREAMS");
    s.side_off = side && side[0] == '0';
    s.side_small_m = side && side[0] == '1';
    const char* pack = getenv("SVGP_DP_PACK");
    s.dp_pack = pack ? (pack[0] != '0' ? 1 : 0) : -1;
    return s;
}
