// The model-level forward orchestration: the four forward passes and the log-mel front-end, workspace sizing, the checks and the graph-replay
// forward behind fv_forward*, and the per-launch profiler ABI.
//
// The engine owns: folded + MFMA-packed weights in HBM, and the static launch plan of a generator forward.
// Per forward it only enqueues kernels on the caller's stream into the caller's workspace (no allocation, no sync).
//
// Reference call stack replaced (paths under the reference project's fish_vocoder/):
//   test.py:89 -> models/gan.py:286 -> modules/generators/hifigan.py:226-249 (HiFiGAN)
//                                       modules/generators/bigvgan.py:352-371 (BigVGAN)
//                                       modules/generators/unify.py:18-33 + encoders/convnext.py:206-214
//                                       + generators/vocos.py:43-69 (Vocos)
#include "engine_internal.h"

// ------------------------------------------------------------------------------------------------
// forward passes
// ------------------------------------------------------------------------------------------------
fv_status fv_engine::ensure_branch_streams(int nk) {
    if ((int)bstreams.size() >= nk - 1 && !bev_fork.empty()) return FV_OK;
    while ((int)bstreams.size() < nk - 1) {
        hipStream_t st;
        FV_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        bstreams.push_back(st);
    }
    const size_t stages = std::max<size_t>(ups.stages.size(), 1);
    while (bev_fork.size() < stages) {
        hipEvent_t e;
        FV_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        bev_fork.push_back(e);
    }
    while (bev_last.size() < stages * (size_t)nk) {
        hipEvent_t e;
        FV_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        bev_last.push_back(e);
    }
    return FV_OK;
}

namespace {

// Workspace of the upsampler: cur / S / Y plus (XB, XT, XA) per concurrent branch = 3 + 3 * num_kernels buffers of `me` floats
struct UpsWorkspace {
    float* ws;
    int64_t me;
    float *cur, *S, *Y;   // the running activation, the upsampler conv's output (the branches' input), the stage output (swapped with cur after every stage)
    UpsWorkspace(float* ws_, int64_t me_) : ws(ws_), me(me_), cur(ws_), S(ws_ + me_), Y(ws_ + 2 * me_) {}
    float* XB(int j) const { return ws + (size_t)(3 + 3 * j) * me; }
    float* XT(int j) const { return ws + (size_t)(4 + 3 * j) * me; }
    float* XA(int j) const { return ws + (size_t)(5 + 3 * j) * me; }
};

enum BranchForm { BRANCH_PAIRS, BRANCH_AMP, BRANCH_LAYERS };   // run_branch_pairs / run_branch_amp / run_branch_layers
// where the stage's branch mean is formed
enum MeanForm {
    MEAN_IN_BRANCHES,   // chain: accumulated into Y by the branches' last epilogues
    MEAN_IN_NEXT_UP,    // tree: the next stage's upsampler conv forms it while staging its input (conv_mfma_impl.h, SUM3)
    MEAN_IN_POST,       // tree, last stage: conv_post (HiFiGAN) / activation_post (BigVGAN) forms it while loading its input
    MEAN_KERNEL,        // tree: mean_of_three_kernel into Y after the join
};
struct BranchPlan {
    int j;         // the branch (UpStage::branches)
    int bj;        // its buffer set XB / XT / XA
    int stream;    // 0: the caller's stream, j > 0: branch stream j - 1
    BranchForm form;
    float* y_last;   // the branch's last kernel writes here, as (y_last [+ v]) * scale_last
    int mode_last;
    float scale_last;
};
struct StagePlan {
    int B, t, ch;
    bool tree;     // the form of the branch mean (plan_stage)
    MeanForm mean;
    bool dbg_here;   // FV_DEBUG_STOP names this stage: the forward ends after it, and the per-layer branches after dilation pair dbg_pair (dbg_half 0: after its c1)
    int dbg_pair, dbg_half;
    BranchPlan br[FV_MAX_KERNELS];   // in the order the host enqueues them
};

// the chip-filling gate of the wide (C = 64 / 128) fused pairs: two workgroups per CU in the F(2,3) C = 128 tiling
static bool pair_fills_chip(int B, int t) { return (long long)B * ((t + 125) / 126) >= 2LL * num_cus(); }

BranchForm plan_branch_form(const fv_engine& e, const ResBranch& br, bool dbg_here, int B, int t, int ch) {
    const EngineOptions& o = e.opt;
    // HiFiGAN narrow stages: the whole (c1, c2) pair in one kernel, intermediate kept in LDS.  Not in place
    // (workgroups read their neighbours' halo), so the branch ping-pongs S -> XB -> XT -> Y.
    // (C = 64 / 128 pairs — k = 3 only — fuse when the launch fills the chip; a single clip's 44 - 88 tiles are better served by the
    //  per-layer latency kernels: conv_wino_lat_impl.h)
    const bool fuse_narrow = ch <= o.pair_max_c && pair_supported(ch, br.k, br.dil[0]) && pair_supported(ch, br.k, br.dil[1]) &&
                             pair_supported(ch, br.k, br.dil[2]) && (ch < 64 || cur_invariant() || pair_fills_chip(B, t) || knobs().pair_wino4 == 2);   // (FV_PAIR_WINO4=2, tests: the wide pairs at any size)
    // f16x3 precision mode: the wide stages (C = 128 / 64) fuse too (pair_f16x3_impl.h)
    const bool fuse_wide = pair_f16x3_supported(br.c1[0], br.c2[0]) && pair_f16x3_supported(br.c1[1], br.c2[1]) &&
                           pair_f16x3_supported(br.c1[2], br.c2[2]);
    if (!e.ups.bigvgan && (fuse_narrow || fuse_wide) && o.fuse_pairs) return BRANCH_PAIRS;
    // BigVGAN narrow stages (C = 32 / 64): each conv runs with its anti-aliased SnakeBeta fused in front (amp_conv.hip) —
    // no activation launches, no activated tensors in HBM
    bool fuse_amp = e.ups.bigvgan && o.fuse_amp_convs && !dbg_here && ch <= o.fuse_amp_max_c && br.k <= o.fuse_amp_max_k;
    for (int n = 0; n < FV_MAX_DILATIONS && fuse_amp; ++n)
        fuse_amp = br.c1[n].precision == FV_PRECISION_F32 && br.c2[n].precision == FV_PRECISION_F32 && br.c1[n].c_in == ch &&
                   br.c1[n].c_out == ch && br.c2[n].c_in == ch && br.c2[n].c_out == ch && br.c1[n].k == br.k && br.c2[n].k == br.k &&
                   amp_conv_supported(ch, br.k, br.c1[n].dil) && br.c2[n].dil == 1 &&
                   br.c1[n].padding == (br.k - 1) / 2 * br.c1[n].dil && br.c2[n].padding == (br.k - 1) / 2 && (long long)ch * t < (1LL << 30);
    return fuse_amp ? BRANCH_AMP : BRANCH_LAYERS;
}

// tree form, after the join: who forms Y = ((y0 + y1) + y2) / 3 — the same additions in the same order as the accumulate chain
MeanForm plan_tree_mean(const fv_engine& e, const Knobs& kn, bool dbg_here, int stage_idx, int B, int t) {
    const UpsamplerModel& ups = e.ups;
    const int n_stages = (int)ups.stages.size();
    // the next stage's upsampler conv forms the mean while staging its input (conv_mfma_impl.h, SUM3); the last stage's
    // output goes through mean_of_three_kernel (its consumers are the narrow post kernels)
    const bool fuse_mean = !kn.no_sum3;
    if (stage_idx + 1 < n_stages && fuse_mean && !dbg_here) return MEAN_IN_NEXT_UP;
    if (stage_idx + 1 == n_stages && fuse_mean && e.opt.post_mean_fused && !dbg_here &&
        (ups.bigvgan || conv_narrow_sum3_ok(B, ups.post_cin, t, 1, ups.cfg.post_conv_kernel_size, get_padding(ups.cfg.post_conv_kernel_size))))
        return MEAN_IN_POST;
    return MEAN_KERNEL;
}

// Every decision of one stage — t: its length after the upsampler conv; multi: the branches run on their own streams.  Enqueues nothing.
StagePlan plan_stage(const fv_engine& e, const Knobs& kn, const UpsWorkspace& w, int stage_idx, int B, int t, bool multi) {
    const EngineOptions& o = e.opt;
    const UpStage& stg = *e.ups.stages[stage_idx];
    const int nk = e.ups.cfg.num_kernels;
    StagePlan sp{B, t, stg.ch};
    sp.dbg_here = o.debug_stop >= 0 && o.debug_stop / 100 == stage_idx;
    sp.dbg_pair = (o.debug_stop / 10) % 10;
    sp.dbg_half = o.debug_stop % 10;
    // ParralelBlock / stack-mean of the three ResBlock1 / AMPBlock branches (hifigan.py:132-133, bigvgan.py:358-365)
    // Y = ((y0 + y1) + y2) / 3 is formed in one of two ways — the same additions in the same order, so bit-identical:
    //   chain  y0 -> Y, (Y + y1) -> Y, (Y + y2) / 3 -> Y in the branches' last epilogues, ordered by events (single stream, other
    //          branch counts, FV_BRANCH_MEAN=chain)
    //   tree   the branches keep their outputs in their own buffers and mean_of_three_kernel forms Y after the join.
    // The chain makes each branch's last kernel wait for the previous branch's: a single clip paid 20-65 us of cross-queue
    // waits per stage (tools/latency_timeline.py), and at B = 32 the k = 7 and k = 11 branches' final convs ran one after the
    // other, alone on the chip, at the end of every stage (rocprofv3 trace).  Without it the host is also free to enqueue the
    // branches longest first (k = 11, 7, 3): a replayed graph starts sibling nodes in creation order, and the k = 11 chain —
    // every stage's critical path — used to start last (53 us after the fork in stage 0 of a single clip).  Tree + longest
    // first: B = 1 1.07 -> 0.97 ms per forward, B = 32 15.12 -> 15.00 ms (the extra pass over four tensors included; with
    // the branches enqueued shortest first the tree was 0.1 ms *slower* than the chain at B = 32).  Summing the other two
    // outputs in the last branch's final epilogue instead of a separate kernel measured 15.02 / 1.04 ms: not kept.  Neither
    // were: two streams, the longest branch on the caller's stream, a wake-up kernel on the side queues, stream priorities.
    // Narrow stages (ch <= chain_max_c, FV_CHAIN_MAX_C): the chain, so that the HBM-bound consumers — the last upsamplers, conv_post — read ONE
    // tensor instead of three; the k = 3 / 7 / 11 branches finish in that order anyway
    // Profiling runs (one stream, hipEvents around every launch: the source of the bench line's `roofline`) take the tree form too since round 6 — the
    // branches back to back, each into its own buffers — so that the table holds the kernel instances the shipped step launches: the chain's last
    // epilogues accumulate (the slow general epilogue of conv_wino44: 321 against 265 us for the dominant layer) and its upsamplers read one tensor,
    // neither of which the three-stream step ever runs.
    sp.tree = (multi || e.profiling || o.single_tree) && nk == 3 && !kn.branch_mean_chain && stg.ch > o.chain_max_c;
    sp.mean = sp.tree ? plan_tree_mean(e, kn, sp.dbg_here, stage_idx, B, t) : MEAN_IN_BRANCHES;
    for (int jj = 0; jj < nk; ++jj) {
        BranchPlan& bp = sp.br[jj];
        bp.j = sp.tree ? nk - 1 - jj : jj;   // tree: longest branch first
        bp.stream = multi ? bp.j : 0;
        bp.bj = (multi || sp.tree) ? bp.j : 0;   // single-stream chain: branches run back to back and share one buffer set
        bp.form = plan_branch_form(e, *stg.branches[bp.j], sp.dbg_here, B, t, stg.ch);
        bp.y_last = sp.tree ? w.XB(bp.bj) : w.Y;   // tree: the branch keeps its own output, summed after the join
        bp.mode_last = !sp.tree && bp.j > 0 ? OUT_ACCUM : OUT_SET;
        bp.scale_last = !sp.tree && bp.j == nk - 1 ? 1.0f / (float)nk : 1.0f;
    }
    return sp;
}

// The nk ResBlock branches of a stage are independent until the stack-mean: they run on their own streams
// (fork after the upsampler conv, join after the last branch) so that one branch's tail / barrier phases are
// filled by the others' workgroups.  The MRF accumulate into Y (chain form) stays ordered j = 0, 1, 2 through events.
// With !multi every operation is a no-op and every branch runs on the caller's stream.
struct BranchOrder {
    fv_engine& e;
    hipStream_t s;   // the caller's stream
    bool multi;
    int nk;
    int stage = 0;
    bool tree = false;
    hipStream_t stream(int idx) const { return idx > 0 ? e.bstreams[idx - 1] : s; }
    hipEvent_t last(int j) const { return e.bev_last[stage * nk + j]; }
    fv_status fork(int stage_idx, bool tree_) {   // after the upsampler conv
        stage = stage_idx;
        tree = tree_;
        if (multi) FV_HIP_CHECK(hipEventRecord(e.bev_fork[stage], s));
        return FV_OK;
    }
    fv_status enter(const BranchPlan& bp) {
        if (bp.stream > 0) FV_HIP_CHECK(hipStreamWaitEvent(stream(bp.stream), e.bev_fork[stage], 0));
        return FV_OK;
    }
    // ordering of the accumulate into Y: branch j's last kernel runs after branch j-1's
    fv_status before_last(const BranchPlan& bp) {
        if (bp.stream > 0 && !tree) FV_HIP_CHECK(hipStreamWaitEvent(stream(bp.stream), last(bp.j - 1), 0));
        return FV_OK;
    }
    fv_status after_last(const BranchPlan& bp) {
        if (multi) FV_HIP_CHECK(hipEventRecord(last(bp.j), stream(bp.stream)));
        return FV_OK;
    }
    fv_status join() {
        if (!multi) return FV_OK;
        if (tree) {   // all three
            for (int j = 1; j < nk; ++j) FV_HIP_CHECK(hipStreamWaitEvent(s, last(j), 0));
        } else {      // chain: the last branch's final kernel is ordered after every other branch's
            FV_HIP_CHECK(hipStreamWaitEvent(s, last(nk - 1), 0));
        }
        return FV_OK;
    }
};

ConvRun conv_run(int B, int t_in, const float* x, float* y) {
    ConvRun r;
    r.batch = B;
    r.t_in = t_in;
    r.x = x;
    r.y = y;
    return r;
}

// The whole (c1, c2) pair in one kernel: S -> XB -> XT -> y_last
fv_status run_branch_pairs(const ResBranch& br, const UpsWorkspace& w, const StagePlan& sp, const BranchPlan& bp, BranchOrder& ord) {
    const hipStream_t bs = ord.stream(bp.stream);
    fv_status st;
    const float* src = w.S;
    // wide k = 3 pairs of a launch that fills the chip: the F(4,3) family (conv_pair_run keeps F(2,3) in batch-invariant mode, for DIRECT and under
    // FV_PAIR_WINO4=0) — streams, session pools, ragged rows and single clips run below the gate or batch-invariant, and keep their bits
    const bool quad = sp.ch >= 64 && !cur_invariant() && pair_fills_chip(sp.B, sp.t);
    for (int n = 0; n < FV_MAX_DILATIONS; ++n) {
        const bool last = n == FV_MAX_DILATIONS - 1;
        float* dst = last ? bp.y_last : (n == 0 ? w.XB(bp.bj) : w.XT(bp.bj));
        if (last && (st = ord.before_last(bp))) return st;
        if ((st = conv_pair_run(br.c1[n], br.c2[n], src, dst, sp.B, sp.t, last ? bp.mode_last : OUT_SET, last ? bp.scale_last : 1.0f, bs, quad)))
            return st;
        src = dst;
    }
    return FV_OK;
}

// BigVGAN: amp_conv for c1 and for c2 + residual
fv_status run_branch_amp(const ResBranch& br, const UpsWorkspace& w, const StagePlan& sp, const BranchPlan& bp, BranchOrder& ord) {
    const hipStream_t bs = ord.stream(bp.stream);
    const int B = sp.B, t = sp.t, ch = sp.ch, bj = bp.bj;
    fv_status st;
    for (int n = 0; n < FV_MAX_DILATIONS; ++n) {
        const float* src = n == 0 ? w.S : w.XB(bj);
        const bool last = n == FV_MAX_DILATIONS - 1;
        const AASnake &a1 = br.act[2 * n], &a2 = br.act[2 * n + 1];
        const double fl = 2.0 * ch * ch * br.k * (double)t * B, el = (double)B * ch * t * 4.0;
        char lbl[96];
        std::snprintf(lbl, sizeof(lbl), "amp_conv<k=%d d=%d C=%d>", br.k, br.c1[n].dil, ch);
        FV_PROF(bs, lbl, fl + 60.0 * B * ch * t, 2.0 * el,
                (launch_amp_conv(br.c1[n], src, w.XT(bj), nullptr, a1.d_alpha, a1.d_inv_beta, a1.d_up, a1.d_down, B, t, OUT_SET,
                                 1.0f, bs) ? FV_OK : FV_ERR_HIP));
        if (last && (st = ord.before_last(bp))) return st;
        std::snprintf(lbl, sizeof(lbl), "amp_conv<k=%d d=1 C=%d>+res", br.k, ch);
        FV_PROF(bs, lbl, fl + 60.0 * B * ch * t, (last && bp.mode_last == OUT_ACCUM ? 4.0 : 3.0) * el,
                (launch_amp_conv(br.c2[n], w.XT(bj), last ? bp.y_last : w.XB(bj), src, a2.d_alpha, a2.d_inv_beta, a2.d_up, a2.d_down, B, t,
                                 last ? bp.mode_last : OUT_SET, last ? bp.scale_last : 1.0f, bs) ? FV_OK : FV_ERR_HIP));
    }
    return FV_OK;
}

fv_status run_aa_snake(const AASnake& a, const float* x, float* y, const StagePlan& sp, hipStream_t bs) {
    FV_PROF(bs, "aa_snake", 60.0 * sp.B * sp.ch * sp.t, 8.0 * sp.B * sp.ch * sp.t,
            launch_aa_snake(x, y, a.d_alpha, a.d_inv_beta, a.d_up, a.d_down, sp.B, sp.ch, sp.t, bs));
    return FV_OK;
}

// One launch per conv (BigVGAN: and per activation, through XA)
fv_status run_branch_layers(const ResBranch& br, bool bigvgan, const UpsWorkspace& w, const StagePlan& sp, const BranchPlan& bp,
                                   BranchOrder& ord) {
    const hipStream_t bs = ord.stream(bp.stream);
    const int bj = bp.bj;
    const int act = bigvgan ? FV_ACT_NONE : FV_ACT_SILU;
    fv_status st;
    for (int n = 0; n < FV_MAX_DILATIONS; ++n) {
        if (sp.dbg_here && n > sp.dbg_pair) break;
        const float* src = n == 0 ? w.S : w.XB(bj);
        const bool last = n == FV_MAX_DILATIONS - 1;
        if (bigvgan && (st = run_aa_snake(br.act[2 * n], src, w.XA(bj), sp, bs))) return st;
        // xt = c1(act(x)); the second activation is fused into c1's epilogue for SiLU
        ConvRun r = conv_run(sp.B, sp.t, bigvgan ? w.XA(bj) : src, w.XT(bj));
        r.pre_act = r.post_act = act;
        if ((st = conv_layer_run(br.c1[n], r, bs))) return st;
        if (sp.dbg_here && n == sp.dbg_pair && sp.dbg_half == 0) break;
        if (bigvgan && (st = run_aa_snake(br.act[2 * n + 1], w.XT(bj), w.XA(bj), sp, bs))) return st;
        // x = c2(act(xt)) + x ; the last pair of each branch accumulates the branch mean into Y
        r = conv_run(sp.B, sp.t, bigvgan ? w.XA(bj) : w.XT(bj), last ? bp.y_last : w.XB(bj));
        r.res = src;
        if (last) {
            r.out_mode = bp.mode_last;
            r.out_scale = bp.scale_last;
            if ((st = ord.before_last(bp))) return st;
        }
        if ((st = conv_layer_run(br.c2[n], r, bs))) return st;
    }
    return FV_OK;
}

// x = ups[i](silu(x))  — HiFiGAN (hifigan.py:230-231); BigVGAN has no pre-activation (bigvgan.py:355-356); returns the stage's length through t
fv_status run_stage_up(fv_engine& e, const UpStage& stg, const UpsWorkspace& w, bool sum3, int B, int T, int& t, hipStream_t s) {
    ConvRun r = conv_run(B, t, w.cur, w.S);
    if (sum3) {   // the previous stage left its three branch outputs: the upsampler conv forms their mean itself
        r.x = w.XB(0);
        r.x2 = w.XB(1);
        r.x3 = w.XB(2);
        r.sum_tmp = w.cur;   // (kernels without the three-operand staging form it here first)
    }
    r.pre_act = e.ups.bigvgan ? FV_ACT_NONE : FV_ACT_SILU;
    if (const fv_status st = conv_layer_run(stg.up, r, s)) return st;
    t = (int)stg.up.out_len(t);
    if (e.ups.cfg.use_template) {   // x = x + noise_convs[i](template)  (hifigan.py:233-234)
        const int Ta = (int)e.ups.out_len(T);
        FV_PROF(s, "noise_conv_add", 2.0 * B * stg.ch * stg.nk * t, 8.0 * B * stg.ch * t,
                launch_noise_conv_add(e.cur_template, stg.d_nw, stg.d_nb, w.S, B, stg.ch, t, Ta, stg.nk, stg.nstride, stg.npad, s));
    }
    return FV_OK;
}

// activation_post -> conv_post -> tanh (hifigan.py:245-247 / bigvgan.py:367-369); sum3: the last stage left its three branch outputs
fv_status run_post(const UpsamplerModel& ups, const UpsWorkspace& w, bool sum3, float* d_out, int B, int t, hipStream_t s) {
    const float* post_in = w.cur;
    int pre = ups.cfg.post_activation;   // post_activation() (hifigan.py:213,245): SiLU by default
    const float pre_slope = ups.cfg.post_activation_slope;
    if (ups.bigvgan) {
        // (XA(0) is free again: every branch has joined)
        FV_PROF(s, sum3 ? "aa_snake sum3" : "aa_snake", 60.0 * B * ups.post_cin * t, (sum3 ? 16.0 : 8.0) * B * ups.post_cin * t,
                launch_aa_snake(sum3 ? w.XB(0) : w.cur, w.XA(0), ups.act_post.d_alpha, ups.act_post.d_inv_beta, ups.act_post.d_up,
                                ups.act_post.d_down, B, ups.post_cin, t, s, sum3 ? w.XB(1) : nullptr, sum3 ? w.XB(2) : nullptr));
        post_in = w.XA(0);
        pre = FV_ACT_NONE;
        sum3 = false;   // the mean is in: conv_post reads the activated tensor
    }
    const int qk = ups.cfg.post_conv_kernel_size;
    FV_PROF(s, sum3 ? "conv_post_narrow sum3" : "conv_post_narrow", 2.0 * B * ups.post_cin * qk * t, 4.0 * B * ((sum3 ? 3 : 1) * ups.post_cin + 1) * t,
            launch_conv_narrow(sum3 ? w.XB(0) : post_in, ups.d_wpost, ups.d_bpost, d_out, B, ups.post_cin, t, 1, qk, get_padding(qk), pre, FV_ACT_TANH,
                               pre_slope, s, sum3 ? w.XB(1) : nullptr, sum3 ? w.XB(2) : nullptr));
    return FV_OK;
}

}  // namespace

fv_status fv_engine::run_upsampler(const float* d_in, float* d_out, int B, int T, float* ws, hipStream_t s) {
    const int nk = ups.cfg.num_kernels, n_stages = (int)ups.stages.size();
    UpsWorkspace w(ws, (ups.max_elems(T) * B + 63) / 64 * 64);
    fv_status st;
    // Profiling runs stay on one stream so that per-kernel hipEvent durations do not overlap.
    const bool multi = opt.branch_streams && nk > 1 && !profiling;
    if (multi && (st = ensure_branch_streams(nk))) return st;
    BranchOrder ord{*this, s, multi, nk};
    // conv_pre (hifigan.py:227)
    if ((st = conv_layer_run(ups.conv_pre, conv_run(B, T, d_in, w.cur), s))) return st;
    int t = (int)ups.conv_pre.out_len(T);
    MeanForm mean = MEAN_IN_BRANCHES;   // of the previous stage
    for (int i = 0; i < n_stages; ++i) {
        const UpStage& stg = *ups.stages[i];
        if ((st = run_stage_up(*this, stg, w, mean == MEAN_IN_NEXT_UP, B, T, t, s))) return st;
        const StagePlan sp = plan_stage(*this, knobs(), w, i, B, t, multi);
        if ((st = ord.fork(i, sp.tree))) return st;
        for (int jj = 0; jj < nk; ++jj) {
            const BranchPlan& bp = sp.br[jj];
            const ResBranch& br = *stg.branches[bp.j];
            if ((st = ord.enter(bp))) return st;
            switch (bp.form) {
                case BRANCH_PAIRS: st = run_branch_pairs(br, w, sp, bp, ord); break;
                case BRANCH_AMP: st = run_branch_amp(br, w, sp, bp, ord); break;
                case BRANCH_LAYERS: st = run_branch_layers(br, ups.bigvgan, w, sp, bp, ord); break;
            }
            if (st || (st = ord.after_last(bp))) return st;
        }
        if ((st = ord.join())) return st;
        mean = sp.mean;
        if (mean == MEAN_KERNEL && (st = launch_mean_of_three(w.XB(0), w.XB(1), w.XB(2), w.Y, (long long)B * sp.ch * t, s))) return st;
        if (sp.dbg_here) {
            std::fprintf(stderr, "FV_DEBUG_STOP: stage %d ch=%d t=%d me=%lld S=%lld Y=%lld\n", i, sp.ch, t, (long long)w.me,
                         (long long)(w.S - ws), (long long)(w.Y - ws));
            return FV_OK;
        }
        std::swap(w.cur, w.Y);
    }
    return run_post(ups, w, mean == MEAN_IN_POST, d_out, B, t, s);
}

fv_status fv_engine::run_convnext(const float* d_in, float* d_out, int B, int T, float* ws, hipStream_t s) {
    const int64_t me = ((int64_t)cnx.max_dim() * T * B + 63) / 64 * 64;
    float* X = ws;               // running activation (dim, T)
    float* H = ws + me;          // LN output (dim, T)
    float* G = ws + 2 * me;      // hidden (4*dim, T)
    fv_status st;
    const int ks = cnx.cfg.kernel_size;
    ConvRun r;
    for (int i = 0; i < cnx.cfg.num_stages; ++i) {
        CnxStage& stg = *cnx.stages[i];
        const int dim = cnx.cfg.dims[i];
        if (i == 0) {
            r = ConvRun();
            r.batch = B;
            r.t_in = T;
            r.x = d_in;
            r.y = H;
            if ((st = conv_layer_run(stg.conv, r, s))) return st;
            FV_PROF(s, "layernorm_cf", 8.0 * B * dim * T, 8.0 * B * dim * T,
                    launch_dwconv_ln(H, nullptr, nullptr, stg.d_ln_w, stg.d_ln_b, X, B, dim, T, 1, 1e-6f, s));
        } else {
            FV_PROF(s, "layernorm_cf", 8.0 * B * stg.ln_dim * T, 8.0 * B * stg.ln_dim * T,
                    launch_dwconv_ln(X, nullptr, nullptr, stg.d_ln_w, stg.d_ln_b, H, B, stg.ln_dim, T, 1, 1e-6f, s));
            r = ConvRun();
            r.batch = B;
            r.t_in = T;
            r.x = H;
            r.y = X;
            if ((st = conv_layer_run(stg.conv, r, s))) return st;
        }
        for (auto& bp : stg.blocks) {
            CnxBlock& blk = *bp;
            // dwconv -> LN (convnext.py:126-129)
            FV_PROF(s, "dwconv_ln", (2.0 * ks + 8.0) * B * dim * T, 8.0 * B * dim * T,
                    launch_dwconv_ln(X, blk.d_dw_w, blk.d_dw_b, blk.d_ln_w, blk.d_ln_b, H, B, dim, T, ks, 1e-6f, s));
            // pwconv1 + GELU (convnext.py:130-131)
            r = ConvRun();
            r.batch = B;
            r.t_in = T;
            r.x = H;
            r.y = G;
            r.post_act = FV_ACT_GELU;
            if ((st = conv_layer_run(blk.pw1, r, s))) return st;
            // pwconv2, * gamma, + input (convnext.py:132-141)
            r = ConvRun();
            r.batch = B;
            r.t_in = T;
            r.x = G;
            r.y = X;
            r.res = X;
            r.gamma = blk.d_gamma;
            if ((st = conv_layer_run(blk.pw2, r, s))) return st;
        }
    }
    FV_PROF(s, "layernorm_cf", 8.0 * B * cnx.out_dim() * T, 8.0 * B * cnx.out_dim() * T,
            launch_dwconv_ln(X, nullptr, nullptr, cnx.d_norm_w, cnx.d_norm_b, d_out, B, cnx.out_dim(), T, 1, 1e-6f, s));
    return FV_OK;
}

fv_status fv_engine::run_head(const float* d_in, float* d_out, int B, int T, float* ws, hipStream_t s) {
    const int N = head.cfg.n_fft, nb = head.nb;
    const int64_t rows = std::max<int64_t>(2 * nb, N);
    const int64_t me = (rows * T * B + 63) / 64 * 64;
    float* Hh = ws;            // (2nb, T) log-mag / phase
    float* Sp = ws + me;       // (2nb, T) Re / Im
    float* Fr = ws + 2 * me;   // (n_fft, T) windowed frames
    fv_status st;
    ConvRun r;
    r.batch = B;
    r.t_in = T;
    r.x = d_in;
    r.y = Hh;
    if ((st = conv_layer_run(head.out, r, s))) return st;
    // Hh is already compacted to 2*nb rows: reuse the spec kernel with n_fft' = nb (rows [0,nb) mag, [nb,2nb) phase)
    FV_PROF(s, "istft_spec", 30.0 * B * nb * T, 16.0 * B * nb * T, launch_istft_spec(Hh, Sp, B, nb, T, nb, nb, s));
    r = ConvRun();
    r.batch = B;
    r.t_in = T;
    r.x = Sp;
    r.y = Fr;
    if ((st = conv_layer_run(head.idft, r, s))) return st;
    // "same": crop (win - hop) / 2 -> T * hop samples (vocos ISTFT); "center": crop n_fft / 2 -> (T - 1) * hop (torch.istft(center=True))
    FV_PROF(s, "istft_ola", 2.0 * B * N * T, 4.0 * B * (N * (double)T + (double)head.out_len(T)),
            launch_istft_ola(Fr, head.d_win2, d_out, B, N, T, head.cfg.hop_length, head.crop(), head.out_len(T), s));
    return FV_OK;
}

// The front-end's workspace for B rows of T frames: [Yp (B, hop, T + taps - 1) | Sp (B, 2 nb, T) | Mg (B, nb, T)], the first two rounded to 64 floats
fv_engine::LogmelParts fv_engine::logmel_carve(float* ws, int B, int T) const {
    const size_t n_yp = ((size_t)B * mel.cfg.hop_length * (T + mel.taps - 1) + 63) / 64 * 64, n_sp = ((size_t)B * 2 * mel.nb * T + 63) / 64 * 64;
    return {ws, ws + n_yp, ws + n_yp + n_sp};
}
size_t fv_engine::logmel_ws_elems(int B, int T) const {
    return ((size_t)B * cfg.mel.hop_length * ((size_t)T + mel.taps) + 64) + ((size_t)B * 3 * mel.nb * T + 128);
}

fv_status fv_engine::run_logmel(const float* d_in, float* d_out, int B, int L, float* ws, hipStream_t s) {
    const int hop = mel.cfg.hop_length;
    const int T = mel.frames(L);
    const int TP = T + mel.taps - 1;
    const LogmelParts p = logmel_carve(ws, B, T);
    FV_PROF(s, "polyphase_reflect", 0.0, 8.0 * B * (double)hop * TP,
            launch_polyphase_reflect(d_in, p.Yp, B, L, hop, TP, mel.pad_l, mel.pad_r, s));
    return run_logmel_tail(p, d_out, B, T, s);
}

// Everything behind the polyphase signal: STFT conv -> magnitude -> filterbank conv with log(clamp).  Shared by the whole forward, the
// ragged call and the stream (engine_logmel.hip): T frames out of Yp's T + taps - 1 slots
fv_status fv_engine::run_logmel_tail(const LogmelParts& p, float* d_out, int B, int T, hipStream_t s) {
    const int nb = mel.nb;
    fv_status st;
    ConvRun r;
    r.batch = B;
    r.t_in = T + mel.taps - 1;
    r.x = p.Yp;
    r.y = p.Sp;
    if ((st = conv_layer_run(mel.stft, r, s))) return st;
    if (mel.cfg.n_mels == 0) {   // LinearSpectrogram alone (spectrogram.py:25-56): the magnitude is the result
        FV_PROF(s, "magnitude", 4.0 * B * nb * T, 12.0 * B * nb * T, launch_magnitude(p.Sp, d_out, B, nb, T, s));
        return FV_OK;
    }
    FV_PROF(s, "magnitude", 4.0 * B * nb * T, 12.0 * B * nb * T, launch_magnitude(p.Sp, p.Mg, B, nb, T, s));
    r = ConvRun();
    r.batch = B;
    r.t_in = T;
    r.x = p.Mg;
    r.y = d_out;
    r.post_act = FV_ACT_LOG_CLAMP;   // compress(): log(clamp(x, 1e-5))  (spectrogram.py:93-94)
    return conv_layer_run(mel.mel, r, s);
}

fv_status fv_engine::run_model_whole(const float* d_in, float* d_out, int batch, int t_in, float* ws, hipStream_t s) {
    fv_engine* e = this;
    switch (e->cfg.model) {
        case FV_MODEL_HIFIGAN:
        case FV_MODEL_BIGVGAN: return e->run_upsampler(d_in, d_out, batch, t_in, ws, s);
        case FV_MODEL_CONVNEXT: return e->run_convnext(d_in, d_out, batch, t_in, ws, s);
        case FV_MODEL_ISTFT_HEAD: return e->run_head(d_in, d_out, batch, t_in, ws, s);
        case FV_MODEL_LOGMEL:
            if (e->mel.frames(t_in) < 1 || t_in <= std::max(e->mel.pad_l, e->mel.pad_r)) {
                set_error("logmel: %d samples is too short for reflect padding %d/%d and one %d-sample frame", t_in, e->mel.pad_l,
                          e->mel.pad_r, e->cfg.mel.n_fft);
                return FV_ERR_INVALID;
            }
            return e->run_logmel(d_in, d_out, batch, t_in, ws, s);
        case FV_MODEL_REFINEGAN: return e->run_refinegan(d_in, d_out, batch, t_in, ws, s);
        case FV_MODEL_VOCOS: {
            const size_t mid = align_up((size_t)e->cnx.out_dim() * t_in * batch, 64);
            fv_status st = e->run_convnext(d_in, ws, batch, t_in, ws + mid, s);
            if (st) return st;
            return e->run_head(ws, d_out, batch, t_in, ws + mid, s);
        }
        case FV_MODEL_FIREFLY: {
            const size_t mid = align_up((size_t)e->cnx.out_dim() * t_in * batch, 64);
            fv_status st = e->run_convnext(d_in, ws, batch, t_in, ws + mid, s);
            if (st) return st;
            return e->run_upsampler(ws, d_out, batch, t_in, ws + mid, s);
        }
    }
    set_error("fv_forward: unknown model");
    return FV_ERR_INVALID;
}

static size_t ups_ws_elems(const fv_engine* e, int B, int T) {
    return (size_t)(3 + 3 * e->ups.cfg.num_kernels) * ((e->ups.max_elems(T) * B + 63) / 64 * 64);
}
static size_t cnx_ws_elems(const fv_engine* e, int B, int T) {
    const size_t me = ((size_t)e->cnx.max_dim() * T * B + 63) / 64 * 64;
    return 2 * me + 4 * me;  // X, H, and the 4x hidden
}
static size_t head_ws_elems(const fv_engine* e, int B, int T) {
    const size_t rows = std::max<size_t>(2 * e->head.nb, e->cfg.head.n_fft);
    return 3 * ((rows * T * B + 63) / 64 * 64);
}

static size_t whole_workspace_bytes(const fv_engine* e, int32_t batch, int32_t t_in) {
    size_t elems = 0;
    switch (e->cfg.model) {
        case FV_MODEL_HIFIGAN:
        case FV_MODEL_BIGVGAN: elems = ups_ws_elems(e, batch, t_in); break;
        case FV_MODEL_CONVNEXT: elems = cnx_ws_elems(e, batch, t_in); break;
        case FV_MODEL_ISTFT_HEAD: elems = head_ws_elems(e, batch, t_in); break;
        case FV_MODEL_LOGMEL: {
            elems = e->logmel_ws_elems(batch, std::max(1, e->mel.frames(t_in)));
            break;
        }
        case FV_MODEL_REFINEGAN: elems = refine_ws_elems(e, batch, t_in); break;
        case FV_MODEL_VOCOS: {
            const size_t mid = align_up((size_t)e->cnx.out_dim() * t_in * batch, 64);
            elems = mid + std::max(cnx_ws_elems(e, batch, t_in), head_ws_elems(e, batch, t_in));
            break;
        }
        case FV_MODEL_FIREFLY: {
            const size_t mid = align_up((size_t)e->cnx.out_dim() * t_in * batch, 64);
            elems = mid + std::max(cnx_ws_elems(e, batch, t_in), ups_ws_elems(e, batch, t_in));
            break;
        }
    }
    return align_up(elems * sizeof(float), 256);
}

// A template where the generator takes one, and none where it does not (check_forward; fv_ragged_forward up front: a batch of empty clips
// runs no forward that would check it)
fv_status check_template(const fv_engine* e, const float* d_template) {
    if (e->wants_template() && !d_template) {
        set_error("fv_forward: this generator was built with use_template=True and needs a template (B, 1, T*hop)");
        return FV_ERR_INVALID;
    }
    if (!e->wants_template() && d_template) {
        set_error("fv_forward: template given but the generator was built with use_template=False");
        return FV_ERR_INVALID;
    }
    return FV_OK;
}

// What every entry that runs the model checks before it enqueues anything (forward_common; fv_ragged_forward for each of its groups)
fv_status check_forward(fv_engine* e, const float* d_in, const float* d_template, float* d_out, int32_t batch, int32_t t_in,
                        void* d_workspace, size_t workspace_bytes) {
    if (!e || !d_in || !d_out) {
        set_error("fv_forward: null argument");
        return FV_ERR_INVALID;
    }
    if (!e->finalized) {
        set_error("fv_forward: call fv_finalize first");
        return FV_ERR_STATE;
    }
    if (batch < 1 || t_in < 1) {
        set_error("fv_forward: empty input (batch=%d, t_in=%d)", batch, t_in);
        return FV_ERR_INVALID;
    }
    {
        const fv_engine::TilePlan tp = e->tile_plan(t_in);
        if (tp.n > 1 && (long long)batch * tp.n > (1 << 24)) {
            set_error("fv_forward: %d clips x %d time tiles of %d frames exceed 2^24 tiles per call: split the batch (or raise FV_TILE_FRAMES)", batch,
                      tp.n, tp.L);
            return FV_ERR_UNSUPPORTED;
        }
    }
    const size_t need = fv_workspace_bytes(e, batch, t_in);
    if (e->cfg.model == FV_MODEL_REFINEGAN && need == 0) {
        set_error("refinegan: the down/up-sampling lengths do not line up for %d frames (the reference's torch.cat would fail)", t_in);
        return FV_ERR_INVALID;
    }
    if (!d_workspace || workspace_bytes < need) {
        set_error("fv_forward: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
        return FV_ERR_INVALID;
    }
    if ((e->cfg.model == FV_MODEL_VOCOS || e->cfg.model == FV_MODEL_ISTFT_HEAD) && e->head.center()) {
        if (t_in < 2) {   // (T - 1) * hop = 0 samples: torch.istft fails on the empty envelope
            set_error("istft head, padding=\"center\": %d frame(s) leave no output samples ((T - 1) * hop)", t_in);
            return FV_ERR_INVALID;
        }
        if (!e->head.center_envelope_ok(t_in)) {
            set_error("istft head, padding=\"center\": window overlap add min < 1e-11 (torch.istft raises here too)");
            return FV_ERR_INVALID;
        }
    }
    return check_template(e, d_template);
}

fv_status forward_common(fv_engine* e, const float* d_in, const float* d_template, const float* d_noise, float* d_out,
                         int32_t batch, int32_t t_in, void* d_workspace, size_t workspace_bytes, void* stream, bool seeded,
                         int64_t origin_frame) {
    if (const fv_status st = check_forward(e, d_in, d_template, d_out, batch, t_in, d_workspace, workspace_bytes)) return st;
    const ForwardScope scope(e, d_template, d_noise, seeded, origin_frame);
    hipStream_t s = (hipStream_t)stream;
    float* ws = (float*)d_workspace;

    // hipGraph replay: a forward is ~110 launches plus fork/join events; at small batch the host launch cost dominates
    // (p50 clip latency).  The launch sequence is static for a given (pointers, batch, frames, stream), so the second
    // consecutive call with the same key is stream-captured (including the branch streams) and later calls replay it.
    // The legacy default stream (0: where the reference's own call runs, test.py:88-90) cannot be captured, but an instantiated graph can be launched on
    // it: the sequence is captured on an engine-owned stream and replayed on stream 0 — without the two cross-stream waits a redirect through a side
    // stream costs every call (single clip: ~0.04 ms of 0.75).
    fv_engine::GraphKey key{d_in, d_out, d_workspace, d_template, d_noise, batch, t_in, s, seeded, seeded ? e->noise_seed : 0,
                            seeded ? e->noise_first_row : 0, seeded ? origin_frame : 0};
    const bool graphable = e->opt.use_graph && !e->profiling;
    if (graphable) {
        for (auto& g : e->graphs)
            if (g.key == key) {
                FV_HIP_CHECK(hipGraphLaunch(g.exec, s));
                return FV_OK;
            }
        if (e->have_last && e->last_key == key) {
            hipStream_t cs = s;
            if (!cs) {
                if (!e->null_capture && hipStreamCreateWithFlags(&e->null_capture, hipStreamNonBlocking) != hipSuccess) {
                    (void)hipGetLastError();
                    e->null_capture = nullptr;
                }
                cs = e->null_capture;
            }
            hipError_t be = cs ? hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) : hipErrorInvalidValue;
            if (be == hipSuccess) {
                fv_status st = e->run_model(d_in, d_out, batch, t_in, ws, cs);
                hipGraph_t graph = nullptr;
                hipError_t ee = hipStreamEndCapture(cs, &graph);
                if (st == FV_OK && ee == hipSuccess && graph) {
                    hipGraphExec_t exec = nullptr;
                    if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) {
                        if (e->graphs.size() >= 8) {
                            (void)hipGraphExecDestroy(e->graphs.front().exec);
                            (void)hipGraphDestroy(e->graphs.front().graph);
                            e->graphs.erase(e->graphs.begin());
                        }
                        e->graphs.push_back({key, graph, exec});
                        FV_HIP_CHECK(hipGraphLaunch(exec, s));
                        return FV_OK;
                    }
                    (void)hipGraphDestroy(graph);
                } else if (graph) {
                    (void)hipGraphDestroy(graph);
                }
                (void)hipGetLastError();
                e->opt.use_graph = false;   // capture is not available in this context: stay eager from now on
                if (st) return st;
            } else {
                (void)hipGetLastError();
                e->opt.use_graph = false;
            }
        }
        e->last_key = key;
        e->have_last = true;
    }
    return e->run_model(d_in, d_out, batch, t_in, ws, s);
}

extern "C" {

FV_API size_t fv_workspace_bytes(const fv_engine* e, int32_t batch, int32_t t_in) {
    if (!e || !e->finalized || batch < 1 || t_in < 1) return 0;
    const fv_engine::TilePlan tp = e->tile_plan(t_in);
    if (tp.n <= 1) return whole_workspace_bytes(e, batch, t_in);
    if ((long long)batch * tp.n > (1 << 24)) return 0;
    return e->tile_workspace_bytes(batch, tp);
}

FV_API fv_status fv_forward(fv_engine* e, const float* d_in, float* d_out, int32_t batch, int32_t t_in, void* d_workspace,
                            size_t workspace_bytes, void* stream) {
    return fv_forward_template(e, d_in, nullptr, d_out, batch, t_in, d_workspace, workspace_bytes, stream);
}

FV_API fv_status fv_forward_template(fv_engine* e, const float* d_in, const float* d_template, float* d_out, int32_t batch,
                                     int32_t t_in, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (e && e->cfg.model == FV_MODEL_REFINEGAN) {
        set_error("fv_forward: a RefineGAN engine needs fv_forward_refinegan (template + AdaIN noise)");
        return FV_ERR_INVALID;
    }
    return forward_common(e, d_in, d_template, nullptr, d_out, batch, t_in, d_workspace, workspace_bytes, stream);
}

// ---- per-launch profile ----
FV_API fv_status fv_profile_begin(fv_engine* e) {
    if (!e) {
        set_error("fv_profile_begin: null engine");
        return FV_ERR_INVALID;
    }
    for (auto& r : e->prof.recs) {
        if (r.e0) (void)hipEventDestroy(r.e0);
        if (r.e1) (void)hipEventDestroy(r.e1);
    }
    e->prof.recs.clear();
    e->profiling = true;
    return FV_OK;
}

FV_API fv_status fv_profile_end(fv_engine* e, char* json_buf, size_t cap, size_t* needed) {
    if (!e) {
        set_error("fv_profile_end: null engine");
        return FV_ERR_INVALID;
    }
    e->profiling = false;
    struct Agg {
        int count = 0;
        double ms = 0, flops = 0, bytes = 0;
    };
    std::map<std::string, Agg> agg;
    std::vector<std::string> order;
    for (auto& r : e->prof.recs) {
        if (!r.e0 || !r.e1) continue;
        FV_HIP_CHECK(hipEventSynchronize(r.e1));
        float ms = 0.f;
        FV_HIP_CHECK(hipEventElapsedTime(&ms, r.e0, r.e1));
        if (!agg.count(r.label)) order.push_back(r.label);
        Agg& a = agg[r.label];
        a.count++;
        a.ms += ms;
        a.flops += r.flops;
        a.bytes += r.bytes;
    }
    std::string js = "[";
    for (size_t i = 0; i < order.size(); ++i) {
        const Agg& a = agg[order[i]];
        char buf[512];
        std::snprintf(buf, sizeof(buf),
                      "%s{\"kernel\": \"%s\", \"launches\": %d, \"total_ms\": %.6f, \"avg_ms\": %.6f, "
                      "\"flops_per_launch\": %.1f, \"bytes_per_launch\": %.1f}",
                      i ? ", " : "", order[i].c_str(), a.count, a.ms, a.ms / a.count, a.flops / a.count, a.bytes / a.count);
        js += buf;
    }
    js += "]";
    for (auto& r : e->prof.recs) {
        if (r.e0) (void)hipEventDestroy(r.e0);
        if (r.e1) (void)hipEventDestroy(r.e1);
    }
    e->prof.recs.clear();
    if (needed) *needed = js.size() + 1;
    if (json_buf && cap > 0) {
        const size_t n = std::min(cap - 1, js.size());
        std::memcpy(json_buf, js.data(), n);
        json_buf[n] = 0;
    }
    return FV_OK;
}

}  // extern "C"
