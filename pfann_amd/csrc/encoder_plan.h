// The launch plan of the encoder: every decision that picks a kernel variant, a grid or a scratch size for a
// pfann_encode chunk, as pure functions of the layer shapes, the batch, the plan batch, the precision, the taps mode and the
// PFANN_* environment switches.  The launchers (encoder_fused.hip, encoder.hip), encode_chunk_fused and the split-K scratch
// sizing (api.hip) execute what these functions return; pfann_encode_plan prints it (tests/test_encoder_plan.py holds the
// text against a kernel trace of the commit before the plan existed, profiles/encoder_plan/parent_launches.json).
// Host code only: no device, no context.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "common.h"

namespace pfann {

// the 16 sub-layer shapes of a model whose log-mel input is F x T; nullptr, or what is wrong with the config
static inline const char *plan_sublayers(const pfann_config &g, int F, int T, SubLayer *sub) {
    const int ch[9] = {1, g.d, g.d, 2 * g.d, 2 * g.d, 4 * g.d, 4 * g.d, g.h, g.h};
    for (int i = 0; i < 8; ++i) {
        const int st = g.stride_t[i] > 0 ? g.stride_t[i] : 2;
        const int sf = g.stride_f[i] > 0 ? g.stride_f[i] : 2;
        const int p1 = (T - 1) / st * st + 3 - T, p2 = (F - 1) / sf * sf + 3 - F;
        const int T1 = (T - 1) / st + 1, F2 = (F - 1) / sf + 1;
        SubLayer &a = sub[2 * i], &b = sub[2 * i + 1];
        a = SubLayer{};
        b = SubLayer{};
        a.ci = ch[i]; a.co = ch[i + 1]; a.F = F; a.T = T; a.Fo = F; a.To = T1;
        a.axis = 0; a.stride = st; a.pad_lo = p1 / 2; a.depthwise = 0;
        b.ci = ch[i + 1]; b.co = ch[i + 1]; b.F = F; b.T = T1; b.Fo = F2; b.To = T1;
        b.axis = 1; b.stride = sf; b.pad_lo = p2 / 2; b.depthwise = g.fuller ? 0 : 1;
        F = F2; T = T1;
    }
    if (F != 1 || T != 1) return "encoder output must be 1x1";
    if (g.d <= 0 || g.h % g.d != 0) return "h must be divisible by d";
    if (g.d % 4 != 0) return "d must be a multiple of 4";
    return nullptr;
}

// whether the LayerNorm-fused path (encoder_fused.hip) can run these layers
static inline bool plan_fused_supported(const SubLayer *sub, int n) {
    for (int i = 0; i < n; ++i) {
        const SubLayer &L = sub[i];
        const int rps = L.Fo * L.To;
        if (rps & (rps - 1)) return false;                  // power of two: tiles never straddle samples unevenly
        if (L.depthwise) { if (L.co % 4 || L.axis != 1) return false; continue; }     // conv_dw_ln_kernel
        if (L.ci == 1) { if (i != 0 || rps % 64 || L.co % 4) return false; }
        else if (L.ci % 4 || L.co % 4) return false;
    }
    return true;
}

// the K range [k_begin, k_end) of the taps that meet the input for at least one output position
static inline void live_taps(const SubLayer &L, int in_len, int &k_begin, int &k_end) {
    const int out_len = L.axis == 0 ? L.To : L.Fo;
    int lo = 3, hi = -1;
    for (int tap = 0; tap < 3; ++tap)
        for (int o = 0; o < out_len; ++o) {
            const int pos = o * L.stride - L.pad_lo + tap;
            if (pos >= 0 && pos < in_len) { lo = tap < lo ? tap : lo; hi = tap > hi ? tap : hi; break; }
        }
    k_begin = lo * L.ci;
    k_end = (hi + 1) * L.ci;
}

// tile size of the fused GEMM of sub-layer L under the plan for batch B
static inline int gemm_tile(const SubLayer &L, int64_t B) {
    const int64_t M = B * L.Fo * L.To;
    const int64_t blocks128 = (int64_t)cdiv(M, 128) * cdiv(L.co, 128);
    static const int64_t min128 = getenv("PFANN_TILE128_MIN") ? atoll(getenv("PFANN_TILE128_MIN")) : 512;
    return (L.co >= 128 && blocks128 >= min128 && L.ci % 32 == 0) ? 128 : 64;
}

// LayerNorm partial (sum, sum of squares) slots per sample that sub-layer L's producer writes under the plan for batch B
static inline int plan_out_slots(const SubLayer &L, int64_t B) {
    const int rps = L.Fo * L.To;
    if (L.ci == 1 || L.depthwise) return rps / 64 > 0 ? rps / 64 : 1;       // conv_first_stats / conv_dw_ln: 64 rows per block
    const int bt = gemm_tile(L, B);
    return (rps >= bt ? rps / bt : 1) * cdiv(L.co, bt);
}

// partial slots per sample the context allocates (pfann_create): every layer's count on 64-row tiles, the largest there is
static inline int64_t plan_part_slots(const SubLayer *sub) {
    int64_t slots = 0;
    for (int i = 0; i < 16; ++i) {
        const int rps = sub[i].Fo * sub[i].To;
        const int64_t n = (int64_t)(rps >= 64 ? rps / 64 : 1) * cdiv(sub[i].co, 64);
        if (n > slots) slots = n;
    }
    return slots;
}

static inline int splitk_chunk_kt() {
    static const int chunk_kt = getenv("PFANN_SPLITK_CHUNK") ? atoi(getenv("PFANN_SPLITK_CHUNK")) : 8;
    return chunk_kt;
}

// Split-K plan of sub-layer L (64x64 tiles only): number of K chunks, 0 = not split.  The cut is chunks of 8 K-tiles whatever
// the batch -- it depends on the layer only -- so a window's bits do not depend on how many windows share the launch;
// WHETHER a layer is split depends on the batch the plan is made for:
//   * plans of at most 64 windows (the one-query regime; pfann_set_plan_batch never pins one): launches of < 192 tiles;
//   * larger plans (round 6: the middle of the batch curve, 65 .. ~1000 windows): the layers whose launch at the PLAN's
//     batch is < 512 tiles of a chip that holds ~1000 -- the deep layers, M = B * (1 .. 8) rows with K loops of 48-96
//     K-tiles: at 76 windows `rows=2 K=3072` was 48 workgroups x 96 K-tiles, 71 us on a sixth of the chip.
static inline int splitk_plan(const SubLayer &L, int64_t B, int64_t Bp, bool first, int k_live) {
    const int chunk_kt = splitk_chunk_kt();
    static const bool no_splitk = getenv("PFANN_NO_SPLITK") != nullptr;
    static const int64_t mid_max = getenv("PFANN_SPLITK_MID_BLOCKS") ? atoll(getenv("PFANN_SPLITK_MID_BLOCKS")) : 512;
    if (no_splitk || first || chunk_kt <= 0 || L.ci % 32 != 0 || k_live % 32 != 0) return 0;
    const int nk = k_live / 32;
    const int n_splits = (nk + chunk_kt - 1) / chunk_kt;
    if (nk < 16 || n_splits <= 1) return 0;
    const int64_t rps = (int64_t)L.Fo * L.To, ntn = cdiv(L.co, 64);
    const int64_t blocks = (int64_t)cdiv(B * rps, 64) * ntn, blocks_p = (int64_t)cdiv(Bp * rps, 64) * ntn;
    const bool small = B <= 64 && Bp <= 64;
    if (small ? blocks >= 192 : (B > Bp || blocks_p >= mid_max)) return 0;
    return n_splits;
}

// A layer whose split-K partials for one stream's share of a call would pass this many bytes is not split: a rule of the layer
// and the share alone.  (Before the plan, such a layer was still split when the grow-only scratch happened to be large enough
// from an earlier call.)  A call on n streams can therefore hold up to n times this much scratch.
static const size_t SPLITK_LAYER_CAP = (size_t)256 << 20;

// ---- the fused conv GEMM of one sub-layer (launch_conv_gemm_ln) ------------------------------------------------------
struct ConvGemmPlan {
    int tile;               // 128 or 64 (rows = columns)
    bool w22;               // the five-block kernel (conv_gemm_ln_w22_kernel)
    bool split16;           // the 3-term fp16 split instantiation (precision 1)
    bool uni;               // C_in % 32 == 0: a K-tile holds one tap
    bool first;             // the C_in = 1 conv folded into the A-loader
    bool relu_bn;           // ReLU after LayerNorm: the <true, *> instantiations
    bool finalize;          // an ln_finalize launch precedes the GEMM
    int n_splits;           // > 1: split-K GEMM + splitk_reduce_ln (which leaves the OUTPUT's (mean, rstd)); else 0
    int k_begin, k_end, k_chunk;
    int out_P;              // partial slots per sample of the output
    int n_tiles_n;
    int64_t blocks;         // ceil(M / tile) * ceil(N / tile)
    int threads;
    size_t scratch;         // bytes of split-K partials, 0 when not split
};

// B: the samples of this launch (grid, scratch); Bsel: the samples of the whole call the launch is a stream's share of
// (0: B) -- the variant is chosen for the CALL, so the stream count never changes a kernel choice; Bp: the plan batch.
static inline ConvGemmPlan plan_conv_gemm_ln(const SubLayer &L, int64_t B, int64_t Bp, bool first, int precision, int act,
                                             int after_bn, bool in_final, int64_t Bsel = 0) {
    ConvGemmPlan q{};
    if (Bsel <= 0) Bsel = B;
    const int rps = L.Fo * L.To;
    const int64_t M = B * rps;
    const int N = L.co, in_len = L.axis == 0 ? L.T : L.F;
    live_taps(L, in_len, q.k_begin, q.k_end);
    q.first = first; q.relu_bn = act == 0 && after_bn; q.uni = L.ci % 32 == 0;
    q.finalize = !in_final;
    q.out_P = plan_out_slots(L, Bp);
    q.tile = gemm_tile(L, Bp);
    q.n_tiles_n = cdiv(N, q.tile);
    q.blocks = (int64_t)cdiv(M, q.tile) * q.n_tiles_n;
    if (q.tile == 128) {
        q.threads = 512;
        // five channel blocks per output pair instead of six (conv_gemm_ln_w22_kernel) where the layer allows it
        static const bool no_w22 = getenv("PFANN_NO_W22") != nullptr;
        const int out_len = L.axis == 0 ? L.To : L.Fo;
        q.w22 = !no_w22 && (!first || (L.axis == 1 && L.ci <= 256 && getenv("PFANN_NO_W22_FIRST") == nullptr)) && precision == 0 &&
                L.stride == 2 && L.pad_lo == 0 && q.k_begin == 0 && q.k_end == 3 * L.ci && out_len % 2 == 0 &&
                in_len >= 2 * out_len && M % 2 == 0 && N % 128 == 0 && (L.axis == 0 || (L.To <= 64 && 128 % (2 * L.To) == 0)) &&
                (int64_t)N * 4 * L.ci * 4 < 0x7FFF0000ll;
        q.split16 = !q.w22 && precision == 1 && q.relu_bn;
        return q;
    }
    q.threads = 256;
    // split-K for launches that cannot fill the chip and have a long K loop (splitk_plan above): chunks of 8 K-tiles
    // (measured on one 19-segment query: 12 -> 344 us, 8 -> 323, 6 -> 323, 4 -> 331 for the whole embed)
    const int n_splits = q.uni ? splitk_plan(L, Bsel, Bp, first, q.k_end - q.k_begin) : 0;
    const size_t bytes = (size_t)(n_splits > 0 ? n_splits : 0) * (size_t)M * N * sizeof(float);
    if (n_splits > 1 && bytes <= SPLITK_LAYER_CAP) {
        q.n_splits = n_splits;
        q.k_chunk = splitk_chunk_kt() * 32;
        q.scratch = bytes;
    }
    return q;
}

static inline std::string conv_gemm_kernel_name(const ConvGemmPlan &q) {
    char buf[160];
    const char *tf[2] = {"false", "true"};
    if (q.w22) snprintf(buf, sizeof buf, "conv_gemm_ln_w22_kernel<%s, %s>", tf[q.relu_bn], tf[q.first]);
    else if (q.tile == 128)
        snprintf(buf, sizeof buf, "conv_gemm_ln_kernel<128, 128, 64, 32, %s, %s, true, 32, %s, false>", tf[q.split16 || q.relu_bn],
                 tf[q.first], tf[q.split16]);
    else if (q.n_splits > 1)
        snprintf(buf, sizeof buf, "conv_gemm_ln_kernel<64, 64, 32, 32, %s, false, true, 32, false, true>", tf[q.relu_bn]);
    else
        snprintf(buf, sizeof buf, "conv_gemm_ln_kernel<64, 64, 32, 32, %s, %s, %s, 32, false, false>", tf[q.relu_bn], tf[q.first],
                 tf[q.uni]);
    return buf;
}

// ---- the projection head (launch_myg_ln) -------------------------------------------------------------------------------
struct HeadPlan {
    bool small;             // myg_ln_small_kernel: one workgroup per segment, weights through LDS
    int seg, vmax;          // myg_ln_kernel<seg, vmax> otherwise
    int threads;
    size_t lds;
    int64_t grid;
};

static inline HeadPlan plan_myg_ln(int d, int u, int v, int64_t B, int64_t Bplan) {
    HeadPlan h{};
    const int nt = ((d + 63) / 64) * 64;
    static const bool no_small = getenv("PFANN_NO_SMALL_HEAD") != nullptr;
    const size_t small_lds = ((size_t)d * v + (size_t)d * u) * sizeof(float);
    if (B <= 64 && (Bplan <= 0 || Bplan <= 64) && !no_small && small_lds <= 60 * 1024) {
        int thr = d * u < 1024 ? ((d * u + 63) / 64) * 64 : 1024;
        if (thr < nt) thr = nt;
        h.small = true; h.threads = thr; h.lds = small_lds; h.grid = B;
        return h;
    }
    h.threads = nt;
    if (v <= 8) { h.seg = 4; h.vmax = 8; h.grid = cdiv(B, 4); }
    else { h.seg = 1; h.vmax = 32; h.grid = B; }
    return h;
}

// ---- the unfused path (encoder.hip) ----------------------------------------------------------------------------------
// tile of conv_gemm_kernel: big tiles when the grid still fills 256 CUs a few times over
static inline int plain_gemm_tile(const SubLayer &L, int64_t B) {
    const int64_t blocks128 = (int64_t)cdiv(B * L.Fo * L.To, 128) * cdiv(L.co, 128);
    return (L.co >= 128 && blocks128 >= 512) ? 128 : 64;
}
static inline int ln_act_threads(const SubLayer &L) { return L.co * L.Fo * L.To >= 65536 ? 1024 : 256; }

// ---- one chunk (encode_chunk1: one stream's share of a pfann_encode call of at most max_batch samples) ------------------
// taps: 0 none; 1 every sub-layer's activation materialised, the first conv not folded (pfann_debug_keep);
//       2 the activations materialised beside the production plan (pfann_debug_keep_at): sub-layers 1..15, and sub-layer 0
//         where that plan does not fold the first conv.
static inline bool plan_fold_first(const SubLayer *sub, int taps) {
    return taps != 1 && sub[1].axis == 1 && sub[0].co <= 256 && getenv("PFANN_NO_FOLD_FIRST") == nullptr;
}

// bytes of split-K scratch a fused chunk of B samples uses: its largest split layer
static inline size_t plan_chunk_scratch(const SubLayer *sub, int64_t B, int64_t Bp, int taps, int64_t Bsel = 0) {
    const bool fold_first = plan_fold_first(sub, taps);
    size_t need = 0;
    for (int i = 1; i < 16; ++i) {
        if (sub[i].depthwise) continue;
        const ConvGemmPlan q = plan_conv_gemm_ln(sub[i], B, Bp, fold_first && i == 1, 0, 0, 1, false, Bsel);
        if (q.scratch > need) need = q.scratch;
    }
    return need;
}

// how a call of B samples (at most max_batch) is spread over the internal streams: the chunk sizes, in order
static inline std::vector<int64_t> plan_stream_chunks(int64_t B, int n_streams) {
    const int64_t by_size = B / 128;
    const int ns = (int)(by_size < n_streams ? by_size : n_streams);
    std::vector<int64_t> out;
    if (ns <= 1) { out.push_back(B); return out; }
    for (int k = 0; k < ns; ++k) out.push_back(B / ns + (k < B % ns ? 1 : 0));
    return out;
}

struct PlannedLaunch {
    std::string name;
    int64_t grid;
    int block;
    size_t lds;
    int layer;              // sub-layer index, -1: the head
    int tile, n_splits, first, out_P;       // conv layers of the fused path (tile 0 otherwise)
};

static inline void plan_chunk_launches(const pfann_config &g, const SubLayer *sub, int64_t B, int64_t Bp, int precision,
                                       bool fused, int taps, std::vector<PlannedLaunch> &out, int64_t Bsel = 0) {
    auto add = [&](const std::string &name, int64_t grid, int block, size_t lds, int layer) {
        out.push_back(PlannedLaunch{name, grid, block, lds, layer, 0, 0, 0, 0});
    };
    const int64_t nb_tap = B < 8 ? B : 8;
    if (!fused) {
        for (int i = 0; i < 16; ++i) {
            const SubLayer &L = sub[i];
            const int64_t M = B * L.Fo * L.To;
            if (L.ci == 1 && !L.depthwise) add("conv_first_kernel", cdiv(M * (L.co / 4), 256), 256, 0, i);
            else if (L.depthwise) add("conv_dw_kernel", cdiv(M * (L.co / 4), 256), 256, 0, i);
            else if (plain_gemm_tile(L, Bsel > 0 ? Bsel : B) == 128) add("conv_gemm_kernel<128, 128, 64, 64>", (int64_t)cdiv(M, 128) * cdiv(L.co, 128), 256, 0, i);
            else add("conv_gemm_kernel<64, 64, 32, 32>", (int64_t)cdiv(M, 64) * cdiv(L.co, 64), 256, 0, i);
            if (L.ci != 1 && !L.depthwise) out.back().tile = plain_gemm_tile(L, Bsel > 0 ? Bsel : B);
            const int nt = ln_act_threads(L);
            add(nt == 1024 ? "ln_act_kernel<1024>" : "ln_act_kernel<256>", B, nt, 0, i);
        }
        add("myg_kernel", B, ((g.d + 63) / 64) * 64, 0, -1);
        return;
    }
    const bool fold_first = plan_fold_first(sub, taps);
    const int64_t M0 = B * sub[0].Fo * sub[0].To;
    if (fold_first && g.relu_after_bn) add("conv_first_gram_stats_kernel", cdiv(M0, 256), 256, 0, 0);
    else add("conv_first_stats_kernel", cdiv(M0, 64), 256, 0, 0);
    out.back().first = fold_first; out.back().out_P = plan_out_slots(sub[0], Bp);
    if (taps == 1 || (taps == 2 && !fold_first)) add("ln_apply_kernel", nb_tap, 256, 0, 0);     // tap 0 wherever it is materialised
    bool stats_final = false;
    for (int i = 1; i < 16; ++i) {
        const SubLayer &L = sub[i];
        const bool first = fold_first && i == 1;
        if (L.depthwise) {
            stats_final = false;
            add("ln_finalize_kernel", cdiv(B, 4), 256, 0, i);
            const int P = plan_out_slots(L, B);
            add(first ? "conv_dw_ln_kernel<true>" : "conv_dw_ln_kernel<false>", B * P, 256, 0, i);
            out.back().first = first; out.back().out_P = P;
        } else {
            const ConvGemmPlan q = plan_conv_gemm_ln(L, B, Bp, first, precision, g.activation, g.relu_after_bn, stats_final, Bsel);
            if (q.finalize) add("ln_finalize_kernel", cdiv(B, 4), 256, 0, i);
            add(conv_gemm_kernel_name(q), q.blocks * (q.n_splits > 1 ? q.n_splits : 1), q.threads, 0, i);
            PlannedLaunch &pl = out.back();
            pl.tile = q.tile; pl.n_splits = q.n_splits; pl.first = first; pl.out_P = q.out_P;
            if (q.n_splits > 1) add("splitk_reduce_ln_kernel", B, 1024, 0, i);
            stats_final = q.n_splits > 1;
        }
        if (taps != 0) add("ln_apply_kernel", nb_tap, 256, 0, i);
    }
    const HeadPlan h = plan_myg_ln(g.d, g.u, g.h / g.d, B, Bp);        // (a stream's share is >= 128 samples: never the small head)
    char buf[64];
    if (h.small) snprintf(buf, sizeof buf, "myg_ln_small_kernel");
    else snprintf(buf, sizeof buf, "myg_ln_kernel<%d, %d>", h.seg, h.vmax);
    add(buf, h.grid, h.threads, h.lds, -1);
}

}  // namespace pfann
