// C-ABI of libpfann_amd.so (include/pfann_amd.h): handles, weight re-layout, workspaces,
// per-kernel HIP-event profiling and the reference's native seam (version / seq_score).
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>

#include "kernels.h"
#include "search_plan.h"

namespace pfann { int launch_rows_to_half(const float *x, int64_t n, int d, void *xh, float *norm_max_dev, hipStream_t s); }

__global__ void noop_api_kernel() {}
static int launch_noop_api() {
    hipLaunchKernelGGL(noop_api_kernel, dim3(1), dim3(1), 0, 0);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

namespace pfann {

static thread_local char g_err[1024] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- profiling ------------------------------------------------------------------------
struct ProfRec { std::string tag; hipEvent_t e0, e1; double work; };
static bool g_prof = false;
static std::vector<ProfRec> g_recs;
static std::vector<hipEvent_t> g_pool;
static hipEvent_t g_pending = nullptr;
bool prof_on() { return g_prof; }
static hipEvent_t get_event() {
    if (!g_pool.empty()) { hipEvent_t e = g_pool.back(); g_pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
void prof_begin(const char *, hipStream_t s) {
    g_pending = get_event();
    (void)hipEventRecord(g_pending, s);
}
void prof_end(const char *tag, hipStream_t s, double work) {
    hipEvent_t e1 = get_event();
    (void)hipEventRecord(e1, s);
    g_recs.push_back({tag, g_pending, e1, work});
    g_pending = nullptr;
}

}  // namespace pfann

using namespace pfann;

// =========================================================================================
// encoder context
// =========================================================================================
struct pfann_ctx {
    pfann_config cfg;
    int device;
    MelPlan mel;
    bool mel_ready = false;
    int F, T;                       // encoder input dims (n_mels, n_frames)
    SubLayer sub[16];
    float *g_w1 = nullptr, *g_b1 = nullptr, *g_w2 = nullptr, *g_b2 = nullptr;
    std::map<std::string, bool> loaded;
    int n_expected = 0;
    float *buf[2] = {nullptr, nullptr};
    int64_t buf_elems[2] = {0, 0};  // per sample
    float *mel_buf = nullptr;
    double *scratch = nullptr;
    std::vector<float> w1_host, b1_host;   // first conv [3][co] / [co] (Gram-form LayerNorm statistics)
    float gram[14] = {};
    bool gram_ready = false;
    bool fused = false;             // LayerNorm fused into the GEMMs (encoder_fused.hip)
    int precision = 0;              // 0: fp32 MFMA (exact); 1: 3-term fp16 split on the fp16 MFMA (opt-in)
    int64_t plan_batch = 0;         // pfann_set_plan_batch: kernel variants chosen for this batch size (0: each call's own)
    int n_streams = 1;              // sub-batches run on this many internal streams (MFMA-bound GEMMs of one
                                    // sub-batch overlap the HBM-bound LayerNorm passes of another)
    hipStream_t side[8] = {};
    hipEvent_t ev_fork = nullptr, ev_join[8] = {};
    float *part[2] = {nullptr, nullptr};
    float *splitk = nullptr;        // partial tiles of the split-K GEMMs (small batches), allocated on first use
    size_t splitk_bytes = 0;
    float *stats = nullptr;         // [max_batch][2] (mean, rstd) of the current GEMM input
    int64_t part_slots = 0;         // per sample
    int keep = 0;                   // verification taps (pfann_debug_keep_at): 0 off, 1 every sub-layer with the first conv
                                    // materialised, 2 sub-layers 1..15 beside the production plan
    int64_t keep_first = 0;         // first of the (up to) 8 consecutive samples of a chunk whose taps are kept
    int64_t keep_B = 0;
    float *dbg[16] = {};
    bool dbg_has[16] = {};          // tap written by the last call
    float *dbg_tmp = nullptr;
    int64_t dbg_cap = 0;
};

extern "C" int pfann_set_streams(pfann_ctx *c, int n);

static int build_plan(pfann_ctx *c) {
    const char *why = plan_sublayers(c->cfg, c->F, c->T, c->sub);       // csrc/encoder_plan.h
    if (why) { set_error("%s", why); return -1; }
    return 0;
}

static int upload(float **dst, const float *src, size_t n) {
    if (*dst == nullptr) PF_HIP(hipMalloc(dst, n * sizeof(float)));
    PF_HIP(hipMemcpy(*dst, src, n * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

__global__ void pfann_bench_region_marker() {}

extern "C" {

long long version(void) { return PFANN_SEQSCORE_VERSION; }

const char *pfann_last_error(void) { return g_err; }

pfann_ctx *pfann_create(const pfann_config *cfg, int device) {
    if (hipSetDevice(device) != hipSuccess) { set_error("hipSetDevice(%d) failed: no usable GPU", device); return nullptr; }
    pfann_ctx *c = new pfann_ctx();
    c->cfg = *cfg;
    c->device = device;
    if (c->cfg.max_batch <= 0) c->cfg.max_batch = 512;
    const int n_fft = cfg->stft_n;
    int log2n = 0;
    while ((1 << log2n) < n_fft) ++log2n;
    if ((1 << log2n) != n_fft || n_fft < 64 || n_fft > 4096) { set_error("stft_n must be a power of two in 64..4096"); delete c; return nullptr; }
    if (cfg->n_mels % 1 != 0 || cfg->n_mels <= 0) { set_error("bad n_mels"); delete c; return nullptr; }
    MelPlan &m = c->mel;
    memset(&m, 0, sizeof(m));
    m.seg_len = cfg->segment_len; m.n_fft = n_fft; m.hop = cfg->stft_hop; m.n_mels = cfg->n_mels;
    m.n_frames = 1 + cfg->segment_len / cfg->stft_hop;
    m.n_freqs = n_fft / 2 + 1; m.log2n = log2n;
    m.power = cfg->power; m.pad_reflect = cfg->pad_reflect; m.log_mode = cfg->log_mode;
    m.spec_norm_max = cfg->spec_norm_max; m.log_eps = cfg->log_eps;
    if (m.pad_reflect && n_fft / 2 >= cfg->segment_len) { set_error("reflect padding needs stft_n/2 < segment_len"); delete c; return nullptr; }
    // periodic hann window and twiddles, computed in double on the host
    std::vector<float> win(n_fft);
    std::vector<float2> tw(n_fft / 2);
    for (int n = 0; n < n_fft; ++n) win[n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * n / n_fft));
    for (int j = 0; j < n_fft / 2; ++j) {
        tw[j].x = (float)cos(-2.0 * M_PI * j / n_fft);
        tw[j].y = (float)sin(-2.0 * M_PI * j / n_fft);
    }
    if (hipMalloc(&m.window, n_fft * sizeof(float)) != hipSuccess ||
        hipMalloc(&m.twiddle, (n_fft / 2) * sizeof(float2)) != hipSuccess) { set_error("hipMalloc failed"); delete c; return nullptr; }
    (void)hipMemcpy(m.window, win.data(), n_fft * sizeof(float), hipMemcpyHostToDevice);
    (void)hipMemcpy(m.twiddle, tw.data(), (n_fft / 2) * sizeof(float2), hipMemcpyHostToDevice);
    c->F = cfg->n_mels;
    c->T = m.n_frames;
    if (build_plan(c)) { delete c; return nullptr; }
    c->n_expected = 8 * 8 + 4;
    // workspaces: ping-pong activation buffers (even sub-layers -> buf[0], odd -> buf[1])
    for (int i = 0; i < 16; ++i) {
        const int64_t e = (int64_t)c->sub[i].co * c->sub[i].Fo * c->sub[i].To;
        c->buf_elems[i & 1] = std::max(c->buf_elems[i & 1], e);
    }
    c->fused = fused_supported(c->sub, 16) && getenv("PFANN_NO_FUSE") == nullptr;
    if (!c->fused && cfg->fuller && getenv("PFANN_NO_FUSE") == nullptr)
        fprintf(stderr, "pfann_amd: this model's layer shapes (an Fo*To that is not a power of two, or channel counts not "
                        "multiples of 4) are outside the LayerNorm-fused GEMM path; using the separate-LayerNorm kernels\n");
    if (getenv("PFANN_STREAMS")) pfann_set_streams(c, atoi(getenv("PFANN_STREAMS")));
    c->part_slots = plan_part_slots(c->sub);         // csrc/encoder_plan.h
    if (hipMalloc(&c->scratch, 16 * sizeof(double)) != hipSuccess) {
        set_error("hipMalloc failed");
        delete c;
        return nullptr;
    }
    return c;
}

void pfann_destroy(pfann_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (int i = 0; i < 16; ++i) {
        if (c->sub[i].w) (void)hipFree(c->sub[i].w);
        if (c->sub[i].w_hi) { (void)hipFree(c->sub[i].w_hi); (void)hipFree(c->sub[i].w_lo); }
        if (c->sub[i].w22) (void)hipFree(c->sub[i].w22);
        if (c->sub[i].bias) (void)hipFree(c->sub[i].bias);
        if (c->sub[i].ln_w) (void)hipFree(c->sub[i].ln_w);
        if (c->sub[i].ln_b) (void)hipFree(c->sub[i].ln_b);
        if (c->dbg[i]) (void)hipFree(c->dbg[i]);
    }
    float *ptrs[] = {c->g_w1, c->g_b1, c->g_w2, c->g_b2, c->buf[0], c->buf[1], c->part[0], c->part[1], c->splitk, c->stats, c->mel_buf, c->mel.window,
                     c->mel.fb_val, c->dbg_tmp};
    for (float *p : ptrs) if (p) (void)hipFree(p);
    if (c->mel.twiddle) (void)hipFree(c->mel.twiddle);
    if (c->mel.fb_ptr) (void)hipFree(c->mel.fb_ptr);
    if (c->mel.fb_idx) (void)hipFree(c->mel.fb_idx);
    if (c->scratch) (void)hipFree(c->scratch);
    delete c;
}

int pfann_set_melbank(pfann_ctx *c, const float *fb, int n_freqs, int n_mels) {
    if (n_freqs != c->mel.n_freqs || n_mels != c->mel.n_mels) {
        set_error("melbank shape [%d,%d] != [%d,%d]", n_freqs, n_mels, c->mel.n_freqs, c->mel.n_mels);
        return -3;
    }
    PF_HIP(hipSetDevice(c->device));
    std::vector<int> ptr(n_mels + 1, 0), idx;
    std::vector<float> val;
    int mx = 0;
    for (int m = 0; m < n_mels; ++m) {
        for (int k = 0; k < n_freqs; ++k) {
            const float v = fb[(size_t)k * n_mels + m];
            if (v != 0.0f) { idx.push_back(k); val.push_back(v); }
        }
        ptr[m + 1] = (int)idx.size();
        mx = std::max(mx, ptr[m + 1] - ptr[m]);
    }
    if (idx.empty()) { idx.push_back(0); val.push_back(0.f); }
    MelPlan &mp = c->mel;
    if (mp.fb_ptr) { (void)hipFree(mp.fb_ptr); (void)hipFree(mp.fb_idx); (void)hipFree(mp.fb_val); }
    PF_HIP(hipMalloc(&mp.fb_ptr, ptr.size() * sizeof(int)));
    PF_HIP(hipMalloc(&mp.fb_idx, idx.size() * sizeof(int)));
    PF_HIP(hipMalloc(&mp.fb_val, val.size() * sizeof(float)));
    PF_HIP(hipMemcpy(mp.fb_ptr, ptr.data(), ptr.size() * sizeof(int), hipMemcpyHostToDevice));
    PF_HIP(hipMemcpy(mp.fb_idx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice));
    PF_HIP(hipMemcpy(mp.fb_val, val.data(), val.size() * sizeof(float), hipMemcpyHostToDevice));
    mp.max_nnz_row = mx;
    mp.fb_nnz = (int)idx.size();
    c->mel_ready = true;
    return 0;
}

int pfann_load_weight(pfann_ctx *c, const char *name, const float *host, int64_t numel) {
    PF_HIP(hipSetDevice(c->device));
    const pfann_config &g = c->cfg;
    int blk = -1;
    char mod[16] = "", kind[16] = "";
    if (sscanf(name, "f.convs.%d.%15[a-z0-9].%15s", &blk, mod, kind) == 3 && blk >= 0 && blk < 8) {
        const bool second = mod[strlen(mod) - 1] == '2';
        SubLayer &L = c->sub[2 * blk + (second ? 1 : 0)];
        const bool is_w = strcmp(kind, "weight") == 0;
        if (!is_w && strcmp(kind, "bias") != 0) { set_error("unknown tensor %s", name); return -2; }
        if (strncmp(mod, "conv", 4) == 0) {
            if (!is_w) {
                if (numel != L.co) { set_error("%s: numel %lld != %d", name, (long long)numel, L.co); return -3; }
                if (upload(&L.bias, host, numel)) return -1;
                if (blk == 0 && !second) { c->b1_host.assign(host, host + numel); c->gram_ready = false; }
            } else {
                const int ci = L.depthwise ? 1 : L.ci;
                if (numel != (int64_t)L.co * ci * 3) { set_error("%s: numel %lld != %lld", name, (long long)numel, (long long)L.co * ci * 3); return -3; }
                std::vector<float> w((size_t)numel);
                if (ci == 1) {          // [co][1][3] -> [3][co]
                    for (int o = 0; o < L.co; ++o)
                        for (int t = 0; t < 3; ++t) w[(size_t)t * L.co + o] = host[(size_t)o * 3 + t];
                } else {                // [co][ci][3] -> [co][3][ci]
                    for (int o = 0; o < L.co; ++o)
                        for (int i = 0; i < ci; ++i)
                            for (int t = 0; t < 3; ++t)
                                w[((size_t)o * 3 + t) * ci + i] = host[((size_t)o * ci + i) * 3 + t];
                }
                if (upload(&L.w, w.data(), numel)) return -1;
                if (blk == 0 && !second) { c->w1_host = w; c->gram_ready = false; }
                if (ci > 1) {
                    // {W1, W0, -W2, W0 + W2} per output channel for the five-block kernel (encoder_fused.hip)
                    std::vector<float> w4((size_t)L.co * 4 * ci);
                    for (int o = 0; o < L.co; ++o)
                        for (int i = 0; i < ci; ++i) {
                            const float w0 = w[((size_t)o * 3 + 0) * ci + i], w1 = w[((size_t)o * 3 + 1) * ci + i],
                                        w2 = w[((size_t)o * 3 + 2) * ci + i];
                            float *d4 = &w4[(size_t)o * 4 * ci + i];
                            d4[0] = w1; d4[ci] = w0; d4[2 * (size_t)ci] = -w2; d4[3 * (size_t)ci] = w0 + w2;
                        }
                    if (upload(&L.w22, w4.data(), (int64_t)w4.size())) return -1;
                }
                if (ci > 1) {
                    // 2-term fp16 split of w * 2^e (largest magnitude in [2^14, 2^15)): hi = fl16(ws),
                    // lo = fl16(ws - hi) exactly representable residual -> 2^-22 relative, both in the normal range
                    float mx = 0.f;
                    for (float v : w) mx = std::max(mx, std::fabs(v));
                    int e = 0;
                    if (mx > 0.f) { (void)std::frexp(mx, &e); e = 15 - e; }      // mx * 2^e in [2^14, 2^15)
                    const float sc = std::ldexp(1.0f, e);
                    std::vector<_Float16> hi((size_t)numel), lo((size_t)numel);
                    for (size_t i = 0; i < (size_t)numel; ++i) {
                        const float ws = w[i] * sc;
                        hi[i] = (_Float16)ws;
                        lo[i] = (_Float16)(ws - (float)hi[i]);
                    }
                    if (!L.w_hi) { PF_HIP(hipMalloc(&L.w_hi, numel * 2)); PF_HIP(hipMalloc(&L.w_lo, numel * 2)); }
                    PF_HIP(hipMemcpy(L.w_hi, hi.data(), numel * 2, hipMemcpyHostToDevice));
                    PF_HIP(hipMemcpy(L.w_lo, lo.data(), numel * 2, hipMemcpyHostToDevice));
                    L.w_inv_scale = std::ldexp(1.0f, -e);
                }
            }
        } else if (strncmp(mod, "ln", 2) == 0) {
            const int64_t hw = (int64_t)L.Fo * L.To;
            if (numel != L.co * hw) { set_error("%s: numel %lld != %lld", name, (long long)numel, (long long)(L.co * hw)); return -3; }
            std::vector<float> w((size_t)numel);   // [co][Fo][To] -> [Fo][To][co]
            for (int o = 0; o < L.co; ++o)
                for (int64_t p = 0; p < hw; ++p) w[(size_t)p * L.co + o] = host[(size_t)o * hw + p];
            if (upload(is_w ? &L.ln_w : &L.ln_b, w.data(), numel)) return -1;
        } else {
            set_error("unknown tensor %s", name);
            return -2;
        }
    } else if (strncmp(name, "g.linear", 8) == 0) {
        const int v = g.h / g.d;
        float **dst = nullptr;
        int64_t want = 0;
        if (!strcmp(name, "g.linear1.weight")) { dst = &c->g_w1; want = (int64_t)g.d * g.u * v; }
        else if (!strcmp(name, "g.linear1.bias")) { dst = &c->g_b1; want = (int64_t)g.d * g.u; }
        else if (!strcmp(name, "g.linear2.weight")) { dst = &c->g_w2; want = (int64_t)g.d * g.u; }
        else if (!strcmp(name, "g.linear2.bias")) { dst = &c->g_b2; want = g.d; }
        else { set_error("unknown tensor %s", name); return -2; }
        if (numel != want) { set_error("%s: numel %lld != %lld", name, (long long)numel, (long long)want); return -3; }
        if (upload(dst, host, numel)) return -1;
    } else {
        set_error("unknown tensor %s", name);
        return -2;
    }
    c->loaded[name] = true;
    return 0;
}

int pfann_weights_missing(pfann_ctx *c) { return c->n_expected - (int)c->loaded.size(); }

int pfann_melspec(pfann_ctx *c, const float *segs, int64_t B, int64_t seg_stride, int remove_mean, float *out,
                  void *stream) {
    PF_HIP(hipSetDevice(c->device));
    if (!c->mel_ready) { set_error("pfann_melspec: mel filterbank not set"); return -5; }
    return launch_melspec(c->mel, segs, B, seg_stride, nullptr, remove_mean, out, (hipStream_t)stream);
}

int pfann_melspec_plan(pfann_ctx *c, int64_t B, int out[4]) {
    if (!c->mel_ready) { set_error("pfann_melspec_plan: mel filterbank not set"); return -5; }
    const MelLaunch ml = plan_melspec(c->mel, B);
    out[0] = ml.group_out; out[1] = ml.parts; out[2] = (int)ml.lds_bytes; out[3] = ml.radix8;
    return 0;
}

// the kept samples of a chunk of B: up to 8 from keep_first, clamped to the chunk
static int64_t keep_window(const pfann_ctx *c, int64_t B, int64_t *first) {
    const int64_t nb = std::min<int64_t>(B, 8);
    *first = std::max<int64_t>(0, std::min<int64_t>(c->keep_first, B - nb));
    return nb;
}

static int keep_tap(pfann_ctx *c, int idx, const float *act, int64_t B, hipStream_t s) {
    const SubLayer &L = c->sub[idx];
    const int64_t e = (int64_t)L.co * L.Fo * L.To;
    int64_t b0;
    const int64_t nb = keep_window(c, B, &b0);
    if (!c->dbg[idx]) PF_HIP(hipMalloc(&c->dbg[idx], 8 * e * sizeof(float)));
    PF_HIP(hipMemcpyAsync(c->dbg[idx], act + b0 * e, nb * e * sizeof(float), hipMemcpyDeviceToDevice, s));
    c->keep_B = nb;
    c->dbg_has[idx] = true;
    return 0;
}

// activation / mel workspaces are allocated on first use (a mel-only context stays small)
static int ensure_workspace(pfann_ctx *c, bool need_mel) {
    const int64_t mb = c->cfg.max_batch;
    if (!c->buf[0]) {
        // the activation workspace: max_batch x the two largest sub-layer outputs (29 GB at 9728 segments of the default
        // model -- sized for a 288 GB MI355X; a device that cannot give it gets told which knob to turn)
        const size_t need = (size_t)mb * (c->buf_elems[0] + c->buf_elems[1]) * sizeof(float);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b < need) {
            set_error("the encoder workspace for max_batch = %lld segments needs %.1f GB but only %.1f GB of device memory are "
                      "free: lower max_batch (the tools: PFANN_MAX_BATCH)", (long long)mb, need / 1e9, free_b / 1e9);
            return -1;
        }
        PF_HIP(hipMalloc(&c->buf[0], mb * c->buf_elems[0] * sizeof(float)));
        PF_HIP(hipMalloc(&c->buf[1], mb * c->buf_elems[1] * sizeof(float)));
        PF_HIP(hipMalloc(&c->part[0], mb * c->part_slots * 2 * sizeof(float)));
        PF_HIP(hipMalloc(&c->part[1], mb * c->part_slots * 2 * sizeof(float)));
        PF_HIP(hipMalloc(&c->stats, mb * 2 * sizeof(float)));
    }
    if (need_mel && !c->mel_buf) PF_HIP(hipMalloc(&c->mel_buf, mb * (int64_t)c->F * c->T * sizeof(float)));
    return 0;
}

static int keep_tap_fused(pfann_ctx *c, int idx, const float *z, const float *part, int P, int64_t B, hipStream_t s) {
    const SubLayer &L = c->sub[idx];
    const int64_t e = (int64_t)L.co * L.Fo * L.To;
    int64_t b0;
    const int64_t nb = keep_window(c, B, &b0);
    if (!c->dbg[idx]) PF_HIP(hipMalloc(&c->dbg[idx], 8 * e * sizeof(float)));
    c->keep_B = nb;
    c->dbg_has[idx] = true;
    return launch_ln_apply(L, z + b0 * e, part + b0 * P * 2, P, c->dbg[idx], nb, c->cfg.activation, c->cfg.relu_after_bn, s);
}

// Gram form of the first conv's LayerNorm statistics (see conv_first_gram_stats_kernel), in fp64
static void build_gram(pfann_ctx *c) {
    const int co = c->sub[0].co;
    const std::vector<float> &w = c->w1_host, &b = c->b1_host;      // w: [3][co]
    double Bsum = 0, Ws[3] = {0, 0, 0}, bb = 0, h[3] = {0, 0, 0}, G[3][3] = {};
    for (int o = 0; o < co; ++o) {
        Bsum += b[o];
        bb += (double)b[o] * b[o];
        for (int t = 0; t < 3; ++t) {
            Ws[t] += w[t * co + o];
            h[t] += (double)b[o] * w[t * co + o];
            for (int u = 0; u < 3; ++u) G[t][u] += (double)w[t * co + o] * w[u * co + o];
        }
    }
    const double v[14] = {Bsum, Ws[0], Ws[1], Ws[2], bb, h[0], h[1], h[2], G[0][0], G[0][1], G[0][2], G[1][1], G[1][2], G[2][2]};
    for (int i = 0; i < 14; ++i) c->gram[i] = (float)v[i];
    c->gram_ready = true;
}

// sk / sk_bytes: this chunk's slice of the split-K scratch, plan_chunk_scratch bytes of it (encode_chunk)
static int encode_chunk_fused(pfann_ctx *c, const float *mel, int64_t B, float *emb, int normalize, hipStream_t s,
                              int64_t slot0, float *sk, size_t sk_bytes, int64_t Bcall) {
    const pfann_config &g = c->cfg;
    float *buf[2] = {c->buf[0] + slot0 * c->buf_elems[0], c->buf[1] + slot0 * c->buf_elems[1]};
    float *part[2] = {c->part[0] + slot0 * c->part_slots * 2, c->part[1] + slot0 * c->part_slots * 2};
    // Sub-layer 0 (C_in = 1 conv): normally only its LayerNorm statistics are computed here and the
    // conv itself is folded into sub-layer 1's A-loader; the 2 MiB/segment tensor is materialised
    // only when verification taps are requested.
    const bool fold_first = plan_fold_first(c->sub, c->keep);         // csrc/encoder_plan.h
    const int64_t Bp = c->plan_batch > 0 ? c->plan_batch : Bcall;     // the variants are those of the whole call
    for (int i = 0; i < 16; ++i) c->dbg_has[i] = false;
    if (fold_first && g.relu_after_bn && (int)c->w1_host.size() == 3 * c->sub[0].co && (int)c->b1_host.size() == c->sub[0].co) {
        if (!c->gram_ready) build_gram(c);
        if (launch_conv_first_gram_stats(c->sub[0], mel, part[0], B, c->gram, s)) return -1;
    } else if (launch_conv_first_stats(c->sub[0], mel, fold_first ? nullptr : buf[0], part[0], B, g.activation, g.relu_after_bn, s)) {
        return -1;
    }
    int P = fused_out_slots(c->sub[0], Bp);
    if ((c->keep == 1 || (c->keep == 2 && !fold_first)) && keep_tap_fused(c, 0, buf[0], part[0], P, B, s)) return -1;
    int stats_final = 0;             // c->stats already holds (mean, rstd) of the next layer's input (split-K reduction)
    for (int i = 1; i < 16; ++i) {
        const bool first = fold_first && i == 1;
        if (c->sub[i].depthwise) {
            stats_final = 0;
            if (launch_conv_dw_ln(c->sub[i], c->sub[i - 1], first ? mel : buf[(i - 1) & 1], part[(i - 1) & 1], P, c->stats + slot0 * 2,
                                  buf[i & 1], part[i & 1], B, g.activation, g.relu_after_bn, first ? &c->sub[0] : nullptr, s)) return -1;
        } else if (launch_conv_gemm_ln(c->sub[i], c->sub[i - 1], first ? mel : buf[(i - 1) & 1], part[(i - 1) & 1], P, c->stats + slot0 * 2, buf[i & 1],
                                part[i & 1], B, g.activation, g.relu_after_bn, first ? &c->sub[0] : nullptr, c->precision, s,
                                sk, sk_bytes, &stats_final, Bp, Bcall)) return -1;
        P = fused_out_slots(c->sub[i], Bp);
        if (c->keep && keep_tap_fused(c, i, buf[i & 1], part[i & 1], P, B, s)) return -1;
    }
    return launch_myg_ln(c->sub[15], buf[1], part[1], P, g.activation, g.relu_after_bn, c->g_w1, c->g_b1,
                         c->g_w2, c->g_b2, g.d, g.u, g.h / g.d, B, emb, normalize, s, Bp);
}

static int encode_chunk1(pfann_ctx *c, const float *mel, int64_t B, float *emb, int normalize, hipStream_t s,
                         int64_t slot0, float *sk, size_t sk_bytes, int64_t Bcall) {
    if (c->fused) return encode_chunk_fused(c, mel, B, emb, normalize, s, slot0, sk, sk_bytes, Bcall);
    for (int i = 0; i < 16; ++i) c->dbg_has[i] = false;
    const float *x = mel;
    for (int i = 0; i < 16; ++i) {
        const SubLayer &L = c->sub[i];
        float *y = c->buf[i & 1] + slot0 * c->buf_elems[i & 1];
        int rc;
        if (L.ci == 1 && !L.depthwise) rc = launch_conv_first(L, x, y, B, s);
        else if (L.depthwise) rc = launch_conv_depthwise(L, x, y, B, s);
        else rc = launch_conv_gemm(L, x, y, B, s, Bcall);
        if (rc) return rc;
        if (launch_ln_act(L, y, B, c->cfg.activation, c->cfg.relu_after_bn, s)) return -1;
        if (c->keep && keep_tap(c, i, y, B, s)) return -1;
        x = y;
    }
    const pfann_config &g = c->cfg;
    return launch_myg(x, c->g_w1, c->g_b1, c->g_w2, c->g_b2, g.d, g.u, g.h / g.d, B, emb, normalize, s);
}

// Splits a chunk over the internal streams: fork after the caller's stream, join back into it.
static int encode_chunk(pfann_ctx *c, const float *mel, int64_t B, float *emb, int normalize, hipStream_t s) {
    // The stream count never changes a kernel choice: every stream's chunk runs the kernel variants the whole call would run
    // on one stream (split-K layers included) on its own slice of the scratch -- [n_splits][rows][N] partials of the chunk's
    // largest split layer (one query: ~5 MB, 304 windows: ~30 MB; a layer whose partials would pass 256 MB is not split).
    const std::vector<int64_t> chunks = plan_stream_chunks(B, c->n_streams);        // csrc/encoder_plan.h
    const int ns = (int)chunks.size();
    size_t sk_off[9] = {0};
    for (int k = 0; k < ns; ++k) {
        const size_t need = c->fused ? plan_chunk_scratch(c->sub, chunks[k], c->plan_batch > 0 ? c->plan_batch : B, c->keep, B) : 0;
        sk_off[k + 1] = sk_off[k] + (need + 255) / 256 * 256;
    }
    if (sk_off[ns] > c->splitk_bytes) {          // grow-only
        if (c->splitk) { PF_HIP(hipStreamSynchronize(s)); (void)hipFree(c->splitk); }
        c->splitk = nullptr; c->splitk_bytes = 0;
        PF_HIP(hipMalloc(&c->splitk, sk_off[ns]));
        c->splitk_bytes = sk_off[ns];
    }
    auto slice = [&](int k) { return c->splitk ? c->splitk + sk_off[k] / sizeof(float) : nullptr; };
    if (ns <= 1) return encode_chunk1(c, mel, B, emb, normalize, s, 0, slice(0), sk_off[1] - sk_off[0], B);
    if (!c->ev_fork) {
        PF_HIP(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        for (int k = 0; k < 8; ++k) {
            PF_HIP(hipStreamCreateWithFlags(&c->side[k], hipStreamNonBlocking));
            PF_HIP(hipEventCreateWithFlags(&c->ev_join[k], hipEventDisableTiming));
        }
    }
    PF_HIP(hipEventRecord(c->ev_fork, s));
    const int64_t per = (int64_t)c->F * c->T;
    int64_t b0 = 0;
    for (int k = 0; k < ns; ++k) {
        const int64_t nb = chunks[k];
        PF_HIP(hipStreamWaitEvent(c->side[k], c->ev_fork, 0));
        if (encode_chunk1(c, mel + b0 * per, nb, emb + b0 * c->cfg.d, normalize, c->side[k], b0, slice(k), sk_off[k + 1] - sk_off[k], B)) return -1;
        PF_HIP(hipEventRecord(c->ev_join[k], c->side[k]));
        PF_HIP(hipStreamWaitEvent(s, c->ev_join[k], 0));
        b0 += nb;
    }
    return 0;
}

int pfann_encode(pfann_ctx *c, const float *mel, int64_t B, float *emb, int normalize, void *stream) {
    PF_HIP(hipSetDevice(c->device));
    if (pfann_weights_missing(c) != 0) { set_error("pfann_encode: %d state_dict tensors not loaded", pfann_weights_missing(c)); return -5; }
    hipStream_t s = (hipStream_t)stream;
    if (ensure_workspace(c, false)) return -1;
    const int64_t per = (int64_t)c->F * c->T;
    for (int64_t b0 = 0; b0 < B; b0 += c->cfg.max_batch) {
        const int64_t nb = std::min<int64_t>(c->cfg.max_batch, B - b0);
        if (encode_chunk(c, mel + b0 * per, nb, emb + b0 * c->cfg.d, normalize, s)) return -1;
    }
    return 0;
}

static int segment_embed_impl(pfann_ctx *c, const float *wav, int64_t B, int64_t seg_stride, const int64_t *starts,
                              float *emb, int normalize, void *stream) {
    PF_HIP(hipSetDevice(c->device));
    if (!c->mel_ready) { set_error("pfann_segment_embed: mel filterbank not set"); return -5; }
    if (pfann_weights_missing(c) != 0) { set_error("pfann_segment_embed: %d state_dict tensors not loaded", pfann_weights_missing(c)); return -5; }
    hipStream_t s = (hipStream_t)stream;
    if (ensure_workspace(c, true)) return -1;
    for (int64_t b0 = 0; b0 < B; b0 += c->cfg.max_batch) {
        const int64_t nb = std::min<int64_t>(c->cfg.max_batch, B - b0);
        const float *src = starts ? wav : wav + b0 * seg_stride;
        if (launch_melspec(c->mel, src, nb, seg_stride, starts ? starts + b0 : nullptr, 1, c->mel_buf, s)) return -1;
        if (encode_chunk(c, c->mel_buf, nb, emb + b0 * c->cfg.d, normalize, s)) return -1;
    }
    return 0;
}

int pfann_segment_embed(pfann_ctx *c, const float *wav, int64_t B, int64_t seg_stride, float *emb, int normalize,
                        void *stream) {
    return segment_embed_impl(c, wav, B, seg_stride, nullptr, emb, normalize, stream);
}

int pfann_segment_embed_at(pfann_ctx *c, const float *wav, const int64_t *starts_dev, int64_t B, float *emb,
                           int normalize, void *stream) {
    return segment_embed_impl(c, wav, B, 0, starts_dev, emb, normalize, stream);
}

int pfann_resample_to_mono(pfann_ctx *c, const int16_t *pcm, int n_ch, const float *kernels, int old_rate, int new_rate, int width,
                           const int64_t *plan, int n_pieces, int64_t n_out, float *tmp, float *wav, void *stream) {
    PF_HIP(hipSetDevice(c->device));
    return launch_resample_to_mono(pcm, n_ch, kernels, old_rate, new_rate, width, plan, n_pieces, n_out, tmp, wav,
                                   reinterpret_cast<float *>(c->scratch), (hipStream_t)stream);
}

int pfann_pcm16_to_mono(pfann_ctx *c, const int16_t *pcm, int64_t n_frames, int n_ch, float *wav, void *stream) {
    PF_HIP(hipSetDevice(c->device));
    if (n_ch < 1) { set_error("n_ch < 1"); return -1; }
    return launch_pcm16_to_mono(pcm, n_frames, n_ch, wav, reinterpret_cast<float *>(c->scratch), (hipStream_t)stream);
}

int pfann_pcm16_files_to_mono(pfann_ctx *c, const void *const *host_pcm, const int64_t *n_samples, const int64_t *dst_off,
                              int n_files, int16_t *pcm_dev, int64_t total, float *wav_dev, void *stream) {
    PF_HIP(hipSetDevice(c->device));
    for (int i = 0; i < n_files; ++i) {
        if (n_samples[i] <= 0) continue;
        if (dst_off[i] < 0 || dst_off[i] + n_samples[i] > total) { set_error("pcm16_files_to_mono: file %d outside the slab", i); return -1; }
        PF_HIP(hipMemcpyAsync(pcm_dev + dst_off[i], host_pcm[i], (size_t)n_samples[i] * sizeof(int16_t), hipMemcpyHostToDevice,
                              (hipStream_t)stream));
    }
    if (total <= 0) return 0;
    return launch_pcm16_to_mono(pcm_dev, total, 1, wav_dev, reinterpret_cast<float *>(c->scratch), (hipStream_t)stream);
}

void pfann_debug_keep(pfann_ctx *c, int on) { (void)pfann_debug_keep_at(c, on != 0 ? 1 : 0, 0); }

int pfann_debug_keep_at(pfann_ctx *c, int mode, int64_t first_sample) {
    if (mode < 0 || mode > 2 || first_sample < 0) { set_error("pfann_debug_keep_at: mode %d, first_sample %lld", mode, (long long)first_sample); return -1; }
    c->keep = mode;
    c->keep_first = first_sample;
    return mode;
}

int pfann_prewarm(int device) {
    if (hipSetDevice(device) != hipSuccess) { set_error("pfann_prewarm: no HIP device %d", device); return -1; }
    int rc = launch_noop_api();
    rc |= prewarm_mel() | prewarm_encoder() | prewarm_encoder_fused() | prewarm_search() | prewarm_search_f16() | prewarm_rerank() | prewarm_monitor() | prewarm_dense() | prewarm_dense_songs() | prewarm_dbstore();
    if (hipDeviceSynchronize() != hipSuccess) rc = -1;
    return rc ? -1 : 0;
}

int64_t pfann_set_plan_batch(pfann_ctx *c, int64_t n) {
    c->plan_batch = n <= 0 ? 0 : (n < 65 ? 65 : n);      // a plan below 65 would select the small-batch kernels, whose
    return c->plan_batch;                                // scratch is sized for actual batches of at most 64
}

int pfann_set_streams(pfann_ctx *c, int n) {
    c->n_streams = n < 1 ? 1 : (n > 8 ? 8 : n);
    return c->n_streams;
}

int pfann_set_encoder_precision(pfann_ctx *c, int mode) {
    c->precision = (mode == 1 && c->fused) ? 1 : 0;
    return c->precision;
}

int pfann_set_fused_layernorm(pfann_ctx *c, int on) {
    if (on && !fused_supported(c->sub, 16)) return 0;
    c->fused = on != 0;
    return c->fused ? 1 : 0;
}

int64_t pfann_debug_activation(pfann_ctx *c, int idx, int64_t B, float *host, int64_t cap) {
    if (idx < 0 || idx > 15 || !c->dbg[idx] || !c->dbg_has[idx]) {
        if (idx == 0 && c->keep == 2 && c->fused)
            set_error("tap 0 is absent in taps mode 2: this model's plan folds the first conv into sub-layer 1's loader and never "
                      "materialises it (taps 1..15 are kept; mode 1 keeps tap 0)");
        else set_error("no tap %d (call pfann_debug_keep(ctx,1) before encoding)", idx);
        return -1;
    }
    if (hipSetDevice(c->device) != hipSuccess) return -1;
    const SubLayer &L = c->sub[idx];
    const int64_t e = (int64_t)L.co * L.Fo * L.To;
    B = std::min(B, c->keep_B);
    if (B * e > cap) { set_error("tap buffer too small"); return -1; }
    if (c->dbg_cap < B * e) {
        if (c->dbg_tmp) (void)hipFree(c->dbg_tmp);
        if (hipMalloc(&c->dbg_tmp, B * e * sizeof(float)) != hipSuccess) return -1;
        c->dbg_cap = B * e;
    }
    if (launch_cl_to_nchw(c->dbg[idx], c->dbg_tmp, B, L.co, L.Fo * L.To, 0)) return -1;
    if (hipMemcpy(host, c->dbg_tmp, B * e * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return B * e;
}

}  // extern "C"

// =========================================================================================
// database shard
// =========================================================================================
struct pfann_db {
    int d, device;
    int64_t n = 0, label_base = 0;
    float *emb = nullptr;
    int64_t *song_pos = nullptr;
    std::vector<int64_t> song_pos_h;
    int n_songs = 0, song_lo = 0, song_hi = 0;
    SearchWorkspace ws;
    void *emb_h = nullptr;              // fp16 rows: a copy for the batched scan's pre-filter (fp32 storage), or the
                                        // ONLY rows kept (fp16 storage)
    int storage = PFANN_DB_F32;
    float xnorm_max = 0.f;
    bool prefilter = true;
    void *match_scratch = nullptr;      // long-query candidate slab (keys + sums), grown on demand
    size_t match_scratch_bytes = 0;
    void *win_scratch = nullptr;        // pfann_match_windows, general path: (qstart, qlen) of the expanded windows
    size_t win_scratch_bytes = 0;
    void *dense_ws = nullptr;           // pfann_match_windows_dense_topn: per-song words of one chunk of windows, grown on demand
    size_t dense_ws_bytes = 0;
    int64_t max_song_rows = 0;          // longest song (pfann_db_load)
    // updates (pfann_db_reserve / _append / _remove_songs).  Invariant: n == 0 <=> emb == emb_h == nullptr and cap == 0 (what
    // a fresh load of no rows leaves), so a reservation on an empty handle is only noted and honoured by the first append
    int64_t cap = 0;                    // rows emb / emb_h can hold
    int song_cap = 0;                   // songs the device song_pos can hold (song_cap + 1 entries)
    int64_t want_rows = 0;
    int want_songs = 0;
    bool norms = false;                 // xnorm_max is kept (fp16 storage, or fp32 storage with the fp16 copy asked for at load)
    std::vector<float> song_norm;       // [n_songs] largest row norm of every song (0: no rows, or norms not kept)
    // the seq_score seam (the reference's ctypes call, database.py:178-189): device slab, PINNED host image and a
    // private stream, kept between calls; seq_mu serialises concurrent callers on one handle (the reference's seam is
    // re-entrant: cpp/seqscore.cpp keeps no state)
    void *seq_scratch = nullptr;
    size_t seq_scratch_bytes = 0;
    char *seq_host = nullptr;
    size_t seq_host_bytes = 0;
    hipStream_t seq_stream = nullptr;
    std::mutex seq_mu;
};

extern "C" {

pfann_db *pfann_db_create(int d, int device) {
    if (hipSetDevice(device) != hipSuccess) { set_error("hipSetDevice(%d) failed: no usable GPU", device); return nullptr; }
    pfann_db *db = new pfann_db();
    db->d = d;
    db->device = device;
    return db;
}

void pfann_db_destroy(pfann_db *db) {
    if (!db) return;
    (void)hipSetDevice(db->device);
    (void)hipDeviceSynchronize();
    if (db->emb) (void)hipFree(db->emb);
    if (db->song_pos) (void)hipFree(db->song_pos);
    if (db->ws.thr) { (void)hipFree(db->ws.thr); (void)hipFree(db->ws.cnt); (void)hipFree(db->ws.cl); }
    if (db->ws.overflow) (void)hipFree(db->ws.overflow);
    if (db->ws.thr_adj) { (void)hipFree(db->ws.thr_adj); (void)hipFree(db->ws.eps); }
    if (db->ws.qh) (void)hipFree(db->ws.qh);
    if (db->ws.row_ovf) (void)hipFree(db->ws.row_ovf);
    if (db->ws.left) (void)hipFree(db->ws.left);
    if (db->ws.excl) (void)hipFree(db->ws.excl);        // (excl_tile lies in the same allocation)
    if (db->match_scratch) (void)hipFree(db->match_scratch);
    if (db->win_scratch) (void)hipFree(db->win_scratch);
    if (db->dense_ws) (void)hipFree(db->dense_ws);
    if (db->seq_scratch) (void)hipFree(db->seq_scratch);
    if (db->seq_host) (void)hipHostFree(db->seq_host);
    if (db->seq_stream) (void)hipStreamDestroy(db->seq_stream);
    if (db->emb_h) (void)hipFree(db->emb_h);
    delete db;
}

int pfann_db_set_prefilter(pfann_db *db, int on) {
    db->prefilter = on != 0;
    return (db->prefilter && db->emb_h != nullptr) ? 1 : 0;
}
int pfann_db_set_storage(pfann_db *db, int mode) {
    if (mode != PFANN_DB_F32 && mode != PFANN_DB_F16) { set_error("pfann_db_set_storage: unknown mode %d", mode); return -1; }
    if (db->n != 0 && mode != db->storage) { set_error("pfann_db_set_storage: call it before pfann_db_load"); return -1; }
    if (mode == PFANN_DB_F16 && db->d % 8 != 0) { set_error("pfann_db_set_storage: fp16 rows need d %% 8 == 0 (d=%d)", db->d); return -1; }
    db->storage = mode;
    return mode;
}
int pfann_db_dim(pfann_db *db) { return db->d; }
int64_t pfann_db_ntotal(pfann_db *db) { return db->n; }
int64_t pfann_db_bytes(pfann_db *db) { return db->n * db->d * (int64_t)(db->storage == PFANN_DB_F16 ? 2 : 4); }

int pfann_db_load(pfann_db *db, const float *emb, int emb_is_device, int64_t n, const int64_t *song_pos,
                  int n_songs, int64_t label_base) {
    PF_HIP(hipSetDevice(db->device));
    if (db->emb) { (void)hipFree(db->emb); db->emb = nullptr; }
    if (db->song_pos) { (void)hipFree(db->song_pos); db->song_pos = nullptr; }
    if (db->emb_h) { (void)hipFree(db->emb_h); db->emb_h = nullptr; }
    db->n = 0;
    db->cap = 0;
    db->label_base = label_base;
    db->n_songs = n_songs;
    db->xnorm_max = 0.f;
    db->norms = false;
    db->song_norm.assign((size_t)std::max(n_songs, 0), 0.f);
    PF_HIP(hipMalloc(&db->song_pos, (size_t)(n_songs + 1) * sizeof(int64_t)));
    PF_HIP(hipMemcpy(db->song_pos, song_pos, (size_t)(n_songs + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    db->song_cap = n_songs;
    // per-song maxima of the row norms, for the updates: beside the conversion below, which they do not change
    float *song_max = nullptr;
    const bool keep_norms = n > 0 && n_songs > 0 &&
                            (db->storage == PFANN_DB_F16 || (db->d % 8 == 0 && getenv("PFANN_NO_F16_PREFILTER") == nullptr));
    if (keep_norms) {
        PF_HIP(hipMalloc(&song_max, (size_t)n_songs * sizeof(float)));
        PF_HIP(hipMemset(song_max, 0, (size_t)n_songs * sizeof(float)));
    }
    if (n > 0 && db->storage == PFANN_DB_F16) {
        // fp16-only storage: the fp32 rows pass through a bounded staging buffer and are never kept
        float *nm = nullptr, *stage = nullptr;
        const int64_t chunk = std::max<int64_t>(1, (64ll << 20) / ((int64_t)db->d * 4));
        PF_HIP(hipMalloc(&db->emb_h, (size_t)n * db->d * 2));
        PF_HIP(hipMalloc(&nm, sizeof(float)));
        PF_HIP(hipMemset(nm, 0, sizeof(float)));
        if (!emb_is_device) PF_HIP(hipMalloc(&stage, (size_t)std::min(chunk, n) * db->d * sizeof(float)));
        for (int64_t r0 = 0; r0 < n; r0 += chunk) {
            const int64_t nr = std::min(chunk, n - r0);
            const float *src = emb + r0 * db->d;
            if (!emb_is_device) {
                PF_HIP(hipMemcpy(stage, src, (size_t)nr * db->d * sizeof(float), hipMemcpyHostToDevice));
                src = stage;
            }
            if (launch_rows_to_half(src, nr, db->d, reinterpret_cast<char *>(db->emb_h) + (size_t)r0 * db->d * 2, nm, 0)) return -1;
            if (song_max && launch_song_norm_max(src, nr, db->d, label_base + r0, db->song_pos, n_songs, 0, song_max, 0)) return -1;
            PF_HIP(hipDeviceSynchronize());
        }
        PF_HIP(hipMemcpy(&db->xnorm_max, nm, sizeof(float), hipMemcpyDeviceToHost));
        (void)hipFree(nm);
        if (stage) (void)hipFree(stage);
        if (!(db->xnorm_max < 6.0e4f)) {
            (void)hipFree(db->emb_h);
            db->emb_h = nullptr;
            if (song_max) (void)hipFree(song_max);
            set_error("db_load: rows with norm %g do not fit fp16 storage", (double)db->xnorm_max);
            return -3;
        }
    } else if (n > 0) {
        PF_HIP(hipMalloc(&db->emb, (size_t)n * db->d * sizeof(float)));
        PF_HIP(hipMemcpy(db->emb, emb, (size_t)n * db->d * sizeof(float),
                         emb_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        // fp16 copy + largest row norm for the batched scan's pre-filter (search_f16.hip)
        if (db->d % 8 == 0 && getenv("PFANN_NO_F16_PREFILTER") == nullptr) {
            float *nm = nullptr;
            PF_HIP(hipMalloc(&db->emb_h, (size_t)n * db->d * 2));
            PF_HIP(hipMalloc(&nm, sizeof(float)));
            PF_HIP(hipMemset(nm, 0, sizeof(float)));
            if (launch_rows_to_half(db->emb, n, db->d, db->emb_h, nm, 0)) return -1;
            if (song_max && launch_song_norm_max(db->emb, n, db->d, label_base, db->song_pos, n_songs, 0, song_max, 0)) return -1;
            PF_HIP(hipMemcpy(&db->xnorm_max, nm, sizeof(float), hipMemcpyDeviceToHost));
            (void)hipFree(nm);
            if (!(db->xnorm_max < 1.0e4f)) {       // fp16 range / NaN guard: keep the exact-fp32 scan only
                (void)hipFree(db->emb_h);
                db->emb_h = nullptr;
            }
        }
    }
    if (song_max) {
        PF_HIP(hipMemcpy(db->song_norm.data(), song_max, (size_t)n_songs * sizeof(float), hipMemcpyDeviceToHost));
        (void)hipFree(song_max);
        db->norms = true;
    }
    db->n = n;
    db->cap = n;
    db->song_pos_h.assign(song_pos, song_pos + n_songs + 1);
    db->max_song_rows = 0;
    for (int i = 0; i < n_songs; ++i) db->max_song_rows = std::max(db->max_song_rows, song_pos[i + 1] - song_pos[i]);
    // songs whose rows all live in [label_base, label_base + n)
    int lo = 0;
    while (lo < n_songs && song_pos[lo] < label_base) ++lo;
    int hi = lo;
    while (hi < n_songs && song_pos[hi + 1] <= label_base + n) ++hi;
    db->song_lo = lo;
    db->song_hi = hi;
    if (n > 0 && (lo >= n_songs || song_pos[lo] != label_base || song_pos[hi] != label_base + n)) {
        set_error("db_load: shard rows [%lld,%lld) do not align with song boundaries", (long long)label_base,
                  (long long)(label_base + n));
        return -3;
    }
    return 0;
}

// ---- updates of a loaded handle (include/pfann_amd.h: "Database updates"; kernels in dbstore.hip) -----------------------
}  // extern "C"

// maximum of two non-negative floats by bit pattern, as the kernels' atomicMax takes it (a NaN wins)
static float norm_max2(float a, float b) {
    unsigned ua, ub;
    memcpy(&ua, &a, 4);
    memcpy(&ub, &b, 4);
    return ua >= ub ? a : b;
}

static bool db_is_shard(const pfann_db *db) {
    return db->label_base != 0 || db->song_lo != 0 || db->song_hi != db->n_songs ||
           (!db->song_pos_h.empty() && db->song_pos_h.back() != db->n) || (db->song_pos_h.empty() && db->n != 0);
}

// device allocations of one update call: whatever was not handed over to the handle is freed when the call returns
struct DbTemps {
    std::vector<void *> p;
    ~DbTemps() { for (void *q : p) if (q) (void)hipFree(q); }
    template <typename T> hipError_t get(T **out, size_t bytes) {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, std::max<size_t>(bytes, 16));
        if (e == hipSuccess) p.push_back(q);
        *out = reinterpret_cast<T *>(q);
        return e;
    }
    void keep(void *q) { for (void *&x : p) if (x == q) x = nullptr; }
};

extern "C" {

int64_t pfann_db_capacity(pfann_db *db) { return db->cap; }
float pfann_db_row_norm_max(pfann_db *db) { return db->xnorm_max; }

int pfann_db_reserve(pfann_db *db, int64_t rows, int songs) {
    PF_HIP(hipSetDevice(db->device));
    PF_HIP(hipDeviceSynchronize());
    if (rows < 0 || songs < 0) { set_error("db_reserve: rows=%lld songs=%d", (long long)rows, songs); return -1; }
    DbTemps tmp;
    float *emb = nullptr;
    char *emb_h = nullptr;
    int64_t *sp = nullptr;
    const bool grow_rows = db->n > 0 && rows > db->cap, grow_songs = db->song_pos != nullptr && songs > db->song_cap;
    // everything new first: a failed allocation leaves the handle as it was
    if (grow_rows && db->emb) PF_HIP(tmp.get(&emb, (size_t)rows * db->d * sizeof(float)));
    if (grow_rows && db->emb_h) PF_HIP(tmp.get(&emb_h, (size_t)rows * db->d * 2));
    if (grow_songs) PF_HIP(tmp.get(&sp, (size_t)(songs + 1) * sizeof(int64_t)));
    if (emb) PF_HIP(hipMemcpy(emb, db->emb, (size_t)db->n * db->d * sizeof(float), hipMemcpyDeviceToDevice));
    if (emb_h) PF_HIP(hipMemcpy(emb_h, db->emb_h, (size_t)db->n * db->d * 2, hipMemcpyDeviceToDevice));
    if (sp) PF_HIP(hipMemcpy(sp, db->song_pos_h.data(), db->song_pos_h.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    PF_HIP(hipDeviceSynchronize());
    if (emb) { (void)hipFree(db->emb); db->emb = emb; tmp.keep(emb); }
    if (emb_h) { (void)hipFree(db->emb_h); db->emb_h = emb_h; tmp.keep(emb_h); }
    if (grow_rows) db->cap = rows;
    if (sp) { (void)hipFree(db->song_pos); db->song_pos = sp; db->song_cap = songs; tmp.keep(sp); }
    db->want_rows = std::max(db->want_rows, rows);
    db->want_songs = std::max(db->want_songs, songs);
    return 0;
}

int pfann_db_append(pfann_db *db, const float *emb, int emb_is_device, int64_t n_rows, const int32_t *song_rows_host,
                    int n_new_songs) {
    PF_HIP(hipSetDevice(db->device));
    PF_HIP(hipDeviceSynchronize());
    // ---- validate before touching anything
    if (n_rows < 0 || n_new_songs < 0 || (n_rows > 0 && emb == nullptr) || (n_new_songs > 0 && song_rows_host == nullptr)) {
        set_error("db_append: n_rows=%lld n_new_songs=%d", (long long)n_rows, n_new_songs);
        return -1;
    }
    if (db_is_shard(db)) {
        set_error("db_append: the handle holds a shard of the database (monitor mode is not song-sharded)");
        return -1;
    }
    int64_t sum = 0;
    for (int i = 0; i < n_new_songs; ++i) {
        if (song_rows_host[i] < 0) { set_error("db_append: song %d has %d rows", i, song_rows_host[i]); return -1; }
        sum += song_rows_host[i];
    }
    if (sum != n_rows) { set_error("db_append: the songs have %lld rows, the call brings %lld", (long long)sum, (long long)n_rows); return -1; }
    if ((int64_t)db->n_songs + n_new_songs > 0x7fffffff - 1) { set_error("db_append: too many songs"); return -1; }
    if (n_new_songs == 0) return 0;
    const int d = db->d;
    const int64_t n0 = db->n, n1 = n0 + n_rows;
    const int s0 = db->n_songs, s1 = s0 + n_new_songs;
    const bool f16 = db->storage == PFANN_DB_F16;
    // the first rows of a handle decide about the fp16 copy and the norms as pfann_db_load would
    const bool norms = n0 == 0 ? (f16 || (d % 8 == 0 && getenv("PFANN_NO_F16_PREFILTER") == nullptr)) : db->norms;
    const bool with_h = f16 || (n0 == 0 ? norms : db->emb_h != nullptr);
    std::vector<int64_t> sp1(db->song_pos_h.empty() ? std::vector<int64_t>(1, 0) : db->song_pos_h);
    sp1.reserve((size_t)s1 + 1);
    for (int i = 0; i < n_new_songs; ++i) sp1.push_back(sp1.back() + song_rows_host[i]);

    // ---- everything new is allocated first; the handle's own buffers are written only behind row n, where no query looks
    DbTemps tmp;
    float *new_emb = nullptr, *song_max = nullptr, *nm = nullptr, *stage = nullptr;
    char *new_h = nullptr;
    int64_t *new_sp = nullptr;
    int64_t new_cap = db->cap;
    int new_song_cap = db->song_cap;
    if (n1 > db->cap) {       // geometric growth: one device-to-device copy per matrix
        new_cap = std::max(std::max(n1, db->cap + db->cap / 2), db->want_rows);
        if (!f16) PF_HIP(tmp.get(&new_emb, (size_t)new_cap * d * sizeof(float)));
        if (with_h) PF_HIP(tmp.get(&new_h, (size_t)new_cap * d * 2));
    }
    if (db->song_pos == nullptr || s1 > db->song_cap) {
        new_song_cap = std::max(std::max(s1, db->song_cap + db->song_cap / 2), db->want_songs);
        PF_HIP(tmp.get(&new_sp, (size_t)(new_song_cap + 1) * sizeof(int64_t)));
    }
    if (norms) {
        PF_HIP(tmp.get(&song_max, (size_t)n_new_songs * sizeof(float)));
        PF_HIP(hipMemset(song_max, 0, (size_t)n_new_songs * sizeof(float)));
    }
    PF_HIP(tmp.get(&nm, sizeof(float)));
    PF_HIP(hipMemset(nm, 0, sizeof(float)));
    const int64_t chunk = std::max<int64_t>(1, (64ll << 20) / ((int64_t)d * 4));
    if (f16 && !emb_is_device && n_rows > 0) PF_HIP(tmp.get(&stage, (size_t)std::min(chunk, n_rows) * d * sizeof(float)));
    if (new_emb && n0 > 0) PF_HIP(hipMemcpy(new_emb, db->emb, (size_t)n0 * d * sizeof(float), hipMemcpyDeviceToDevice));
    if (new_h && n0 > 0 && db->emb_h) PF_HIP(hipMemcpy(new_h, db->emb_h, (size_t)n0 * d * 2, hipMemcpyDeviceToDevice));
    if (new_sp) PF_HIP(hipMemcpy(new_sp, sp1.data(), sp1.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    else PF_HIP(hipMemcpy(db->song_pos + s0 + 1, sp1.data() + s0 + 1, (size_t)n_new_songs * sizeof(int64_t), hipMemcpyHostToDevice));
    const int64_t *sp_dev = new_sp ? new_sp : db->song_pos;
    float *E = new_emb ? new_emb : db->emb;
    char *H = with_h ? (new_h ? new_h : reinterpret_cast<char *>(db->emb_h)) : nullptr;

    // ---- the new rows: copied (fp32 storage) or passed through the staging buffer (fp16 storage), the tail of the fp16
    // copy converted, the new songs' norm maxima taken; the old rows are not read
    if (n_rows > 0 && !f16) {
        float *tail = E + (size_t)n0 * d;
        PF_HIP(hipMemcpy(tail, emb, (size_t)n_rows * d * sizeof(float), emb_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        if (H && launch_rows_to_half(tail, n_rows, d, H + (size_t)n0 * d * 2, nm, 0)) return -1;
        if (norms && launch_song_norm_max(tail, n_rows, d, n0, sp_dev, s1, s0, song_max, 0)) return -1;
    } else if (n_rows > 0) {
        for (int64_t r0 = 0; r0 < n_rows; r0 += chunk) {
            const int64_t nr = std::min(chunk, n_rows - r0);
            const float *src = emb + r0 * d;
            if (!emb_is_device) {
                PF_HIP(hipMemcpy(stage, src, (size_t)nr * d * sizeof(float), hipMemcpyHostToDevice));
                src = stage;
            }
            if (launch_rows_to_half(src, nr, d, H + (size_t)(n0 + r0) * d * 2, nm, 0)) return -1;
            if (launch_song_norm_max(src, nr, d, n0 + r0, sp_dev, s1, s0, song_max, 0)) return -1;
            PF_HIP(hipDeviceSynchronize());
        }
    }
    std::vector<float> new_norm((size_t)n_new_songs, 0.f);
    if (norms) PF_HIP(hipMemcpy(new_norm.data(), song_max, (size_t)n_new_songs * sizeof(float), hipMemcpyDeviceToHost));
    PF_HIP(hipDeviceSynchronize());
    float xmax = norms ? db->xnorm_max : 0.f, tail_max = 0.f;
    for (float v : new_norm) tail_max = norm_max2(tail_max, v);
    xmax = norm_max2(xmax, tail_max);
    if (f16 && !(tail_max < 6.0e4f)) {        // pfann_db_load's rule; the handle is as it was
        set_error("db_append: rows with norm %g do not fit fp16 storage", (double)tail_max);
        return -3;
    }
    const bool drop_h = !f16 && H != nullptr && !(xmax < 1.0e4f);      // fp16 range / NaN guard of pfann_db_load

    // ---- commit: nothing below can fail
    if (new_emb) { if (db->emb) (void)hipFree(db->emb); db->emb = new_emb; tmp.keep(new_emb); }
    if (new_h) { if (db->emb_h) (void)hipFree(db->emb_h); db->emb_h = new_h; tmp.keep(new_h); }
    if (drop_h) { (void)hipFree(db->emb_h); db->emb_h = nullptr; }
    if (new_sp) { if (db->song_pos) (void)hipFree(db->song_pos); db->song_pos = new_sp; tmp.keep(new_sp); }
    db->cap = new_cap;
    db->song_cap = new_song_cap;
    db->n = n1;
    db->n_songs = s1;
    db->song_lo = 0;
    db->song_hi = s1;
    db->song_pos_h.swap(sp1);
    db->song_norm.resize((size_t)s0, 0.f);
    db->song_norm.insert(db->song_norm.end(), new_norm.begin(), new_norm.end());
    for (int i = 0; i < n_new_songs; ++i) db->max_song_rows = std::max<int64_t>(db->max_song_rows, song_rows_host[i]);
    if (n1 > 0) { db->norms = norms; db->xnorm_max = xmax; }
    db->ws.bound_valid = false;
    return 0;
}

int pfann_db_remove_songs(pfann_db *db, const int32_t *songs_host, int n) {
    PF_HIP(hipSetDevice(db->device));
    PF_HIP(hipDeviceSynchronize());
    if (n < 0 || (n > 0 && songs_host == nullptr)) { set_error("db_remove_songs: n=%d", n); return -1; }
    if (db_is_shard(db)) {
        set_error("db_remove_songs: the handle holds a shard of the database (monitor mode is not song-sharded)");
        return -1;
    }
    std::vector<char> gone((size_t)db->n_songs, 0);
    for (int i = 0; i < n; ++i) {
        if (songs_host[i] < 0 || songs_host[i] >= db->n_songs) {
            set_error("db_remove_songs: song %d outside 0..%d", songs_host[i], db->n_songs - 1);
            return -1;
        }
        gone[songs_host[i]] = 1;
    }
    if (n == 0 || db->n == 0) return 0;
    const int d = db->d;
    std::vector<DbRun> runs;
    int64_t first = 0;
    const int64_t n1 = db_kept_runs(db->song_pos_h, gone, runs, &first);
    if (n1 == db->n) return 0;                // only songs without rows
    std::vector<int64_t> sp1(db->song_pos_h.size(), 0);
    float xmax = 0.f;
    int64_t longest = 0;
    for (int s = 0; s < db->n_songs; ++s) {
        const int64_t len = gone[s] ? 0 : db->song_pos_h[s + 1] - db->song_pos_h[s];
        sp1[s + 1] = sp1[s] + len;
        longest = std::max(longest, len);
        if (!gone[s] && len > 0) xmax = norm_max2(xmax, db->song_norm[s]);
    }
    if (!db->norms) xmax = 0.f;
    // a fresh load of the rows left keeps an fp16 copy when their norms allow it: the song that stood in its way may be gone
    const bool rebuild_h = db->storage == PFANN_DB_F32 && db->norms && db->emb_h == nullptr && n1 > 0 && xmax < 1.0e4f;
    DbTemps tmp;
    char *stage = nullptr, *new_h = nullptr;
    DbRun *runs_dev = nullptr;
    float *nm = nullptr;
    // rows per chunk of the move: the 64 MB staging of the fp16 load, or PFANN_DB_MOVE_ROWS (read at every call)
    int64_t chunk = std::max<int64_t>(1, (64ll << 20) / ((int64_t)d * 4));
    if (const char *env = getenv("PFANN_DB_MOVE_ROWS")) {
        if (atoll(env) > 0) chunk = atoll(env);
    }
    chunk = std::min<int64_t>(chunk, (1ll << 30) / d);        // (the gather kernel indexes a chunk's vectors with 31 bits)
    const int64_t row_bytes = db->emb ? (int64_t)d * 4 : (int64_t)d * 2;
    if (n1 > first) {
        PF_HIP(tmp.get(&stage, (size_t)(std::min(chunk, n1 - first) * row_bytes)));
        PF_HIP(tmp.get(&runs_dev, runs.size() * sizeof(DbRun)));
    }
    if (rebuild_h) {
        PF_HIP(tmp.get(&new_h, (size_t)db->cap * d * 2));
        PF_HIP(tmp.get(&nm, sizeof(float)));
        PF_HIP(hipMemset(nm, 0, sizeof(float)));
    }
    // ---- the move, every matrix alike: ascending chunks of destination rows, gather -> staging -> down, in stream order
    if (n1 > first) {
        PF_HIP(hipMemcpy(runs_dev, runs.data(), runs.size() * sizeof(DbRun), hipMemcpyHostToDevice));
        struct { char *base; int64_t rb; } mats[2] = {{reinterpret_cast<char *>(db->emb), (int64_t)d * 4},
                                                     {reinterpret_cast<char *>(db->emb_h), (int64_t)d * 2}};
        for (auto &m : mats) {
            if (m.base == nullptr) continue;
            for (int64_t r0 = first; r0 < n1; r0 += chunk) {
                const int64_t nr = std::min(chunk, n1 - r0);
                if (launch_gather_rows(m.base, stage, runs_dev, (int)runs.size(), r0, nr, m.rb, 0)) return -1;
                PF_HIP(hipMemcpyAsync(m.base + (size_t)r0 * m.rb, stage, (size_t)nr * m.rb, hipMemcpyDeviceToDevice, 0));
            }
        }
    }
    if (rebuild_h && launch_rows_to_half(db->emb, n1, d, new_h, nm, 0)) return -1;
    PF_HIP(hipDeviceSynchronize());
    PF_HIP(hipMemcpy(db->song_pos, sp1.data(), sp1.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    if (new_h) { db->emb_h = new_h; tmp.keep(new_h); }
    if (n1 == 0) {                            // what a fresh load of no rows leaves
        if (db->emb) { (void)hipFree(db->emb); db->emb = nullptr; }
        if (db->emb_h) { (void)hipFree(db->emb_h); db->emb_h = nullptr; }
        db->cap = 0;
        db->norms = false;
    }
    db->n = n1;
    db->song_pos_h.swap(sp1);
    db->max_song_rows = longest;
    db->xnorm_max = xmax;
    for (int s = 0; s < db->n_songs; ++s) if (gone[s]) db->song_norm[s] = 0.f;
    db->ws.bound_valid = false;
    return 0;
}

int pfann_search_topk(pfann_db *db, const float *q, int64_t nq, int k, float *D, int64_t *I, void *stream) {
    PF_HIP(hipSetDevice(db->device));
    // the survivor workspace is 64 KB per query row: bound it by walking big batches in chunks
    const int64_t chunk = 16384;
    for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
        const int64_t n = std::min(chunk, nq - q0);
        const int rc = search_topk(db->emb, (db->prefilter || db->emb == nullptr) ? db->emb_h : nullptr, db->xnorm_max, db->n, db->d,
                                   db->label_base, q + q0 * db->d, n, k, D + q0 * k, I + q0 * k, db->ws,
                                   (hipStream_t)stream);
        if (rc) return rc;
    }
    return 0;
}

int pfann_search_topk_excl(pfann_db *db, const float *q, int64_t nq, int k, const int64_t *excl_lo, const int64_t *excl_hi, float *D,
                           int64_t *I, void *stream) {
    if (excl_lo == nullptr && excl_hi == nullptr) return pfann_search_topk(db, q, nq, k, D, I, stream);
    if (excl_lo == nullptr || excl_hi == nullptr) { set_error("pfann_search_topk_excl: one of excl_lo / excl_hi is NULL"); return -1; }
    PF_HIP(hipSetDevice(db->device));
    const int64_t chunk = 16384;
    for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
        const int64_t n = std::min(chunk, nq - q0);
        const int rc = search_topk(db->emb, (db->prefilter || db->emb == nullptr) ? db->emb_h : nullptr, db->xnorm_max, db->n, db->d,
                                   db->label_base, q + q0 * db->d, n, k, D + q0 * k, I + q0 * k, db->ws,
                                   (hipStream_t)stream, 0, nullptr, 1, excl_lo + q0, excl_hi + q0);
        if (rc) return rc;
    }
    return 0;
}

int pfann_search_bound(pfann_db *db, const float *q, int64_t nq, int k, int m, float *lb, void *stream) {
    PF_HIP(hipSetDevice(db->device));
    if (nq > 16384) { set_error("pfann_search_bound: at most 16384 query rows per call (got %lld)", (long long)nq); return -1; }
    if (m < 1 || m > 1024) { set_error("pfann_search_bound: m=%d outside 1..1024", m); return -1; }
    return search_topk(db->emb, (db->prefilter || db->emb == nullptr) ? db->emb_h : nullptr, db->xnorm_max, db->n, db->d,
                       db->label_base, q, nq, k, nullptr, nullptr, db->ws, (hipStream_t)stream, 1, lb, m);
}

int pfann_search_topk_bounded(pfann_db *db, const float *q, int64_t nq, int k, const float *lb, float *D, int64_t *I,
                              void *stream) {
    PF_HIP(hipSetDevice(db->device));
    if (nq > 16384) { set_error("pfann_search_topk_bounded: at most 16384 query rows per call (got %lld)", (long long)nq); return -1; }
    return search_topk(db->emb, (db->prefilter || db->emb == nullptr) ? db->emb_h : nullptr, db->xnorm_max, db->n, db->d,
                       db->label_base, q, nq, k, D, I, db->ws, (hipStream_t)stream, 2, const_cast<float *>(lb));
}

int pfann_search_plan(int64_t n, int d, int64_t nq, int k, int storage, int phase, int resume_with_lb, int mtop, char *buf, int len) {
    if (storage < STORE_F32 || storage > STORE_F16 || phase < 0 || phase > 2 || (buf == nullptr && len > 0)) {
        set_error("pfann_search_plan: storage=%d phase=%d", storage, phase);
        return -1;
    }
    SearchShape sh;
    sh.n = n; sh.d = d; sh.nq = nq; sh.k = k; sh.storage = storage; sh.phase = phase; sh.mtop = mtop;
    sh.resume = phase == 2 && resume_with_lb != 0;
    sh.has_lb = phase == 2;
    return print_search_plan(plan_search(sh, search_tuning()), buf, len);
}

int pfann_encode_plan(const pfann_config *cfg, int64_t B, int64_t plan_batch, int precision, int fused, int taps, int n_streams,
                      char *buf, int len) {
    if (cfg == nullptr || B < 1 || precision < 0 || precision > 1 || taps < 0 || taps > 2 || n_streams < 1 || n_streams > 8 ||
        (buf == nullptr && len > 0) || cfg->stft_hop <= 0) {
        set_error("pfann_encode_plan: B=%lld precision=%d taps=%d streams=%d", (long long)B, precision, taps, n_streams);
        return -1;
    }
    SubLayer sub[16];
    const char *why = plan_sublayers(*cfg, cfg->n_mels, 1 + cfg->segment_len / cfg->stft_hop, sub);
    if (why) { set_error("pfann_encode_plan: %s", why); return -1; }
    // what pfann_create, pfann_set_fused_layernorm, pfann_set_encoder_precision and pfann_set_plan_batch make of the request
    const bool can_fuse = plan_fused_supported(sub, 16) && getenv("PFANN_NO_FUSE") == nullptr;
    const bool use_fused = fused < 0 ? can_fuse : (fused != 0 && plan_fused_supported(sub, 16));
    if (!use_fused) precision = 0;
    const int64_t pinned = plan_batch <= 0 ? 0 : (plan_batch < 65 ? 65 : plan_batch);
    const int64_t max_batch = cfg->max_batch > 0 ? cfg->max_batch : 512;
    if (B > max_batch) B = max_batch;           // the first chunk of a longer call
    const int64_t part_slots = plan_part_slots(sub);
    std::string out;
    char line[320];
    const std::vector<int64_t> chunks = plan_stream_chunks(B, n_streams);
    size_t total = 0;
    int64_t b0 = 0;
    for (size_t k = 0; k < chunks.size(); ++k) {
        const int64_t nb = chunks[k], Bp = pinned > 0 ? pinned : B;        // the variants are those of the whole call
        const size_t need = use_fused ? plan_chunk_scratch(sub, nb, Bp, taps, B) : 0;
        snprintf(line, sizeof line, "chunk %d b0=%lld B=%lld splitk_offset=%zu splitk_bytes=%zu\n", (int)k, (long long)b0, (long long)nb,
                 total, need);
        out += line;
        std::vector<PlannedLaunch> ls;
        plan_chunk_launches(*cfg, sub, nb, Bp, precision, use_fused, taps, ls, B);
        for (const PlannedLaunch &l : ls) {
            snprintf(line, sizeof line, "%s grid=%lld block=%d lds=%zu layer=%d tile=%d n_splits=%d first=%d out_P=%d\n", l.name.c_str(),
                     (long long)l.grid, l.block, l.lds, l.layer, l.tile, l.n_splits, l.first, l.out_P);
            out += line;
        }
        total += (need + 255) / 256 * 256;
        b0 += nb;
    }
    snprintf(line, sizeof line, "flags fused=%d precision=%d plan_batch=%lld fold_first=%d chunks=%d splitk_bytes=%zu part_slots=%lld\n",
             use_fused ? 1 : 0, precision, (long long)pinned, use_fused && plan_fold_first(sub, taps) ? 1 : 0, (int)chunks.size(), total,
             (long long)part_slots);
    out += line;
    if ((int)out.size() + 1 > len) { set_error("pfann_encode_plan: the text needs %d bytes", (int)out.size() + 1); return -2; }
    memcpy(buf, out.c_str(), out.size() + 1);
    return (int)out.size();
}

int pfann_search_plan_excl(int64_t n, int d, int64_t nq, int k, int storage, char *buf, int len) {
    if (storage < STORE_F32 || storage > STORE_F16 || (buf == nullptr && len > 0)) {
        set_error("pfann_search_plan_excl: storage=%d", storage);
        return -1;
    }
    SearchShape sh;
    sh.n = n; sh.d = d; sh.nq = nq; sh.k = k; sh.storage = storage; sh.excl = true;
    return print_search_plan(plan_search(sh, search_tuning()), buf, len);
}

int pfann_topk_merge(pfann_db *db, const float *S, const int64_t *L, int64_t nq, int m, int k, float *D,
                     int64_t *I, void *stream) {
    PF_HIP(hipSetDevice(db->device));
    return topk_merge(S, L, nq, m, k, D, I, (hipStream_t)stream);
}

int pfann_bound_reduce(pfann_db *db, const float *cands_dev, int n_ranks, int64_t nq, int m, int k, float *lb_dev, void *stream) {
    PF_HIP(hipSetDevice(db->device));
    return bound_reduce(cands_dev, n_ranks, nq, m, k, lb_dev, (hipStream_t)stream);
}

int pfann_topk_merge_lists(pfann_db *db, const float *D_lists_dev, const int64_t *I_lists_dev, int n_lists, int64_t nq, int k,
                           float *D_dev, int64_t *I_dev, void *stream) {
    PF_HIP(hipSetDevice(db->device));
    return merge_lists(D_lists_dev, I_lists_dev, n_lists, nq, k, D_dev, I_dev, (hipStream_t)stream);
}

}  // extern "C"

// The handle's grow-only scratch buffers (match_scratch, win_scratch, dense_ws): the larger buffer is allocated FIRST and the old
// one freed only when that succeeded, so a failed allocation leaves the handle as it was (the error is reported as PF_HIP
// reports it); for that moment the old and the new bytes are both held.  drain: earlier calls on `st` may still read the old
// buffer -- wait for them first (not needed where the caller has drained the stream already).
static int grow_scratch(void **buf, size_t *bytes, size_t need, hipStream_t st, bool drain) {
    if (*bytes >= need) return 0;
    if (drain) PF_HIP(hipStreamSynchronize(st));
    void *grown = nullptr;
    PF_HIP(hipMalloc(&grown, need));
    if (*buf) (void)hipFree(*buf);
    *buf = grown;
    *bytes = need;
    return 0;
}

// pfann_match and pfann_match_topn: one set-up, one launch plan (topn == 0: the single answer and the per-song block)
static int match_call(pfann_db *db, const float *q, const int64_t *labels, int k, const int64_t *qstart,
                      const int32_t *qlen, int64_t nQ, int max_qlen, int frame_shift_mul, float score_alpha, int mode,
                      int only_owned, pfann_match_result *results, float *song_scores, int topn, pfann_match_result *top,
                      int32_t *n_found, void *stream) {
    PF_HIP(hipSetDevice(db->device));
    // the contiguous scoring path reads rows as float4 / four halves (rerank.hip), like the search (search.hip: search_topk)
    if (db->d % 4 != 0) { set_error("match: d %% 4 != 0 (d=%d)", db->d); return -1; }
    RerankArgs a;
    a.db = db->emb; a.dbh = db->emb_h; a.n = db->n; a.d = db->d; a.label_base = db->label_base;
    a.song_pos = db->song_pos; a.n_songs = db->n_songs; a.song_lo = db->song_lo; a.song_hi = db->song_hi;
    a.q = q; a.labels = labels; a.k = k; a.qstart = qstart; a.qlen = qlen; a.nQ = nQ;
    a.fsm = frame_shift_mul; a.alpha = score_alpha; a.mode = mode; a.only_owned = only_owned & 1;
    // bit 1 of only_owned (PFANN_MATCH_OWNED_BLOCK): song_scores is [nQ][owned songs][2] instead of [nQ][n_songs][2]
    a.ss_lo = 0; a.ss_n = db->n_songs;
    if (only_owned & 2) {
        if (!(only_owned & 1)) { set_error("match: the owned-songs score block needs only_owned candidates"); return -1; }
        a.ss_lo = db->song_lo; a.ss_n = db->song_hi - db->song_lo;
    }
    int P = 1;
    while (P < (int64_t)max_qlen * k) P <<= 1;
    a.pmax = P;
    a.gkeys = nullptr; a.gscore = nullptr; a.ncand = nullptr; a.phase = 0;
    // a handful of queries: spread each one's candidate scoring over the GPU (three launches: candidates, scores on all CUs,
    // argmax).  One workgroup per query -- the single-launch form -- leaves most of the chip idle below ~128 queries.
    // (round 6, tools/ubench/match_mid.py: 32 queries 0.54 -> 0.21 ms, 64 queries 0.54 -> 0.33, same decisions and scores; at
    // 128 queries the single launch is level, 0.52 vs 0.56; up to round 5 the limit was 16)
    static const int64_t phased_max = getenv("PFANN_MATCH_PHASED_MAX") ? atoll(getenv("PFANN_MATCH_PHASED_MAX")) : 64;
    const bool phased = nQ <= phased_max;
    if (P > 8192 || phased) {     // longer than the LDS candidate buffer, or phased: per-query slabs in HBM
        if ((int64_t)max_qlen * k > (1 << 22)) { set_error("match: query of %d rows x top_k %d is too long", max_qlen, k); return -1; }
        const size_t need = (size_t)nQ * P * 12 + (size_t)nQ * sizeof(int);
        if (grow_scratch(&db->match_scratch, &db->match_scratch_bytes, need, (hipStream_t)stream, true)) return -1;
        a.gkeys = reinterpret_cast<unsigned long long *>(db->match_scratch);
        a.gscore = reinterpret_cast<float *>(a.gkeys + (size_t)nQ * P);
        if (phased) { a.ncand = reinterpret_cast<int *>(a.gscore + (size_t)nQ * P); a.phase = 1; }
    }
    a.results = results; a.song_scores = song_scores;
    a.topn = topn; a.top = top; a.n_found = n_found;
    return launch_match(a, (hipStream_t)stream);
}

// a recording is matched against ALL songs by one GPU: a shard of a song-sharded database cannot answer
static bool db_is_whole(const pfann_db *db) {
    return db->label_base == 0 && db->song_lo == 0 && db->song_hi == db->n_songs && !db->song_pos_h.empty() &&
           db->song_pos_h.back() == db->n;
}
static int refuse_shard() {
    set_error("match_windows: the handle holds a shard of the database (monitor mode is not song-sharded)");
    return -1;
}

// pfann_match_windows (n == 0: results) and pfann_match_windows_topn (n >= 1: top, n_found or null): one set of checks, ONE
// routing -- so that entry 0 of a ranked window and the window's answer come from the same summation order -- and one general
// path; `what` names the call
static int windows_call(const char *what, pfann_db *db, const float *q, const int64_t *labels, int k, const int64_t *rstart,
                        const int32_t *rlen, int64_t nR, int window, int hop, int frame_shift_mul, float score_alpha, int mode,
                        const int64_t *wfirst, pfann_match_result *results, int n, pfann_match_result *top, int32_t *n_found,
                        void *stream) {
    PF_HIP(hipSetDevice(db->device));
    hipStream_t st = (hipStream_t)stream;
    const bool ranked = n != 0;
    if (db->d % 4 != 0) { set_error("%s: d %% 4 != 0 (d=%d)", what, db->d); return -1; }
    if (window < 1 || hop < 1 || k < 1 || nR < 0) { set_error("%s: window=%d hop=%d k=%d nR=%lld", what, window, hop, k, (long long)nR); return -1; }
    if (mode != 0 && mode != 1) { set_error("%s: unknown mode %d", what, mode); return -1; }
    if (!db_is_whole(db)) return refuse_shard();
    if (nR == 0) return 0;
    const int C = match_windows_chunk(k, window, hop);
    // PFANN_WINDOWS_GENERAL=1: every call takes the general path (A/B timing, tests); read per call, no process state
    const char *env = getenv("PFANN_WINDOWS_GENERAL");
    const bool forced = env != nullptr && env[0] != 0 && !(env[0] == '0' && env[1] == 0);
    const bool fast = !forced && mode == 0 && frame_shift_mul == 1 && score_alpha == 0.0f && C >= 1 && n <= WIN_TOPN_FAST &&
                      db->n_songs < (1 << 28) - 1 && db->max_song_rows < (1ll << 28) - 2 * WIN_SMAX;
    if (fast) {
        WindowsTopnArgs a;
        a.db = db->emb; a.dbh = db->emb_h; a.d = db->d; a.song_pos = db->song_pos; a.n_songs = db->n_songs;
        a.q = q; a.labels = labels; a.k = k; a.rstart = rstart; a.rlen = rlen; a.nR = nR;
        a.window = window; a.hop = hop; a.C = C; a.wfirst = wfirst; a.results = results;
        a.n = n; a.top = top; a.n_found = n_found;
        return ranked ? launch_match_windows_topn(a, st) : launch_match_windows(a, st);
    }
    // ---- general path: the windows become (qstart, qlen) pairs on the device and go through match_call.  Its launches
    // are sized on the host, so the number of windows is read back first: ONE synchronisation with the stream.
    int64_t nW = 0;
    PF_HIP(hipMemcpyAsync(&nW, wfirst + nR, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PF_HIP(hipStreamSynchronize(st));
    if (nW <= 0) return 0;
    const size_t o_ql = (size_t)nW * sizeof(int64_t), need = o_ql + (size_t)nW * sizeof(int32_t);
    if (grow_scratch(&db->win_scratch, &db->win_scratch_bytes, need, st, false)) return -1;    // (the stream was drained above)
    int64_t *qs = reinterpret_cast<int64_t *>(db->win_scratch);
    int32_t *ql = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(db->win_scratch) + o_ql);
    if (launch_expand_windows(rstart, rlen, nR, window, hop, wfirst, nW, qs, ql, st)) return -1;
    // windows per match_call: its HBM slabs (lists longer than the LDS, or few queries) stay below 256 MB
    int64_t P = 1;
    while (P < (int64_t)window * k) P <<= 1;
    const int64_t step = P > 8192 ? std::max<int64_t>(1, (256ll << 20) / (P * 12)) : 65536;
    for (int64_t j0 = 0; j0 < nW; j0 += step) {
        const int64_t m = std::min(step, nW - j0);
        if (match_call(db, q, labels, k, qs + j0, ql + j0, m, window, frame_shift_mul, score_alpha, mode, 0,
                       ranked ? nullptr : results + j0, nullptr, n, ranked ? top + j0 * n : nullptr,
                       n_found != nullptr ? n_found + j0 : nullptr, stream))
            return -1;
    }
    return 0;
}

extern "C" {

int pfann_match(pfann_db *db, const float *q, const int64_t *labels, int k, const int64_t *qstart,
                const int32_t *qlen, int64_t nQ, int max_qlen, int frame_shift_mul, float score_alpha, int mode,
                int only_owned, pfann_match_result *results, float *song_scores, void *stream) {
    return match_call(db, q, labels, k, qstart, qlen, nQ, max_qlen, frame_shift_mul, score_alpha, mode, only_owned, results,
                      song_scores, 0, nullptr, nullptr, stream);
}

int pfann_match_topn(pfann_db *db, const float *q, const int64_t *labels, int k, const int64_t *qstart,
                     const int32_t *qlen, int64_t nQ, int max_qlen, int frame_shift_mul, float score_alpha, int mode,
                     int only_owned, int n, pfann_match_result *top, int32_t *n_found, void *stream) {
    if (n < 1 || n > 64) { set_error("match_topn: n=%d outside 1..64", n); return -1; }
    if (mode != 0 && mode != 1) { set_error("match_topn: unknown mode %d", mode); return -1; }
    if (only_owned & ~1) { set_error("match_topn: only_owned=%d (the owned-songs score block has no meaning here)", only_owned); return -1; }
    if (top == nullptr) { set_error("match_topn: top_dev is null"); return -1; }
    return match_call(db, q, labels, k, qstart, qlen, nQ, max_qlen, frame_shift_mul, score_alpha, mode, only_owned, nullptr,
                      nullptr, n, top, n_found, stream);
}

int pfann_match_windows(pfann_db *db, const float *q, const int64_t *labels, int k, const int64_t *rstart, const int32_t *rlen,
                        int64_t nR, int window, int hop, int frame_shift_mul, float score_alpha, int mode,
                        const int64_t *wfirst, pfann_match_result *results, void *stream) {
    return windows_call("match_windows", db, q, labels, k, rstart, rlen, nR, window, hop, frame_shift_mul, score_alpha, mode, wfirst,
                        results, 0, nullptr, nullptr, stream);
}

// ---- dense matcher: the three calls on one handle of the whole database, the parts on any fp32 handle, the merges on any handle
// The refusals the calls share, in the order each call has always reported them.  whole: the handle must hold the whole database,
// and window, hop, nR and n_windows are one refusal; otherwise window is checked before the id bound and the rest after it.
// needs_rows: the call reads the handle's rows (everything but pfann_match_windows_dense_merge, which passes hop 1).  The id
// bound is that of the WHOLE database (every handle has its song_pos).
static int dense_check(const char *what, pfann_db *db, int window, int hop, int64_t nR, int64_t n_windows, bool needs_rows, bool whole) {
    if (whole) {
        if (!db_is_whole(db)) return refuse_shard();
    } else if (db->song_pos_h.empty()) {
        set_error("%s: no database loaded", what);
        return -1;
    }
    if (needs_rows && (db->storage != PFANN_DB_F32 || (db->n > 0 && db->emb == nullptr))) {
        set_error("%s: fp16-only storage (the dense matcher scores fp32 rows)", what);
        return -1;
    }
    if (needs_rows && db->d % 4 != 0) { set_error("%s: d %% 4 != 0 (d=%d)", what, db->d); return -1; }
    const bool counts_bad = hop < 1 || nR < 0 || n_windows < 0;
    // whole handles: window and the counts are ONE refusal, so of everything below only the id bound can still fire for them
    if (whole && (window < 1 || window > 64 || counts_bad)) {
        set_error("%s: window=%d (1..64) hop=%d nR=%lld n_windows=%lld", what, window, hop, (long long)nR, (long long)n_windows);
        return -1;
    }
    // parts and the merge: window, the id bound, (parts) rows against songs, the counts
    if (window < 1 || window > 64) { set_error("%s: window=%d outside 1..64", what, window); return -1; }
    if (db->song_pos_h.back() + (int64_t)db->n_songs * (window - 1) >= (1ll << 32)) {
        set_error("%s: %lld rows and %d songs at window %d do not fit the 32-bit alignment id", what, (long long)db->song_pos_h.back(),
                  db->n_songs, window);
        return -1;
    }
    // the owned songs span exactly the handle's rows (pfann_db_load, pfann_db_set_owned_songs): the ranked workspace relies on it
    // (a whole handle passed db_is_whole above, which says the same)
    if (needs_rows && !whole && (db->song_lo < 0 || db->song_hi < db->song_lo || db->song_hi > db->n_songs ||
                                 db->song_pos_h[db->song_lo] != db->label_base || db->song_pos_h[db->song_hi] != db->label_base + db->n)) {
        set_error("%s: the handle's rows [%lld,%lld) are not its songs [%d,%d)", what, (long long)db->label_base,
                  (long long)(db->label_base + db->n), db->song_lo, db->song_hi);
        return -1;
    }
    if (counts_bad) {
        if (needs_rows) set_error("%s: hop=%d nR=%lld n_windows=%lld", what, hop, (long long)nR, (long long)n_windows);
        else set_error("%s: nR=%lld n_windows=%lld", what, (long long)nR, (long long)n_windows);
        return -1;
    }
    return 0;
}

// songs of the database with len > 0 (n_cand)
static int64_t songs_with_rows(const pfann_db *db) {
    int64_t with_rows = 0;
    for (int s = 0; s < db->n_songs; ++s) with_rows += db->song_pos_h[s + 1] > db->song_pos_h[s];
    return with_rows;
}

// what every form of the tile kernel takes from the handle and the call (after dense_check); the outputs of the form are the caller's
static DenseArgs dense_args(const pfann_db *db, const float *q, const int64_t *rstart, const int32_t *rlen, int64_t nR, int window,
                            int hop, const int64_t *wfirst, int64_t n_windows, const int32_t *excl_song) {
    DenseArgs a = {};
    a.db = db->emb; a.ntotal = db->song_pos_h.back(); a.d = db->d; a.song_pos = db->song_pos; a.n_songs = db->n_songs;
    a.q = q; a.rstart = rstart; a.rlen = rlen; a.nR = nR; a.window = window; a.hop = hop; a.wfirst = wfirst;
    a.nW = n_windows; a.excl = excl_song;
    a.row_lo = db->label_base; a.nrows = db->n; a.song_lo = db->song_lo; a.n_owned = db->song_hi - db->song_lo;
    return a;
}

// the unranked calls: pfann_match_windows_dense / _stats (results, and stats or null) on a whole handle, _part (words, and stats
// or null) on any fp32 handle; `what` names the call
static int dense_unranked_call(const char *what, pfann_db *db, bool shard, const float *q, const int64_t *rstart, const int32_t *rlen,
                               int64_t nR, int window, int hop, const int64_t *wfirst, int64_t n_windows, const int32_t *excl_song,
                               pfann_match_result *results, uint64_t *words, pfann_dense_stats *stats, void *stream) {
    PF_HIP(hipSetDevice(db->device));
    if (shard && words == nullptr) { set_error("%s: words_dev is null", what); return -1; }
    if (dense_check(what, db, window, hop, nR, n_windows, true, !shard)) return -1;
    if (nR == 0 || n_windows == 0) return 0;
    DenseArgs a = dense_args(db, q, rstart, rlen, nR, window, hop, wfirst, n_windows, excl_song);
    a.results = results; a.words = reinterpret_cast<unsigned long long *>(words); a.stats = stats;
    return launch_dense_unranked(a, shard, shard ? 0 : songs_with_rows(db), (hipStream_t)stream);
}

int pfann_match_windows_dense(pfann_db *db, const float *q, const int64_t *rstart, const int32_t *rlen, int64_t nR, int window,
                              int hop, const int64_t *wfirst, int64_t n_windows, const int32_t *excl_song,
                              pfann_match_result *results, void *stream) {
    return dense_unranked_call("match_windows_dense", db, false, q, rstart, rlen, nR, window, hop, wfirst, n_windows, excl_song,
                               results, nullptr, nullptr, stream);
}

int pfann_match_windows_dense_stats(pfann_db *db, const float *q, const int64_t *rstart, const int32_t *rlen, int64_t nR, int window,
                                    int hop, const int64_t *wfirst, int64_t n_windows, const int32_t *excl_song,
                                    pfann_match_result *results, pfann_dense_stats *stats, void *stream) {
    if (stats == nullptr) { set_error("match_windows_dense_stats: stats_dev is null"); return -1; }
    return dense_unranked_call("match_windows_dense_stats", db, false, q, rstart, rlen, nR, window, hop, wfirst, n_windows, excl_song,
                               results, nullptr, stats, stream);
}

int pfann_match_windows_dense_part(pfann_db *db, const float *q, const int64_t *rstart, const int32_t *rlen, int64_t nR, int window,
                                   int hop, const int64_t *wfirst, int64_t n_windows, const int32_t *excl_song, uint64_t *words,
                                   pfann_dense_stats *stats, void *stream) {
    return dense_unranked_call("match_windows_dense_part", db, true, q, rstart, rlen, nR, window, hop, wfirst, n_windows, excl_song,
                               nullptr, words, stats, stream);
}

// the ranked calls: pfann_match_windows_dense_topn on a whole handle, _topn_part (no per-song block) on any fp32 handle.  Chunks of
// whole row-tile slots: the workspace holds 8 bytes per (window the chunk's slots can hold, song of the handle), at most 256 MB
// unless one slot alone needs more; PFANN_DENSE_TOPN_WINDOWS (read per call) lowers the windows per chunk.  stats (whole handles
// only, or null): pfann_match_windows_dense_topn_stats -- zeroed ONCE, before the first chunk: the tile kernel adds into the
// windows of the call, and every (window, tile) pair belongs to exactly one chunk
static int dense_ranked_call(const char *what, pfann_db *db, bool shard, const float *q, const int64_t *rstart, const int32_t *rlen,
                             int64_t nR, int window, int hop, const int64_t *wfirst, int64_t n_windows, const int32_t *excl_song, int n,
                             pfann_match_result *top, int32_t *n_found, float *song_scores, pfann_dense_stats *stats, void *stream) {
    PF_HIP(hipSetDevice(db->device));
    hipStream_t st = (hipStream_t)stream;
    if (n < 1 || n > 64) { set_error("%s: n=%d outside 1..64", what, n); return -1; }
    if (top == nullptr) { set_error("%s: top_dev is null", what); return -1; }
    if (dense_check(what, db, window, hop, nR, n_windows, true, !shard)) return -1;
    if (nR == 0 || n_windows == 0) return 0;
    DenseArgs a = dense_args(db, q, rstart, rlen, nR, window, hop, wfirst, n_windows, excl_song);
    const int wps = dense_topn_wps(window, hop);
    const int64_t n_slots = dense_topn_slots(n_windows, nR, window, hop);
    const int64_t songs = std::max(shard ? a.n_owned : a.n_songs, 1);
    int64_t cap = (256ll << 20) / (8 * songs);
    const char *env = getenv("PFANN_DENSE_TOPN_WINDOWS");
    if (env != nullptr && env[0] != 0 && atoll(env) > 0) cap = std::min<int64_t>(cap, atoll(env));
    const int64_t step = std::min(n_slots, std::max<int64_t>(1, cap / wps));
    const size_t need = (size_t)step * wps * songs * 8;
    // (growing drains the stream, the one exception to the asynchrony: earlier calls may still read the workspace)
    if (grow_scratch(&db->dense_ws, &db->dense_ws_bytes, need, st, true)) return -1;
    a.ws = reinterpret_cast<unsigned long long *>(db->dense_ws); a.wps = wps;
    a.n = n; a.top = top; a.n_found = n_found; a.song_scores = song_scores; a.stats = stats;
    if (stats != nullptr) PF_HIP(hipMemsetAsync(stats, 0, (size_t)n_windows * sizeof(pfann_dense_stats), st));
    for (int64_t s0 = 0; s0 < n_slots; s0 += step) {
        a.slot_lo = s0; a.slot_n = std::min(step, n_slots - s0);
        if (launch_dense_ranked(a, shard, st)) return -1;
    }
    return 0;
}

int pfann_match_windows_dense_topn(pfann_db *db, const float *q, const int64_t *rstart, const int32_t *rlen, int64_t nR, int window,
                                   int hop, const int64_t *wfirst, int64_t n_windows, const int32_t *excl_song, int n,
                                   pfann_match_result *top, int32_t *n_found, float *song_scores, void *stream) {
    return dense_ranked_call("match_windows_dense_topn", db, false, q, rstart, rlen, nR, window, hop, wfirst, n_windows, excl_song, n, top,
                             n_found, song_scores, nullptr, stream);
}

int pfann_match_windows_dense_topn_stats(pfann_db *db, const float *q, const int64_t *rstart, const int32_t *rlen, int64_t nR,
                                         int window, int hop, const int64_t *wfirst, int64_t n_windows, const int32_t *excl_song,
                                         int n, pfann_match_result *top, int32_t *n_found, float *song_scores,
                                         pfann_dense_stats *stats, void *stream) {
    if (stats == nullptr) { set_error("match_windows_dense_topn_stats: stats_dev is null"); return -1; }
    return dense_ranked_call("match_windows_dense_topn_stats", db, false, q, rstart, rlen, nR, window, hop, wfirst, n_windows, excl_song,
                             n, top, n_found, song_scores, stats, stream);
}

int pfann_match_windows_dense_topn_part(pfann_db *db, const float *q, const int64_t *rstart, const int32_t *rlen, int64_t nR,
                                        int window, int hop, const int64_t *wfirst, int64_t n_windows, const int32_t *excl_song,
                                        int n, pfann_match_result *top, int32_t *n_found, void *stream) {
    return dense_ranked_call("match_windows_dense_topn_part", db, true, q, rstart, rlen, nR, window, hop, wfirst, n_windows, excl_song, n,
                             top, n_found, nullptr, nullptr, stream);
}

// the rescoring stage: the listed songs of every query, every alignment (dense_songs.hip).  The packed words live in top_dev's
// score fields between its two kernels, so the call needs no workspace
int pfann_match_songs_dense(pfann_db *db, const float *q, const int64_t *qstart, const int32_t *qlen, int64_t nQ,
                            const pfann_match_result *cand, int m, pfann_match_result *top, int32_t *n_found, void *stream) {
    const char *what = "match_songs_dense";
    PF_HIP(hipSetDevice(db->device));
    if (!db_is_whole(db)) return refuse_shard();
    if (db->storage != PFANN_DB_F32 || (db->n > 0 && db->emb == nullptr)) {
        set_error("%s: fp16-only storage (the dense matcher scores fp32 rows)", what);
        return -1;
    }
    if (m < 1 || m > 64) { set_error("%s: m=%d outside 1..64", what, m); return -1; }
    if (db->d % 4 != 0) { set_error("%s: d %% 4 != 0 (d=%d)", what, db->d); return -1; }
    if (nQ < 0) { set_error("%s: nQ=%lld", what, (long long)nQ); return -1; }
    if (cand == nullptr || top == nullptr) { set_error("%s: cand_dev or top_dev is null", what); return -1; }
    // an alignment id is offset + n - 1 < len + 63, kept in 32 bits
    if (db->max_song_rows + PFANN_SONGS_DENSE_MAX_ROWS >= (1ll << 31)) {
        set_error("%s: a song of %lld rows does not fit the 32-bit alignment id", what, (long long)db->max_song_rows);
        return -1;
    }
    if (nQ == 0) return 0;
    SongsDenseArgs a;
    a.db = db->emb; a.d = db->d; a.song_pos = db->song_pos; a.n_songs = db->n_songs;
    a.q = q; a.qstart = qstart; a.qlen = qlen; a.nQ = nQ; a.cand = cand; a.m = m; a.top = top; a.n_found = n_found;
    return launch_match_songs_dense(a, (hipStream_t)stream);
}

// the nomination in front of it (nominate.hip): chunks of queries whose scratch -- 4 bytes per (query, song), the packed fp16
// query rows, their bounds and norms -- fits 256 MB unless one query alone needs more; PFANN_NOMINATE_QUERIES (read per call)
// lowers the queries per chunk.  The scratch is the handle's dense_ws, grown on demand
int pfann_nominate_songs_dense(pfann_db *db, const float *q, const int64_t *qstart, const int32_t *qlen, int64_t nQ, int max_qlen,
                               int n, pfann_match_result *cand, int32_t *n_found, int32_t *n_close, void *stream) {
    const char *what = "nominate_songs_dense";
    PF_HIP(hipSetDevice(db->device));
    hipStream_t st = (hipStream_t)stream;
    if (!db_is_whole(db)) return refuse_shard();
    if (db->storage != PFANN_DB_F32 || (db->n > 0 && db->emb == nullptr)) {
        set_error("%s: fp16-only storage (the dense matcher scores fp32 rows)", what);
        return -1;
    }
    if (db->n > 0 && db->emb_h == nullptr) {
        set_error("%s: the handle keeps no fp16 copy of its rows (d %% 8 != 0, PFANN_NO_F16_PREFILTER at load, or row norms >= 1e4; d=%d)",
                  what, db->d);
        return -1;
    }
    if (n < 1 || n > 64) { set_error("%s: n=%d outside 1..64", what, n); return -1; }
    if (max_qlen < 1 || max_qlen > 64) { set_error("%s: max_qlen=%d outside 1..64", what, max_qlen); return -1; }
    if (nQ < 0) { set_error("%s: nQ=%lld", what, (long long)nQ); return -1; }
    if (cand == nullptr) { set_error("%s: cand_dev is null", what); return -1; }
    if (nQ == 0) return 0;
    NominateArgs a = {};
    a.dbh = db->emb_h; a.ntotal = db->n; a.d = db->d; a.xnorm_max = db->xnorm_max; a.song_pos = db->song_pos; a.n_songs = db->n_songs;
    a.q = q; a.qstart = qstart; a.qlen = qlen; a.nQ = nQ; a.max_qlen = max_qlen;
    a.n = n; a.cand = cand; a.n_found = n_found; a.n_close = n_close;
    int64_t step = std::max<int64_t>(1, (int64_t)((256ull << 20) / nominate_query_bytes(a.n_songs, max_qlen, a.d)));
    const char *env = getenv("PFANN_NOMINATE_QUERIES");
    if (env != nullptr && env[0] != 0 && atoll(env) > 0) step = std::min<int64_t>(step, atoll(env));
    step = std::min(step, nQ);
    // (growing drains the stream, the one exception to the asynchrony: earlier calls may still read the scratch)
    if (grow_scratch(&db->dense_ws, &db->dense_ws_bytes, nominate_scratch_bytes(step, a.n_songs, max_qlen, a.d), st, true)) return -1;
    for (int64_t j0 = 0; j0 < nQ; j0 += step) {
        a.q_lo = j0; a.q_n = std::min(step, nQ - j0);
        nominate_scratch_layout(a, db->dense_ws);
        if (launch_nominate_songs_dense(a, st)) return -1;
    }
    return 0;
}

// the nomination for every window of long recordings (nominate_windows.hip).  The scratch is the handle's dense_ws: the call's
// fp16 row image with its bounds, norms and flags, then the ws of one chunk.  Chunks of whole row-tile slots as in
// dense_ranked_call: 4 bytes per (window the chunk's slots can hold, song), at most 256 MB unless one slot alone needs more;
// PFANN_NOMINATE_WINDOWS (read per call) lowers the windows per chunk
int pfann_nominate_windows_dense(pfann_db *db, const float *q, const int64_t *rstart, const int32_t *rlen, int64_t nR, int window,
                                 int hop, const int64_t *wfirst, int64_t n_windows, const int32_t *excl_song, int n,
                                 pfann_match_result *cand, int32_t *n_found, int32_t *n_close, void *stream) {
    const char *what = "nominate_windows_dense";
    PF_HIP(hipSetDevice(db->device));
    hipStream_t st = (hipStream_t)stream;
    if (!db_is_whole(db)) return refuse_shard();
    if (db->storage != PFANN_DB_F32 || (db->n > 0 && db->emb == nullptr)) {
        set_error("%s: fp16-only storage (the dense matcher scores fp32 rows)", what);
        return -1;
    }
    if (db->n > 0 && db->emb_h == nullptr) {
        set_error("%s: the handle keeps no fp16 copy of its rows (d %% 8 != 0, PFANN_NO_F16_PREFILTER at load, or row norms >= 1e4; d=%d)",
                  what, db->d);
        return -1;
    }
    if (n < 1 || n > 64) { set_error("%s: n=%d outside 1..64", what, n); return -1; }
    if (window < 1 || window > 64) { set_error("%s: window=%d outside 1..64", what, window); return -1; }
    if (hop < 1) { set_error("%s: hop=%d", what, hop); return -1; }
    if (nR < 0 || n_windows < 0) { set_error("%s: nR=%lld n_windows=%lld", what, (long long)nR, (long long)n_windows); return -1; }
    if (cand == nullptr) { set_error("%s: cand_dev is null", what); return -1; }
    if (nR == 0 || n_windows == 0) return 0;
    NominateWindowsArgs a = {};
    a.dbh = db->emb_h; a.ntotal = db->n; a.d = db->d; a.xnorm_max = db->xnorm_max; a.song_pos = db->song_pos; a.n_songs = db->n_songs;
    a.q = q; a.rstart = rstart; a.rlen = rlen; a.nR = nR; a.window = window; a.hop = hop; a.wfirst = wfirst; a.nW = n_windows;
    a.excl = excl_song;
    a.n = n; a.cand = cand; a.n_found = n_found; a.n_close = n_close;
    a.n_rows = nominate_windows_rows(n_windows, nR, window, hop);
    a.wps = dense_topn_wps(window, hop);
    const int64_t n_slots = dense_topn_slots(n_windows, nR, window, hop);
    const int64_t songs = std::max(a.n_songs, 1);
    int64_t cap = (256ll << 20) / (4 * songs);
    const char *env = getenv("PFANN_NOMINATE_WINDOWS");
    if (env != nullptr && env[0] != 0 && atoll(env) > 0) cap = std::min<int64_t>(cap, atoll(env));
    const int64_t step = std::min(n_slots, std::max<int64_t>(1, cap / a.wps));
    const size_t need = nominate_windows_image_bytes(a.n_rows, a.d) + (size_t)step * a.wps * songs * 4;
    // (growing drains the stream, the one exception to the asynchrony: earlier calls may still read the scratch)
    if (grow_scratch(&db->dense_ws, &db->dense_ws_bytes, need, st, true)) return -1;
    nominate_windows_scratch_layout(a, db->dense_ws);
    if (launch_nominate_windows_prep(a, st)) return -1;
    for (int64_t s0 = 0; s0 < n_slots; s0 += step) {
        a.slot_lo = s0; a.slot_n = std::min(step, n_slots - s0);
        if (launch_nominate_windows_dense(a, st)) return -1;
    }
    return 0;
}

int pfann_match_windows_dense_merge(pfann_db *db, const uint64_t *words, const pfann_dense_stats *part_stats, int n_parts,
                                    const int32_t *rlen, int64_t nR, int window, const int64_t *wfirst, int64_t n_windows,
                                    const int32_t *excl_song, pfann_match_result *results, pfann_dense_stats *stats, void *stream) {
    const char *what = "match_windows_dense_merge";
    PF_HIP(hipSetDevice(db->device));
    if (words == nullptr || results == nullptr) { set_error("%s: words_dev or results_dev is null", what); return -1; }
    if ((part_stats == nullptr) != (stats == nullptr)) {
        set_error("%s: part_stats_dev and stats_dev go together (both or neither)", what);
        return -1;
    }
    if (n_parts < 1) { set_error("%s: n_parts=%d", what, n_parts); return -1; }
    if (dense_check(what, db, window, 1, nR, n_windows, false, false)) return -1;
    if (nR == 0 || n_windows == 0) return 0;
    DenseMergeArgs a;
    a.song_pos = db->song_pos; a.n_songs = db->n_songs; a.ntotal = db->song_pos_h.back(); a.songs_with_rows = songs_with_rows(db);
    a.words = reinterpret_cast<const unsigned long long *>(words); a.part_stats = part_stats; a.n_parts = n_parts;
    a.rlen = rlen; a.nR = nR; a.window = window; a.wfirst = wfirst; a.nW = n_windows; a.excl = excl_song;
    a.results = results; a.stats = stats;
    return launch_dense_merge(a, (hipStream_t)stream);
}

int pfann_match_windows_dense_topn_merge(pfann_db *db, const pfann_match_result *tops, const int32_t *n_found_parts, int n_parts,
                                         int64_t n_windows, int n, pfann_match_result *top, int32_t *n_found, void *stream) {
    const char *what = "match_windows_dense_topn_merge";
    PF_HIP(hipSetDevice(db->device));
    if (n < 1 || n > 64) { set_error("%s: n=%d outside 1..64", what, n); return -1; }
    if (tops == nullptr || top == nullptr) { set_error("%s: tops_dev or top_dev is null", what); return -1; }
    if ((n_found_parts == nullptr) != (n_found == nullptr)) {
        set_error("%s: n_found_parts_dev and n_found_dev go together (both or neither)", what);
        return -1;
    }
    if (n_parts < 1 || n_windows < 0) { set_error("%s: n_parts=%d n_windows=%lld", what, n_parts, (long long)n_windows); return -1; }
    return launch_dense_topn_merge(tops, n_found_parts, n_parts, n_windows, n, top, n_found, (hipStream_t)stream);
}

int pfann_match_windows_topn(pfann_db *db, const float *q, const int64_t *labels, int k, const int64_t *rstart, const int32_t *rlen,
                             int64_t nR, int window, int hop, int frame_shift_mul, float score_alpha, int mode,
                             const int64_t *wfirst, int n, pfann_match_result *top, int32_t *n_found, void *stream) {
    if (n < 1 || n > 64) { set_error("match_windows_topn: n=%d outside 1..64", n); return -1; }
    if (top == nullptr) { set_error("match_windows_topn: top_dev is null"); return -1; }
    return windows_call("match_windows_topn", db, q, labels, k, rstart, rlen, nR, window, hop, frame_shift_mul, score_alpha, mode,
                        wfirst, nullptr, n, top, n_found, stream);
}

int pfann_song_scores_to_seconds(pfann_db *db, float *song_scores_dev, int64_t n_pairs, int frame_shift_mul, double hop_size,
                                 int native_path, void *stream) {
    PF_HIP(hipSetDevice(db->device));
    return launch_song_scores_to_seconds(song_scores_dev, n_pairs, frame_shift_mul, hop_size, native_path, (hipStream_t)stream);
}

int pfann_db_set_owned_songs(pfann_db *db, int song_lo, int song_hi) {
    // the caller's own cut (pfann_amd/dist.py: shard_songs): songs without rows at a shard boundary belong to whichever side
    // the CUT says, which the row range alone cannot tell
    if (song_lo < 0 || song_hi < song_lo || song_hi > db->n_songs || (size_t)db->n_songs + 1 != db->song_pos_h.size()) {
        set_error("db_set_owned_songs: [%d,%d) outside 0..%d", song_lo, song_hi, db->n_songs);
        return -1;
    }
    if (db->song_pos_h[song_lo] != db->label_base || db->song_pos_h[song_hi] != db->label_base + db->n) {
        set_error("db_set_owned_songs: songs [%d,%d) are rows [%lld,%lld), the shard holds [%lld,%lld)", song_lo, song_hi,
                  (long long)db->song_pos_h[song_lo], (long long)db->song_pos_h[song_hi], (long long)db->label_base,
                  (long long)(db->label_base + db->n));
        return -3;
    }
    db->song_lo = song_lo;
    db->song_hi = song_hi;
    return 0;
}

int pfann_db_owned_songs(pfann_db *db, int *song_lo, int *song_hi) {
    if (song_lo) *song_lo = db->song_lo;
    if (song_hi) *song_hi = db->song_hi;
    return db->song_hi - db->song_lo;
}

int pfann_match_pack(pfann_db *db, const pfann_match_result *results_dev, int64_t nQ, uint64_t *keys_dev, void *stream) {
    PF_HIP(hipSetDevice(db->device));
    return launch_match_pack(results_dev, nQ, reinterpret_cast<unsigned long long *>(keys_dev), (hipStream_t)stream);
}

int pfann_match_pick(pfann_db *db, const uint64_t *keys_dev, int n_ranks, int64_t nQ, pfann_match_result *out_dev, void *stream) {
    PF_HIP(hipSetDevice(db->device));
    if (n_ranks < 1) { set_error("pfann_match_pick: n_ranks < 1"); return -1; }
    return launch_match_pick(reinterpret_cast<const unsigned long long *>(keys_dev), n_ranks, nQ, out_dev, (hipStream_t)stream);
}

int seq_score(void *index, const int64_t *song_pos, int n_songs, const float *query, int query_len,
              const int64_t *labels, int top_k, float *song_scores, int frame_shift_mul, float score_alpha) {
    pfann_db *db = (pfann_db *)index;
    if (!db) { set_error("seq_score: null index"); return -1; }
    if (hipSetDevice(db->device) != hipSuccess) { set_error("seq_score: hipSetDevice failed"); return -1; }
    if (n_songs != db->n_songs || memcmp(song_pos, db->song_pos_h.data(), sizeof(int64_t) * (n_songs + 1)) != 0) {
        set_error("seq_score: song_pos differs from the one the database handle was loaded with");
        return -1;
    }
    if (query_len <= 0 || top_k <= 0) return -1;
    // One device slab and one pinned host image, kept in the handle between calls (grown on demand), laid out
    //   [song_scores f32 n_songs*2 | result | qstart i64 | qlen i32 | query f32 | labels i64]
    // Per call: host memcpy of the inputs into the pinned image, then on the handle's private stream 1 memset + 1 H2D
    // + the match launches + 1 D2H, and ONE wait for that stream.  No allocation, no pageable staging copies, no
    // null-stream synchronisation with whatever else the process has in flight.
    std::lock_guard<std::mutex> lock(db->seq_mu);
    const size_t nq = (size_t)query_len;
    const size_t ss_bytes = (size_t)std::max(n_songs, 1) * 2 * sizeof(float);
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t o_res = up16(ss_bytes), o_qs = o_res + up16(sizeof(pfann_match_result)), o_ql = o_qs + 16;
    const size_t o_q = o_ql + 16, o_l = o_q + up16(nq * db->d * sizeof(float));
    const size_t total = o_l + nq * top_k * sizeof(int64_t);
    if (!db->seq_stream && hipStreamCreateWithFlags(&db->seq_stream, hipStreamNonBlocking) != hipSuccess) {
        set_error("seq_score: stream creation failed");
        return -1;
    }
    hipStream_t st = db->seq_stream;
    if (db->seq_scratch_bytes < total) {
        if (db->seq_scratch) { (void)hipStreamSynchronize(st); (void)hipFree(db->seq_scratch); }
        db->seq_scratch = nullptr; db->seq_scratch_bytes = 0;
        if (hipMalloc(&db->seq_scratch, total + (total >> 2)) != hipSuccess) { set_error("seq_score: device allocation failed"); return -1; }
        db->seq_scratch_bytes = total + (total >> 2);
    }
    if (db->seq_host_bytes < total) {
        if (db->seq_host) { (void)hipStreamSynchronize(st); (void)hipHostFree(db->seq_host); }
        db->seq_host = nullptr; db->seq_host_bytes = 0;
        if (hipHostMalloc(reinterpret_cast<void **>(&db->seq_host), total + (total >> 2), hipHostMallocDefault) != hipSuccess) {
            set_error("seq_score: pinned host allocation failed");
            return -1;
        }
        db->seq_host_bytes = total + (total >> 2);
    }
    char *dev = reinterpret_cast<char *>(db->seq_scratch);
    char *host = db->seq_host;
    const int64_t zero = 0;
    const int32_t ql = query_len;
    memcpy(host + o_qs, &zero, sizeof(zero));
    memcpy(host + o_ql, &ql, sizeof(ql));
    memcpy(host + o_q, query, nq * db->d * sizeof(float));
    memcpy(host + o_l, labels, nq * top_k * sizeof(int64_t));
    if (hipMemsetAsync(dev, 0, ss_bytes, st) != hipSuccess ||
        hipMemcpyAsync(dev + o_qs, host + o_qs, total - o_qs, hipMemcpyHostToDevice, st) != hipSuccess) {
        set_error("seq_score: upload failed");
        return -1;
    }
    if (pfann_match(db, reinterpret_cast<float *>(dev + o_q), reinterpret_cast<int64_t *>(dev + o_l), top_k,
                    reinterpret_cast<int64_t *>(dev + o_qs), reinterpret_cast<int32_t *>(dev + o_ql), 1, query_len,
                    frame_shift_mul, score_alpha, 1, 0, reinterpret_cast<pfann_match_result *>(dev + o_res),
                    reinterpret_cast<float *>(dev), st) != 0) return -1;
    if (hipMemcpyAsync(host, dev, o_qs, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) { set_error("seq_score: download failed"); return -1; }
    pfann_match_result res;
    memcpy(&res, host + o_res, sizeof(res));
    if (res.song == -2) { set_error("seq_score: query_len*top_k too large for the candidate buffer"); return -1; }
    const float *ss = reinterpret_cast<const float *>(host);
    for (int s = 0; s < n_songs; ++s)            // seqscore.cpp:126-133 against the caller's slots
        if (ss[2 * s] > song_scores[2 * s]) { song_scores[2 * s] = ss[2 * s]; song_scores[2 * s + 1] = ss[2 * s + 1]; }
    return res.song;
}

// ---- profiling ------------------------------------------------------------------------
void pfann_prof_marker(void *stream) {
    PF_LAUNCH(pfann_bench_region_marker, dim3(1), dim3(64), 0, (hipStream_t)stream);
}
void pfann_prof_enable(int on) { g_prof = on != 0; }
void pfann_prof_reset(void) {
    for (auto &r : g_recs) { g_pool.push_back(r.e0); g_pool.push_back(r.e1); }
    g_recs.clear();
}
double pfann_prof_elapsed_ms(const char *tag, int64_t *count) {
    double tot = 0;
    int64_t n = 0;
    for (auto &r : g_recs) {
        if (r.tag != tag) continue;
        (void)hipEventSynchronize(r.e1);
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) { tot += ms; ++n; }
    }
    if (count) *count = n;
    return tot;
}
double pfann_prof_work(const char *tag) {
    double w = 0;
    for (auto &r : g_recs) if (r.tag == tag) w += r.work;
    return w;
}
int pfann_prof_tags(char *out, int cap) {
    std::map<std::string, int> seen;
    for (auto &r : g_recs) seen[r.tag]++;
    std::string s;
    for (auto &kv : seen) { if (!s.empty()) s += ","; s += kv.first; }
    if ((int)s.size() + 1 > cap) return -1;
    memcpy(out, s.c_str(), s.size() + 1);
    return (int)seen.size();
}

}  // extern "C"
