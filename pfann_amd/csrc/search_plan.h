// The launch plan of search_topk (search.hip): which kernels a call runs, in order, and what each launch is sized by.
// Host-only and pure: no HIP types, no allocation, fixed-size structs.  plan_search is the ONLY place a kernel variant of
// the search is chosen; search_topk executes the stages it returns, pfann_search_plan prints them (tests/test_search_plan.py
// holds them against a kernel trace of the dispatch this header replaced, profiles/search_plan/parent_launches.json).
//
// The paths, by the names used below and in DESIGN.md §4:
//   empty        n = 0: fill_empty_kernel (phase 1: bound_none_kernel).
//   small        nq <= 32, d = 64 / 128: the HBM-bound streaming kernel scan_small_kernel<D, ELT, MODE>.
//     dense      n <= CAP: counters = n, one dense pass (MODE 2), one select -- select_dense_* (canonical re-scoring) for fp32
//                rows with an fp16 copy, select_kernel otherwise -- and the fallback launch.
//     sampled    n > CAP: group-maximum pass over every R-th row (MODE 1, 2048 groups), group select = tau, full pass into
//                32 sub-lists (MODE 0), select + fallback.  fp32 rows with a copy stream the fp16 rows (ELT 2) as a pre-filter
//                and re-score; d = 128 is "folded": query preparation at the head of the sampled pass, big select + fallback in
//                one launch (select_tail_kernel) -- five launches.
//   gmax         nq > 32 with fp16 rows, k <= 128, d = 64 / 128: query-stationary group-maximum pass over every 4th (2nd,
//                every) row -- the coarsest stride that gives >= 4 k groups of >= 4 tiles --, group select, full
//                query-stationary pass into 4 S private lists per row, select with re-scoring, fallback.  Phase 1 of a
//                sharded search stops after the group select, phase 2 resumes behind it (bound_in_kernel, wave select tier).
//   ladder_f16   fp16 rows where gmax does not apply: dense coarsest level, then one thresholded level per factor R, each
//                followed by a select with re-scoring (mode 0 = threshold only); scan_f16_qres_kernel where the
//                query-stationary kernel applies, scan_f16_kernel<QT> otherwise.
//   ladder_f32   fp32 rows only: the same ladder on scan_emit_kernel + select_kernel.
// SearchShape.excl (pfann_search_topk_excl: every query row leaves one row range out): the same paths on the masked twins of
// the scans and of the fallback (the last template argument; DESIGN.md, "Self-match"), behind one excl_prep_kernel.  A masked
// row never reaches a group maximum, a threshold or a survivor list, so the selects run as they are; the dense levels
// append with a counter that starts at 0 instead of writing slot = row under a counter preset to n, because an excluded
// row must be absent, not last.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

namespace pfann {

static constexpr int CAP = 8192;         // survivor slots per query row
static constexpr int NSUB_MAX = 256;     // most sub-lists per query row (cnt is [nq][NSUB_MAX], the selects' s_off likewise)
static constexpr int SMALL_N = 4096;     // most survivors of a row the 256-thread selects take
static constexpr int WAVE_N = 256;       // most survivors (and largest k) of the wave-per-row select
static constexpr int GROUPS_MAX = 4096;  // most group maxima per row (group_max_select_kernel's LDS array)
static constexpr int QRES_S_MAX = 64;    // most db slices of a query-stationary pass
static_assert(4 * QRES_S_MAX <= NSUB_MAX, "the query-stationary full pass keeps four private lists per (row, slice)");
static_assert(64 * QRES_S_MAX <= GROUPS_MAX, "the sampled pass gives 64 groups per slice");

// Kernels launched with one ScanParams argument: X(id, instantiation as a kernel trace prints it)
#define PF_SCAN_KERNELS(X)                               \
    X(SCAN_SMALL_128_4_0, scan_small_kernel<128, 4, 0>)  \
    X(SCAN_SMALL_128_4_1, scan_small_kernel<128, 4, 1>)  \
    X(SCAN_SMALL_128_4_2, scan_small_kernel<128, 4, 2>)  \
    X(SCAN_SMALL_128_2_0, scan_small_kernel<128, 2, 0>)  \
    X(SCAN_SMALL_128_2_1, scan_small_kernel<128, 2, 1>)  \
    X(SCAN_SMALL_128_2_2, scan_small_kernel<128, 2, 2>)  \
    X(SCAN_SMALL_64_4_0, scan_small_kernel<64, 4, 0>)    \
    X(SCAN_SMALL_64_4_1, scan_small_kernel<64, 4, 1>)    \
    X(SCAN_SMALL_64_4_2, scan_small_kernel<64, 4, 2>)    \
    X(SCAN_SMALL_64_2_0, scan_small_kernel<64, 2, 0>)    \
    X(SCAN_SMALL_64_2_1, scan_small_kernel<64, 2, 1>)    \
    X(SCAN_SMALL_64_2_2, scan_small_kernel<64, 2, 2>)    \
    X(SCAN_EMIT_32, scan_emit_kernel<32, 128, 32, 32, 1>)     \
    X(SCAN_EMIT_64, scan_emit_kernel<64, 64, 32, 32, 1>)      \
    X(SCAN_EMIT_128_QT4, scan_emit_kernel<128, 128, 64, 64, 4>) \
    X(SCAN_EMIT_128_QT1, scan_emit_kernel<128, 128, 64, 64, 1>)
#define PF_SCAN_F16_KERNELS(X)                                         \
    X(SCAN_F16_QT4, scan_f16_kernel<4>)                                \
    X(SCAN_F16_QT1, scan_f16_kernel<1>)                                \
    X(QRES_GMAX_8_NBUF3, scan_f16_qres_kernel<8, true, 128, 3>)        \
    X(QRES_GMAX_8, scan_f16_qres_kernel<8, true, 128, 2>)              \
    X(QRES_GMAX_4, scan_f16_qres_kernel<4, true, 128, 2>)              \
    X(QRES_8_DBR64_NBUF3, scan_f16_qres_kernel<8, false, 64, 3>)       \
    X(QRES_8_DBR64, scan_f16_qres_kernel<8, false, 64, 2>)             \
    X(QRES_8, scan_f16_qres_kernel<8, false, 128, 2>)                  \
    X(QRES_4, scan_f16_qres_kernel<4, false, 128, 2>)
// every other kernel of the search (each has its own argument list: search.hip launch_stage, search_f16.hip launch_stage_f16)
#define PF_AUX_KERNELS(X)                                       \
    X(FILL_EMPTY, fill_empty_kernel)                            \
    X(BOUND_NONE, bound_none_kernel)                            \
    X(BOUND_IN, bound_in_kernel)                                \
    X(FILL_INT, fill_int_kernel)                                \
    X(FILL_INT2, fill_int2_kernel)                              \
    X(Q_PREP, q_prep_kernel)                                    \
    X(GROUP_SELECT, group_max_select_kernel)                    \
    X(GROUP_SELECT_WAVE_8, group_max_select_wave_kernel<8>)     \
    X(GROUP_SELECT_WAVE_16, group_max_select_wave_kernel<16>)   \
    X(SELECT, select_kernel)                                    \
    X(SELECT_RESCORE_SMALL, select_rescore_small_kernel)        \
    X(SELECT_RESCORE, select_rescore_kernel)                    \
    X(SELECT_RESCORE_WAVE, select_rescore_wave_kernel)          \
    X(SELECT_RESCORE_SMALL_LIST, select_rescore_small_list_kernel) \
    X(SELECT_RESCORE_LIST, select_rescore_list_kernel)          \
    X(SELECT_DENSE_SMALL, select_dense_small_kernel)            \
    X(SELECT_DENSE, select_dense_kernel)                        \
    X(SELECT_TAIL_4, select_tail_kernel<4>)                     \
    X(SELECT_TAIL_2, select_tail_kernel<2>)                     \
    X(FALLBACK_4, topk_fallback_kernel<4>)                      \
    X(FALLBACK_2, topk_fallback_kernel<2>)

// The masked twins (SearchShape.excl), in lists of their own and in the order of their unmasked kernels: the three lists
// above are, name for name, the kernels of the recorded trace of the unmasked search (tests/test_search_plan.py).  The twin
// of scan kernel K_x is K_x_EXCL = K_x + (K_SCAN_SMALL_128_4_0_EXCL - K_SCAN_SMALL_128_4_0): excl_twin().
#define PF_SCAN_EXCL_KERNELS(Y)                                     \
    Y(SCAN_SMALL_128_4_0_EXCL, scan_small_kernel<128, 4, 0, true>)  \
    Y(SCAN_SMALL_128_4_1_EXCL, scan_small_kernel<128, 4, 1, true>)  \
    Y(SCAN_SMALL_128_4_2_EXCL, scan_small_kernel<128, 4, 2, true>)  \
    Y(SCAN_SMALL_128_2_0_EXCL, scan_small_kernel<128, 2, 0, true>)  \
    Y(SCAN_SMALL_128_2_1_EXCL, scan_small_kernel<128, 2, 1, true>)  \
    Y(SCAN_SMALL_128_2_2_EXCL, scan_small_kernel<128, 2, 2, true>)  \
    Y(SCAN_SMALL_64_4_0_EXCL, scan_small_kernel<64, 4, 0, true>)    \
    Y(SCAN_SMALL_64_4_1_EXCL, scan_small_kernel<64, 4, 1, true>)    \
    Y(SCAN_SMALL_64_4_2_EXCL, scan_small_kernel<64, 4, 2, true>)    \
    Y(SCAN_SMALL_64_2_0_EXCL, scan_small_kernel<64, 2, 0, true>)    \
    Y(SCAN_SMALL_64_2_1_EXCL, scan_small_kernel<64, 2, 1, true>)    \
    Y(SCAN_SMALL_64_2_2_EXCL, scan_small_kernel<64, 2, 2, true>)    \
    Y(SCAN_EMIT_32_EXCL, scan_emit_kernel<32, 128, 32, 32, 1, true>)       \
    Y(SCAN_EMIT_64_EXCL, scan_emit_kernel<64, 64, 32, 32, 1, true>)        \
    Y(SCAN_EMIT_128_QT4_EXCL, scan_emit_kernel<128, 128, 64, 64, 4, true>) \
    Y(SCAN_EMIT_128_QT1_EXCL, scan_emit_kernel<128, 128, 64, 64, 1, true>)
#define PF_SCAN_F16_EXCL_KERNELS(Y)                                            \
    Y(SCAN_F16_QT4_EXCL, scan_f16_kernel<4, true>)                             \
    Y(SCAN_F16_QT1_EXCL, scan_f16_kernel<1, true>)                             \
    Y(QRES_GMAX_8_NBUF3_EXCL, scan_f16_qres_kernel<8, true, 128, 3, true>)     \
    Y(QRES_GMAX_8_EXCL, scan_f16_qres_kernel<8, true, 128, 2, true>)           \
    Y(QRES_GMAX_4_EXCL, scan_f16_qres_kernel<4, true, 128, 2, true>)           \
    Y(QRES_8_DBR64_NBUF3_EXCL, scan_f16_qres_kernel<8, false, 64, 3, true>)    \
    Y(QRES_8_DBR64_EXCL, scan_f16_qres_kernel<8, false, 64, 2, true>)          \
    Y(QRES_8_EXCL, scan_f16_qres_kernel<8, false, 128, 2, true>)               \
    Y(QRES_4_EXCL, scan_f16_qres_kernel<4, false, 128, 2, true>)
#define PF_AUX_EXCL_KERNELS(Y)                                  \
    Y(EXCL_PREP, excl_prep_kernel)                              \
    Y(SELECT_TAIL_4_EXCL, select_tail_kernel<4, true>)          \
    Y(SELECT_TAIL_2_EXCL, select_tail_kernel<2, true>)          \
    Y(FALLBACK_4_EXCL, topk_fallback_kernel<4, true>)           \
    Y(FALLBACK_2_EXCL, topk_fallback_kernel<2, true>)

#define PF_ALL_SEARCH_KERNELS(X) \
    PF_SCAN_KERNELS(X) PF_SCAN_F16_KERNELS(X) PF_AUX_KERNELS(X) PF_SCAN_EXCL_KERNELS(X) PF_SCAN_F16_EXCL_KERNELS(X) PF_AUX_EXCL_KERNELS(X)
enum SearchKernel {
#define X(id, ...) K_##id,
    PF_ALL_SEARCH_KERNELS(X)
#undef X
    K_COUNT
};
static_assert(K_QRES_4_EXCL - K_QRES_4 == K_SCAN_SMALL_128_4_0_EXCL - K_SCAN_SMALL_128_4_0, "the masked scans mirror the scan lists");
// the masked twin of a scan kernel of the first two lists
inline int excl_twin(int scan_kernel) { return scan_kernel + (K_SCAN_SMALL_128_4_0_EXCL - K_SCAN_SMALL_128_4_0); }
inline const char *search_kernel_name(int kernel) {
    static const char *const names[K_COUNT] = {
#define X(id, ...) #__VA_ARGS__,
        PF_ALL_SEARCH_KERNELS(X)
#undef X
    };
    return kernel >= 0 && kernel < K_COUNT ? names[kernel] : "?";
}

enum { STORE_F32 = 0, STORE_F32_COPY = 1, STORE_F16 = 2 };       // fp32 rows only / fp32 rows + their fp16 copy / fp16 rows only
struct SearchShape {
    int64_t n = 0;           // rows of the shard
    int d = 0;
    int64_t nq = 0;          // query rows of the call (<= 16384: pfann_search_topk walks larger batches in chunks)
    int k = 0;
    int storage = STORE_F32; // what search_topk is GIVEN: the copy counts only while the pre-filter is on
    int phase = 0;           // 0 whole search, 1 bound only, 2 bounded full pass
    bool resume = false;     // phase 2 behind a phase 1 of the same (q, nq, k): thresholds and fp16 query rows are in place
    bool has_lb = false;     // phase 2 was given the global bound
    int mtop = 1;            // phase 1: bounds per query row
    bool excl = false;       // phase 0 only: every query row leaves one row range out (pfann_search_topk_excl)
};

// Every A/B switch of the search.  Set (to anything) = on; read once per process (search_tuning()).
//   switch                      field                   effect                                                   record under profiles/
//   PFANN_SMALL_F32             small_f32               small sampled: stream the fp32 rows, MFMA scores final     r4/NOTES.md
//   PFANN_NO_FOLDED_SMALL       no_folded_small         small sampled, d = 128: one launch per stage (8, not 5)    r3/NOTES.md
//   PFANN_NO_GMAX               no_gmax                 batched fp16: the survivor ladder instead of gmax          r4/NOTES.md
//   PFANN_QRES_MIN_NQ=<rows>    qres_min_nq (33)        fewest query rows of the query-stationary kernels          r6/scan_mid_before.txt
//   PFANN_GMAX_S=<slices>       gmax_s (0 = computed)   slices of the sampled gmax pass, clamped to QRES_S_MAX     r4/sharded_scan_model.txt
//   PFANN_NO_QRES               no_qres                 full / ladder passes on scan_f16_kernel                    r4/NOTES.md
//   PFANN_SCAN_DBR128           scan_dbr128             full pass on 128-row db tiles (not 64)                     r6/NOTES.md
//   PFANN_SCAN_S=<slices>       scan_s (0 = computed)   slices of the query-stationary full / ladder pass,         r6/NOTES.md
//                                                       clamped to QRES_S_MAX (4 S private lists <= NSUB_MAX)
//   PFANN_SCAN_NBUF3            scan_nbuf3              full pass: three tile buffers whatever the grid            r6/NOTES.md
//   PFANN_NO_WAVE_SELECT        no_wave_select          phase 2: no wave-per-row select tier                       r4/NOTES.md
//   PFANN_NO_WAVE_GROUP_SELECT  no_wave_group_select    group select: the workgroup form for every G               r5/NOTES.md
struct SearchTuning {
    bool small_f32 = false, no_folded_small = false, no_gmax = false, no_qres = false, scan_dbr128 = false, scan_nbuf3 = false,
         no_wave_select = false, no_wave_group_select = false;
    int64_t qres_min_nq = 33;
    int gmax_s = 0, scan_s = 0;
};
inline SearchTuning search_tuning_from_env() {
    SearchTuning t;
    t.small_f32 = getenv("PFANN_SMALL_F32") != nullptr;
    t.no_folded_small = getenv("PFANN_NO_FOLDED_SMALL") != nullptr;
    t.no_gmax = getenv("PFANN_NO_GMAX") != nullptr;
    t.no_qres = getenv("PFANN_NO_QRES") != nullptr;
    t.scan_dbr128 = getenv("PFANN_SCAN_DBR128") != nullptr;
    t.scan_nbuf3 = getenv("PFANN_SCAN_NBUF3") != nullptr;
    t.no_wave_select = getenv("PFANN_NO_WAVE_SELECT") != nullptr;
    t.no_wave_group_select = getenv("PFANN_NO_WAVE_GROUP_SELECT") != nullptr;
    if (const char *v = getenv("PFANN_QRES_MIN_NQ")) t.qres_min_nq = atoll(v);
    if (const char *v = getenv("PFANN_GMAX_S")) t.gmax_s = atoi(v);
    if (const char *v = getenv("PFANN_SCAN_S")) t.scan_s = atoi(v);
    return t;
}
inline const SearchTuning &search_tuning() {
    static const SearchTuning t = search_tuning_from_env();
    return t;
}

enum { THR_NONE = 0, THR_EXACT = 1, THR_ADJ = 2 };               // ScanParams.thr: nullptr (dense) / ws.thr / ws.thr_adj
struct SearchStage {
    int kernel = 0;                      // SearchKernel
    unsigned grid = 0, block = 256, lds = 0;       // workgroups, threads, dynamic LDS bytes
    const char *tag = nullptr;           // ProfScope tag (nullptr: none) ...
    int scope = 1;                       // ... which brackets this and the next scope - 1 stages
    double work = 0.0;                   // ... and its work figure
    bool zero_cnt = false;               // thresholded counter initialisation: cnt[0 .. nq) = 0 before the launch
    bool zero_overflow = false;          // overflow[1..2] = 0 before the launch
    // scans
    int elt = 4;                         // bytes per element of the rows (and query rows) the scan reads
    int64_t stride = 1, nrows = 0;       // every stride-th row; rows scanned = ceil(n / stride)
    int n_tiles_m = 1, nsub = 1;         // 128-row query tiles; ScanParams.nsub (slices S / sub-lists)
    int thr = THR_NONE;
    bool gmax = false, fold_prep = false;          // group-maximum pass; with the query preparation at its head
    // group select
    int G = 0, ncnt = 0;                 // group maxima per row; counters per row it zeroes
    bool with_eps = false, topm = false, zero_me = false;
    float margin = 0.f, margin_out = 0.f;
    // selects
    int mode = 1, rescore = 0;           // 0: threshold only, 1: results; exact re-scoring
    bool few_survivors = false;
    int fb_elt = 4;                      // fallback / tail: element size of the rows it streams
    int fill = 0;                        // FILL_INT*: dense counter initialisation, cnt[0 .. nq) = fill
    bool excl = false;                   // a masked scan / fallback / tail: reads the row ranges excl_prep_kernel left
};

enum { QPREP_NONE = 0, QPREP_LAUNCH = 1, QPREP_FOLDED = 2 };
enum { FB_NONE = 0, FB_LAUNCH = 1, FB_TAIL = 2 };
enum {
    PLAN_OK = 0, PLAN_ERR_K, PLAN_ERR_D4, PLAN_ERR_ROWS, PLAN_ERR_D1024, PLAN_ERR_DENSE_CAP, PLAN_ERR_STRIDE_WINDOW, PLAN_ERR_GROUPS,
    PLAN_ERR_STAGES, PLAN_ERR_EXCL_PHASE
};
inline const char *plan_error_name(int e) {
    static const char *const names[] = {"none", "k", "d%4", "n>=2^32", "d>1024", "dense>CAP", "stride_window", "groups", "stages", "excl_phase"};
    return e >= 0 && e <= PLAN_ERR_EXCL_PHASE ? names[e] : "?";
}

struct SearchPlan {
    // ladders: n < 2^32 and R = 2 give at most 21 levels of (fill or none) + scan + two selects
    static constexpr int MAX_STAGES = 96;
    int n_stages = 0;
    SearchStage stages[MAX_STAGES];
    int error = PLAN_OK;
    char error_msg[128] = {0};
    const char *path = "none";           // nq <= 0: nothing to do
    int q_prep = QPREP_NONE, fallback = FB_NONE;
    bool need_qh = false;                // the call needs ws.qh sized for nq x d halves
    bool canonical_scores = false;       // every returned score is the canon_part / canon_sum one
    bool leaves_bound = false;           // phase 1 left thresholds a phase 2 may resume behind
    bool consumes_bound = false;         // phase 2 resumed with the global bound
    int G = 0;                           // gmax: group maxima per row
};

namespace plan_detail {
inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int sample_ratio(int k) { return k <= 128 ? 16 : (k <= 512 ? 4 : 2); }    // expected survivors of a level ~ R k per row

// The query-stationary kernel addresses a db tile with 32-bit chunk offsets against a per-tile descriptor of 0x7FFFFFF0
// bytes: the last row of a strided 128-row tile must lie inside it (stride <= ~66 k, i.e. shards below ~268 M rows for the
// ladder's largest stride); beyond that the plan takes the generic kernel / the survivor ladder.
inline bool qres_stride_ok(int64_t stride, int d) { return 127ll * stride * (2ll * d) + 2ll * d <= 0x7FFFFFF0ll; }
// ... and where it applies at all.  (qres_min_nq was 1024 up to round 5: between the small path and 1024 rows the ladder
// ran on the generic kernel, 1.1-1.4 ms whatever the row count, profiles/r6/scan_mid_before.txt.)
inline bool qres_ok(const SearchShape &sh, const SearchTuning &t, int64_t db_tiles, int64_t stride) {
    return (sh.d == 128 || sh.d == 64) && sh.nq >= t.qres_min_nq && db_tiles >= 16 && qres_stride_ok(stride, sh.d);
}

struct Builder {
    SearchPlan &p;
    bool excl = false;
    // a scan of the first two lists: its masked twin when the shape excludes rows
    SearchStage &add_scan(int kernel, int64_t grid, const char *tag, double work) {
        SearchStage &st = add(excl ? excl_twin(kernel) : kernel, grid, 256, 0, tag, work);
        st.excl = excl;
        return st;
    }
    SearchStage &add(int kernel, int64_t grid, unsigned block = 256, unsigned lds = 0, const char *tag = nullptr, double work = 0.0) {
        if (p.n_stages == SearchPlan::MAX_STAGES) { fail(PLAN_ERR_STAGES, "search plan: more than %lld stages", SearchPlan::MAX_STAGES, 0); --p.n_stages; }
        SearchStage &st = p.stages[p.n_stages++];
        st = SearchStage();
        st.kernel = kernel; st.grid = (unsigned)grid; st.block = block; st.lds = lds; st.tag = tag; st.work = work;
        return st;
    }
    void fail(int err, const char *fmt, long long a, long long b) {
        if (p.error != PLAN_OK) return;
        p.error = err;
        snprintf(p.error_msg, sizeof(p.error_msg), fmt, a, b);
    }
};
}  // namespace plan_detail

inline SearchPlan plan_search(const SearchShape &sh, const SearchTuning &t) {
    using namespace plan_detail;
    SearchPlan plan;
    Builder b{plan};
    const int64_t n = sh.n, nq = sh.nq;
    const int d = sh.d, k = sh.k;
    if (nq <= 0) return plan;
    if (k < 1 || k > 1024) { b.fail(PLAN_ERR_K, "search_topk: k=%lld outside 1..1024", k, 0); return plan; }
    if (d % 4 != 0) { b.fail(PLAN_ERR_D4, "search_topk: d=%lld must be a multiple of 4", d, 0); return plan; }
    if (n >= (1ll << 32)) { b.fail(PLAN_ERR_ROWS, "search_topk: shard rows %lld >= 2^32", n, 0); return plan; }
    if (sh.excl && sh.phase != 0) { b.fail(PLAN_ERR_EXCL_PHASE, "search_topk: row exclusion with phase %lld (the sharded halves have none)", sh.phase, 0); return plan; }
    b.excl = sh.excl && n > 0;
    auto no_bound = [&]() { b.add(K_BOUND_NONE, cdiv64(nq * sh.mtop, 256)); };     // phase 1 without a sampled threshold
    if (n == 0) {
        plan.path = "empty";
        if (sh.phase == 1) no_bound();
        else b.add(K_FILL_EMPTY, cdiv64(nq * k, 256));
        return plan;
    }
    // the fallback keeps a query row in LDS (standalone launch or inside the tail launch)
    if (d > 1024) { b.fail(PLAN_ERR_D1024, "search_topk: d=%lld > 1024", d, 0); return plan; }
    const bool half_only = sh.storage == STORE_F16, has_copy = sh.storage == STORE_F32_COPY;
    // the ranges in row space, clipped to the shard, and their union per 128-row query tile (the scans' per-tile test)
    if (b.excl) b.add(K_EXCL_PREP, cdiv64(nq, 128), 128);
    const bool small = nq <= 32 && (d == 128 || d == 64);
    // <= 32 query rows against fp32 rows with an fp16 copy: stream the copy (half the bytes) as a pre-filter and re-score
    const bool small_pre = small && has_copy && n > CAP && !t.small_f32;
    const bool folded = small && n > CAP && d == 128 && !t.no_folded_small;
    plan.need_qh = half_only || (has_copy && nq > 32) || small_pre;
    if (plan.need_qh) {
        if (folded && sh.phase != 1) plan.q_prep = QPREP_FOLDED;
        else if (!sh.resume) { plan.q_prep = QPREP_LAUNCH; b.add(K_Q_PREP, cdiv64(nq, 4)); }
    }
    auto fallback = [&]() {
        plan.fallback = FB_LAUNCH;
        const int kern = half_only ? K_FALLBACK_2 : K_FALLBACK_4;
        b.add(b.excl ? kern + (K_FALLBACK_4_EXCL - K_FALLBACK_4) : kern, nq, 256, 0, "topk_fallback").excl = b.excl;
    };
    auto group_select = [&](int G, int ncnt, bool with_eps, float margin) -> SearchStage & {
        if (G < 1 || G > GROUPS_MAX) b.fail(PLAN_ERR_GROUPS, "group select: %lld groups (the kernel's LDS array holds %lld)", G, GROUPS_MAX);
        const bool wave = !t.no_wave_group_select;
        SearchStage &st = wave && G <= 64 * 8    ? b.add(K_GROUP_SELECT_WAVE_8, cdiv64(nq, 4), 256, 0, "topk_group_select")
                          : wave && G <= 64 * 16 ? b.add(K_GROUP_SELECT_WAVE_16, cdiv64(nq, 4), 256, 0, "topk_group_select")
                                                 : b.add(K_GROUP_SELECT, nq, 256, 0, "topk_group_select");
        st.G = G; st.ncnt = ncnt; st.with_eps = with_eps; st.margin = margin;
        return st;
    };
    // select with re-scoring (rescore = 0: the keys' scores are final): the 256-thread select, then the 1024-thread one for
    // the rows it left; few_survivors (phase 2 behind the global bound: a few dozen per row): a wave-per-row tier first
    auto select_rescore = [&](int mode, int nsub, int rescore, bool few) {
        const char *tag = rescore ? "topk_select_rescore" : "topk_select_radix";
        const int first = plan.n_stages;
        if (few && mode == 1 && nsub <= NSUB_MAX && k <= WAVE_N && !t.no_wave_select) {
            b.add(K_SELECT_RESCORE_WAVE, cdiv64(nq, 4), 256, 0, tag);
            b.add(K_SELECT_RESCORE_SMALL_LIST, nq < 2048 ? nq : 2048);
            b.add(K_SELECT_RESCORE_LIST, nq < 512 ? nq : 512, 1024, CAP * 8);
        } else {
            b.add(K_SELECT_RESCORE_SMALL, nq, 256, 0, tag);
            b.add(K_SELECT_RESCORE, nq, 1024, CAP * 8);
        }
        plan.stages[first].scope = plan.n_stages - first;
        plan.stages[first].zero_overflow = true;
        for (int i = first; i < plan.n_stages; ++i) {
            SearchStage &st = plan.stages[i];
            st.mode = mode; st.nsub = nsub; st.rescore = rescore; st.few_survivors = few;
        }
    };

    if (small) {
        if (sh.phase == 1) { plan.path = "small"; no_bound(); return plan; }
        const int elt = (half_only || small_pre) ? 2 : 4;
        const int k0 = (d == 128 ? K_SCAN_SMALL_128_4_0 : K_SCAN_SMALL_64_4_0) + (elt == 2 ? 3 : 0);      // + MODE
        const double bytes_per_row = (double)d * elt;
        if (n <= CAP) {
            plan.path = "small_dense";
            b.add(K_FILL_INT, cdiv64(nq, 256)).fill = b.excl ? 0 : (int)n;        // (masked: the dense pass appends)
            SearchStage &sc = b.add_scan(k0 + 2, cdiv64(n, 128) < 512 ? cdiv64(n, 128) : 512, "scan_topk", n * bytes_per_row);
            sc.elt = elt; sc.nrows = n;
            if (has_copy) {
                // the MFMA scores are a pre-filter, the select re-scores in the canonical order
                plan.canonical_scores = true;
                // (masked: the rows that remain may be SMALL_N or fewer although n is not -- each select leaves the other's rows)
                // With both, the small select counts the rows it leaves in overflow[1]; the dense select does not read it, but
                // the counter is zeroed first all the same, so that it holds this call's count and never a sum over calls.
                if (n <= SMALL_N || b.excl)
                    b.add(K_SELECT_DENSE_SMALL, nq, 256, 0, "topk_select_rescore").zero_overflow = b.excl && n > SMALL_N;
                if (n > SMALL_N) b.add(K_SELECT_DENSE, nq, 1024, CAP * 8, "topk_select_rescore");
            } else {
                b.add(K_SELECT, nq, 1024, CAP * 8, "topk_select");
            }
            fallback();
            return plan;
        }
        plan.path = folded ? "small_sampled_folded" : "small_sampled";
        plan.canonical_scores = small_pre;
        const int GRID = 512, W = GRID * 4;            // persistent: 2 workgroups per CU; W groups in the sampled pass
        int64_t R = sample_ratio(k);
        if (R > n / W) R = n / W;                      // at least one sampled row per group (n > CAP = 4 W)
        SearchStage &sm = b.add_scan(k0 + 1, GRID, "scan_topk_sample", cdiv64(n, R) * bytes_per_row);
        sm.elt = elt; sm.stride = R; sm.nrows = cdiv64(n, R); sm.gmax = true; sm.fold_prep = folded && elt == 2;
        group_select(W, 32, small_pre, small_pre ? 2.f : 0.f).zero_me = folded;
        SearchStage &sc = b.add_scan(k0, GRID, "scan_topk", n * bytes_per_row);
        sc.elt = elt; sc.nrows = n; sc.nsub = 32; sc.thr = small_pre ? THR_ADJ : THR_EXACT;
        if (!folded) {
            select_rescore(1, 32, small_pre ? 1 : 0, false);
            fallback();
            return plan;
        }
        // the 256-thread select alone (overflow[1] was zeroed by the group select), then the rows it left and, behind them,
        // the exact fallback of flagged rows -- both normally idle -- in one launch
        SearchStage &s1 = b.add(K_SELECT_RESCORE_SMALL, nq, 256, 0, small_pre ? "topk_select_rescore" : "topk_select_radix");
        s1.nsub = 32; s1.rescore = small_pre ? 1 : 0;
        const int tail = half_only ? K_SELECT_TAIL_2 : K_SELECT_TAIL_4;
        SearchStage &tl = b.add(b.excl ? tail + (K_SELECT_TAIL_4_EXCL - K_SELECT_TAIL_4) : tail, nq, 1024, CAP * 8, "topk_select_tail");
        tl.excl = b.excl;
        tl.nsub = 32; tl.rescore = s1.rescore; tl.fb_elt = half_only ? 2 : 4;
        plan.fallback = FB_TAIL;
        return plan;
    }

    // ---- ladders: the shard is scanned at strides R^L .. R, 1; the coarsest level keeps everything and is fully sorted per
    // query row: <= 4096 rows (it still holds > 4096 / R >= k rows).  (R = 8 and 4 were measured for the batched path too:
    // more passes and selects cost more than the shorter survivor lists save.)
    const int R = sample_ratio(k);
    int levels = 0;
    int64_t stride = 1;
    while (cdiv64(n, stride) > 4096) { stride *= R; ++levels; }
    const int n_tiles_m = (int)cdiv64(nq, 128);
    auto dense_or_zero = [&](int fill_kernel, int64_t nrows, bool dense) {      // counters of a scan level; true = zero_cnt
        if (!dense) return true;
        if (nrows > CAP) b.fail(PLAN_ERR_DENSE_CAP, "scan: dense level with %lld rows > %lld", nrows, CAP);
        b.add(fill_kernel, cdiv64(nq, 256)).fill = b.excl ? 0 : (int)nrows;       // (masked: the dense level appends)
        return false;
    };

    if (plan.need_qh) {
        // ---- fp16 MFMA scans.  fp32 rows with a copy: pre-filter with a rigorous margin + exact re-scoring; fp16 rows only:
        // eps = 0, the s16 scores are the result
        const int rescore = half_only ? 0 : 1;
        plan.canonical_scores = !half_only && sh.phase != 1;
        // one level: counters, scan; returns the sub-lists per row the select that follows reads
        auto scan_f16 = [&](int64_t st_, bool dense) -> int {
            const int64_t nrows = cdiv64(n, st_), db_tiles = cdiv64(nrows, 128);
            const bool zero = dense_or_zero(K_FILL_INT2, nrows, dense);
            const char *tag = st_ == 1 ? "scan_topk_f16" : "scan_topk_f16_sample";
            const double work = 2.0 * (double)nq * nrows * d;
            SearchStage *sc;
            int nsub_out = 1;
            if (!dense && !t.no_qres && qres_ok(sh, t, db_tiles, st_)) {
                // S interleaved db slices: about four rounds of the 512 resident workgroups, sub-lists of >= 256; with few
                // query tiles up to 64 slices (sub-lists of 128: a row's ~330 survivors spread over them), so that one query
                // tile still becomes 64 workgroups
                const int s_max = n_tiles_m * 32 < 768 ? QRES_S_MAX : 32;
                int S = 2048 / n_tiles_m;
                S = S < 1 ? 1 : (S > s_max ? s_max : S);
                // 64-row db tiles, three workgroups per CU (168 VGPRs) for the full pass: 2.97 -> 2.86 ms on the bench's
                // 9728 x 1 M pass (four per CU would need <= 128 VGPRs: 35 spilled)
                const bool dbr64 = d == 128 && !t.scan_dbr128 && st_ == 1;
                if (dbr64) {
                    // whole rounds of the 768 resident workgroups: 76 query tiles x 26 slices are 2.57 rounds; 30 slices
                    // (2.97 rounds) run the pass in 2.77 instead of 2.91 ms (20: 2.82, 32: 2.97)
                    const int64_t slots = 768, rounds = (n_tiles_m * (int64_t)S + slots - 1) / slots;
                    const int64_t s2 = rounds * slots / n_tiles_m;
                    if (s2 >= S && s2 <= s_max) S = (int)s2;
                }
                if (t.scan_s > 0) S = t.scan_s > QRES_S_MAX ? QRES_S_MAX : t.scan_s;
                if (S > db_tiles) S = (int)db_tiles;
                // less than one round of the resident slots: nobody covers a tile's round trip -> three tile buffers
                const int kern = dbr64 ? ((n_tiles_m * S < 768 || t.scan_nbuf3) ? K_QRES_8_DBR64_NBUF3 : K_QRES_8_DBR64)
                                       : (d == 128 ? K_QRES_8 : K_QRES_4);
                sc = &b.add_scan(kern, (int64_t)n_tiles_m * S, tag, work);
                sc->nsub = S;
                nsub_out = 4 * S;                  // four private lists per (row, slice), one per owner lane
            } else if (db_tiles * cdiv64(n_tiles_m, 4) >= 4096) {
                // long runs of query tiles per block only when the grid still fills the chip many times over
                sc = &b.add_scan(K_SCAN_F16_QT4, db_tiles * cdiv64(n_tiles_m, 4), tag, work);
            } else {
                sc = &b.add_scan(K_SCAN_F16_QT1, db_tiles * n_tiles_m, tag, work);
            }
            sc->elt = 2; sc->stride = st_; sc->nrows = nrows; sc->n_tiles_m = n_tiles_m; sc->zero_cnt = zero;
            sc->thr = dense ? THR_NONE : THR_ADJ;
            return nsub_out;
        };
        // gmax: one group-maximum pass over every gs-th row instead of the dense + 1/16 survivor levels; shards too small to
        // give 4 k groups of >= 4 tiles at that stride (the 1/4 and 1/8 shards of a multi-GPU job) are sampled more densely
        int gs_found = 0, S_found = 0;
        if (k <= 128 && !t.no_gmax) {
            for (int64_t gs = 4; gs >= 1 && !gs_found; gs >>= 1) {
                const int64_t db_tiles = cdiv64(cdiv64(n, gs), 128);
                if (!qres_ok(sh, t, db_tiles, gs)) continue;
                // few query tiles (the middle of the batch curve): up to 64 slices, so that one tile still becomes 64 workgroups
                const int s_max = n_tiles_m * 32 < 512 ? QRES_S_MAX : 32;
                int S = 2048 / n_tiles_m;
                S = S < 1 ? 1 : (S > s_max ? s_max : S);
                // no more groups than the threshold needs: 5 k of them (64 per slice) give the k-th best group maximum the
                // quality 1000-1600 did while the group select, whose cost is the number of groups, halves
                // (profiles/r4/sharded_scan_model.txt) ... but never fewer slices than fill the chip twice, and whole rounds
                // of the 512 resident workgroups: 76 query tiles x 8 slices are 1.2 rounds, x 14 are 2.08, x 13 are 1.93
                const int a = (5 * k + 63) / 64, c = 1024 / n_tiles_m;
                const int s_cap = a > 8 ? (a > c ? a : c) : (8 > c ? 8 : c);
                if (S > s_cap) S = s_cap;
                if (t.gmax_s > 0) S = t.gmax_s > QRES_S_MAX ? QRES_S_MAX : t.gmax_s;
                if (S > db_tiles) S = (int)db_tiles;
                // one group per (slice, row position in the 128-row tile up to the lane half); >= 4 tiles per slice
                if (S * 64 < 4 * k || db_tiles < 4 * (int64_t)S) continue;
                gs_found = (int)gs; S_found = S;
            }
        }
        if (sh.resume || gs_found) {
            plan.path = "gmax";
            plan.G = S_found * 64;
            if (!sh.resume) {
                const int64_t nrows = cdiv64(n, gs_found);
                // at most one workgroup per CU: nobody covers a tile's round trip -> three tile buffers (96 KB)
                const int kern = d == 128 ? (n_tiles_m * S_found <= 256 ? K_QRES_GMAX_8_NBUF3 : K_QRES_GMAX_8) : K_QRES_GMAX_4;
                SearchStage &sm = b.add_scan(kern, (int64_t)n_tiles_m * S_found, "scan_topk_f16_sample", 2.0 * (double)nq * nrows * d);
                sm.elt = 2; sm.stride = gs_found; sm.nrows = nrows; sm.n_tiles_m = n_tiles_m; sm.nsub = S_found; sm.gmax = true;
                SearchStage &g = group_select(plan.G, 0, true, rescore ? 2.f : 0.f);
                g.topm = sh.phase == 1; g.margin_out = rescore ? 1.f : 0.f;
            }
            if (sh.phase == 1) { plan.leaves_bound = true; plan.canonical_scores = false; return plan; }
            const bool bounded = sh.resume && sh.has_lb;
            if (bounded) {
                // rows of this shard whose true score reaches the global bound have s16 >= lb - eps
                b.add(K_BOUND_IN, cdiv64(nq, 256)).margin = rescore ? 1.f : 0.f;
                plan.consumes_bound = true;
            }
            const int nsub = scan_f16(1, false);
            select_rescore(1, nsub, rescore, bounded);
            fallback();
            return plan;
        }
        plan.path = "ladder_f16";
        if (sh.phase == 1) { no_bound(); plan.canonical_scores = false; return plan; }
        for (int lev = levels; lev >= 0; --lev) {
            const int nsub = scan_f16(stride, lev == levels);          // the coarsest level (levels = 0: the only one) is dense
            select_rescore(lev == 0 ? 1 : 0, nsub, rescore, false);
            stride /= R;
        }
        fallback();
        return plan;
    }

    // ---- fp32 rows only: fp32 MFMA tiles, one survivor list per row, MFMA-order scores
    plan.path = "ladder_f32";
    if (sh.phase == 1) { no_bound(); return plan; }
    for (int lev = levels; lev >= 0; --lev) {
        const int64_t nrows = cdiv64(n, stride), db_tiles = cdiv64(nrows, 128);
        // one buffer window per 32-row sub-tile: 32 strided rows must span less than the 2 GB an offset can address
        if ((unsigned long long)31 * stride * d * 4ull >= 0x7FFF0000ull)
            b.fail(PLAN_ERR_STRIDE_WINDOW, "scan: sampling stride %lld x d %lld exceeds the 2 GB window of a 32-row sub-tile", stride, d);
        const bool dense = lev == levels;
        const bool zero = dense_or_zero(K_FILL_INT, nrows, dense);
        const char *tag = stride == 1 ? "scan_topk" : "scan_topk_sample";
        const double work = 2.0 * (double)nq * nrows * d;
        SearchStage *sc;
        if (nq <= 32) sc = &b.add_scan(K_SCAN_EMIT_32, db_tiles, tag, work);
        else if (nq <= 64) sc = &b.add_scan(K_SCAN_EMIT_64, cdiv64(nrows, 64), tag, work);
        else if (db_tiles * cdiv64(n_tiles_m, 4) >= 4096) sc = &b.add_scan(K_SCAN_EMIT_128_QT4, db_tiles * cdiv64(n_tiles_m, 4), tag, work);
        else sc = &b.add_scan(K_SCAN_EMIT_128_QT1, db_tiles * n_tiles_m, tag, work);
        sc->stride = stride; sc->nrows = nrows; sc->n_tiles_m = nq <= 64 ? 1 : n_tiles_m; sc->zero_cnt = zero;
        sc->thr = dense ? THR_NONE : THR_EXACT;
        b.add(K_SELECT, nq, 1024, CAP * 8, "topk_select").mode = lev == 0 ? 1 : 0;
        stride /= R;
    }
    fallback();
    return plan;
}

// One line per stage -- kernel, grid, block, dynamic LDS bytes --, then one line of flags.  Returns the length of the whole
// text (snprintf's convention: it is cut to len - 1 characters).
inline int print_search_plan(const SearchPlan &p, char *buf, int len) {
    int at = 0;
    auto put = [&](const char *fmt, auto... a) {
        const int room = len - at > 0 ? len - at : 0;
        at += snprintf(room > 0 ? buf + at : nullptr, (size_t)room, fmt, a...);
    };
    if (p.error == PLAN_OK)
        for (int i = 0; i < p.n_stages; ++i)
            put("%s grid=%u block=%u lds=%u\n", search_kernel_name(p.stages[i].kernel), p.stages[i].grid, p.stages[i].block, p.stages[i].lds);
    static const char *const qp[] = {"none", "launch", "folded"}, *const fb[] = {"none", "launch", "tail"};
    if (p.error != PLAN_OK) put("flags path=none q_prep=none fallback=none canonical_scores=0 error=%s\n", plan_error_name(p.error));
    else put("flags path=%s q_prep=%s fallback=%s canonical_scores=%d leaves_bound=%d consumes_bound=%d groups=%d error=none\n",
             p.path, qp[p.q_prep], fb[p.fallback], p.canonical_scores ? 1 : 0, p.leaves_bound ? 1 : 0, p.consumes_bound ? 1 : 0, p.G);
    return at;
}

}  // namespace pfann
