// Host-side launchers of the HIP kernels (one translation unit per stage).
#pragma once
#include "common.h"
#include "encoder_plan.h"

namespace pfann {

// ---- mel.hip -------------------------------------------------------------------------
struct MelPlan {
    int seg_len, n_fft, hop, n_mels, n_frames, n_freqs, log2n;
    int power, pad_reflect, log_mode, spec_norm_max;
    float log_eps;
    float *window;        // [n_fft] periodic hann
    float2 *twiddle;      // [n_fft/2] exp(-2*pi*i*j/n_fft)
    int *fb_ptr;          // [n_mels+1] CSR over mel bins
    int *fb_idx;          // [nnz] frequency bin
    float *fb_val;        // [nnz]
    int max_nnz_row, fb_nnz;
};
// What one melspec_kernel launch of B windows is given: frames per output group (0: whole tile), workgroups per window,
// dynamic LDS bytes, and whether the 8x8x8 register FFT runs (n_fft == 1024) instead of the radix-2 FFT in LDS.
struct MelLaunch {
    int group_out, parts, radix8;
    size_t lds_bytes;
};
MelLaunch plan_melspec(const MelPlan &mp, int64_t B);
int launch_melspec(const MelPlan &mp, const float *segs, int64_t B, int64_t seg_stride,
                   const int64_t *starts, int remove_mean, float *out, hipStream_t s);
int launch_resample_to_mono(const int16_t *pcm, int n_ch, const float *K, int old_r, int new_r, int width, const int64_t *plan,
                            int n_pieces, int64_t n_out, float *tmp, float *wav, float *scratch2, hipStream_t s);
int launch_pcm16_to_mono(const int16_t *pcm, int64_t n_frames, int n_ch, float *wav,
                         float *scratch2, hipStream_t s);

// ---- encoder.hip ---------------------------------------------------------------------
int launch_conv_first(const SubLayer &L, const float *x, float *y, int64_t B, hipStream_t s);
int launch_conv_gemm(const SubLayer &L, const float *x, float *y, int64_t B, hipStream_t s, int64_t Bcall = 0);
int launch_conv_depthwise(const SubLayer &L, const float *x, float *y, int64_t B, hipStream_t s);
int launch_ln_act(const SubLayer &L, float *xy, int64_t B, int activation, int relu_after_bn,
                  hipStream_t s);
int launch_myg(const float *x, const float *w1, const float *b1, const float *w2, const float *b2,
               int d, int u, int v, int64_t B, float *emb, int normalize, hipStream_t s);
int launch_cl_to_nchw(const float *x, float *y, int64_t B, int C, int HW, hipStream_t s);

// ---- encoder_fused.hip (LayerNorm fused into the GEMM; "fuller" models) -------------------
bool fused_supported(const SubLayer *sub, int n);
int fused_out_slots(const SubLayer &L, int64_t B);
int launch_conv_first_stats(const SubLayer &L, const float *x, float *y, float *part, int64_t B, int act,
                            int after_bn, hipStream_t s);
int launch_conv_first_gram_stats(const SubLayer &L, const float *x, float *part, int64_t B, const float *gram14,
                                 hipStream_t s);
// in_stats: workspace for B x (mean, rstd) of the input, filled here from in_part
int launch_conv_gemm_ln(const SubLayer &L, const SubLayer &Lin, const float *x, const float *in_part, int in_P,
                        float *in_stats, float *y, float *out_part, int64_t B, int act, int after_bn,
                        const SubLayer *Lfirst, int precision, hipStream_t s, float *splitk_scratch = nullptr,
                        size_t splitk_bytes = 0, int *stats_final = nullptr, int64_t Bplan = 0, int64_t Bcall = 0);
// Bcall: the samples of the whole call when this launch is one internal stream's share of it (0: B); the variant is chosen for
// the call, so the stream count never changes a kernel choice.
// Every variant decision of the launchers above and below is made by csrc/encoder_plan.h (plan_conv_gemm_ln, plan_myg_ln,
// plan_out_slots); splitk_scratch must hold what plan_chunk_scratch states for the chunk.
int launch_conv_dw_ln(const SubLayer &L, const SubLayer &Lin, const float *x, const float *in_part, int in_P, float *in_stats,
                      float *y, float *out_part, int64_t B, int act, int after_bn, const SubLayer *Lfirst, hipStream_t s);
int launch_ln_apply(const SubLayer &L, const float *z, const float *part, int P, float *out, int64_t B, int act,
                    int after_bn, hipStream_t s);
int launch_myg_ln(const SubLayer &Llast, const float *z, const float *part, int P, int act, int after_bn,
                  const float *w1, const float *b1, const float *w2, const float *b2, int d, int u, int v, int64_t B,
                  float *emb, int normalize, hipStream_t s, int64_t Bplan = 0);
// Bplan (pfann_set_plan_batch): the batch size the kernel VARIANTS (tile size, split-K, small-batch head) are chosen for;
// 0 = the launch's own B.  With a fixed plan a segment's fingerprint has the same bits in every batch it is part of.

// ---- search.hip ----------------------------------------------------------------------
struct SearchWorkspace {
    int64_t cap_q = 0;      // query rows the buffers are sized for
    float *thr = nullptr;   // [cap_q]
    int *cnt = nullptr;     // [cap_q]
    int64_t *cl = nullptr;  // [cap_q][CAP] packed survivor keys (a sampled pass: [cap_q][groups] group maxima)
    int *overflow = nullptr;   // [0] unused, [1] rows left to the big select kernel, [2] rows the wave-per-row select left, [3] spare
    int *left = nullptr;       // [cap_q] the rows counted in overflow[2]: the workgroup selects then walk THIS list with a small grid
    int *row_ovf = nullptr;    // [cap_q] set by a select kernel whose row lost survivors (a sub-list overflowed);
                               // topk_fallback_kernel recomputes those rows exactly ON DEVICE and clears the flag:
                               // no host round trip, no retry loop (allocated zeroed)
    // fp16 pre-filter path (search_f16.hip)
    float *thr_adj = nullptr;  // [cap_q] tau - eps
    float *eps = nullptr;      // [cap_q] per-row bound of |s16 - s|
    void *qh = nullptr;        // [cap_q][d] fp16 query rows
    int64_t qh_elems = 0;
    // masked search (pfann_search_topk_excl; written by excl_prep_kernel, allocated on first use)
    uint2 *excl = nullptr;       // [cap_q] row range every query row leaves out
    uint2 *excl_tile = nullptr;  // [cap_q / 128 + 1] span of the union of each 128-row query tile's ranges (= excl + cap_q: one allocation)
    int64_t excl_cap = 0;
    // two-phase search of a song-sharded job (search_topk phase 1 -> all-reduce MAX of the bounds -> phase 2): what
    // phase 1 left behind, valid for exactly this (q, nq, k)
    const float *bound_q = nullptr;
    int64_t bound_nq = 0;
    int bound_k = 0, bound_G = 0;
    bool bound_valid = false;
};
// db != nullptr: fp32 rows, exact results; dbh != nullptr additionally: fp16 copy of the rows for the pre-filter path
// (batches > 64 rows), xnorm_max = largest row norm of db.
// db == nullptr (fp16-only storage, pfann_db_set_storage): scores are s16 = sum fl16(q_i) * fl16(x_i) accumulated in
// fp32, no fp32 re-scoring.  Fully asynchronous on `s`: no host synchronisation inside.
// phase 0: the whole search.  Song-sharded jobs split it around one collective (pfann_search_bound / _bounded):
//   phase 1: query preparation + sampled group-maximum pass + group select only; lb[m][0..mtop) = the mtop best sampled
//            group maxima of query row m, each lowered to a bound of the TRUE score of its row (-inf padding; all -inf
//            where this path has no sampled threshold).  The k-th largest of the union of all shards' values bounds the
//            k-th best over all shards from below (>= k different real rows reach it);
//   phase 2: lb[m] = that lower bound of the k-th best over ALL shards: the full pass
//            emits only rows that can be in the global top-k, so D / I may hold fewer than k entries (padded) -- the
//            merge of the shards' lists is still the exact global top-k.
int search_topk(const float *db, const void *dbh, float xnorm_max, int64_t n, int d, int64_t label_base,
                const float *q, int64_t nq, int k, float *D, int64_t *I, SearchWorkspace &ws, hipStream_t s,
                int phase = 0, float *lb = nullptr, int mtop = 1, const int64_t *excl_lo = nullptr,
                const int64_t *excl_hi = nullptr);
int topk_merge(const float *S, const int64_t *L, int64_t nq, int m, int k, float *D, int64_t *I,
               hipStream_t s);
// one wavefront per query row (search.hip): k-th largest of the gathered bound candidates; merge of G sorted shard lists
int bound_reduce(const float *cands, int G, int64_t nq, int m, int k, float *lb, hipStream_t s);
int merge_lists(const float *Dl, const int64_t *Il, int G, int64_t nq, int k, float *D, int64_t *I, hipStream_t s);

// ---- rerank.hip ----------------------------------------------------------------------
struct RerankArgs {
    const float *db; const void *dbh;   // fp32 rows, or (db == nullptr) fp16 rows
    int64_t n; int d; int64_t label_base;
    const int64_t *song_pos; int n_songs; int song_lo, song_hi;  // owned songs [lo,hi)
    const float *q; const int64_t *labels; int k;
    const int64_t *qstart; const int32_t *qlen; int64_t nQ;
    int fsm; float alpha; int mode; int only_owned;
    int pmax;               // next pow2 >= max_qlen * k (LDS sizing)
    unsigned long long *gkeys; float *gscore;   // HBM scratch [nQ][pmax] used instead of LDS when pmax > 8192
    int *ncand;             // [nQ] scratch of the phased launch (few queries: scoring spread over the whole GPU)
    int phase;              // 0: whole query in one workgroup; 1: candidates; 2: scores; 3: argmax (1-3 need gkeys)
    pfann_match_result *results; float *song_scores;
    int ss_lo, ss_n;        // the song_scores block of one query covers songs [ss_lo, ss_lo + ss_n): all, or the owned ones
    // pfann_match_topn (topn > 0: results and song_scores are null): top[nQ][topn] ranked songs, n_found[nQ] or null
    int topn = 0; pfann_match_result *top = nullptr; int *n_found = nullptr;
};
int launch_match(const RerankArgs &a, hipStream_t s);
int launch_match_pack(const pfann_match_result *res, int64_t nQ, unsigned long long *keys, hipStream_t s);
int launch_match_pick(const unsigned long long *keys, int G, int64_t nQ, pfann_match_result *out, hipStream_t s);
int launch_song_scores_to_seconds(float *ss, int64_t n_pairs, int fsm, double hop_size, int native_path, hipStream_t s);

// ---- monitor.hip: the matcher over every window of long recordings (pfann_match_windows) ----------------
static constexpr int WIN_SMAX = 256;    // rows one chunk of windows may span (and the longest window of the fast path)
struct WindowsArgs {
    const float *db; const void *dbh;   // fp32 rows, or (db == nullptr) fp16 rows; the WHOLE database (label_base 0)
    int d;
    const int64_t *song_pos; int n_songs;
    const float *q; const int64_t *labels; int k;
    const int64_t *rstart; const int32_t *rlen; int64_t nR;
    int window, hop;
    int C;                  // most window starts per chunk: match_windows_chunk(k, window, hop), >= 1
    const int64_t *wfirst;  // [nR + 1]
    pfann_match_result *results;
};
// window starts one workgroup can take (0: the lists do not fit the LDS, the caller expands the windows instead)
int match_windows_chunk(int k, int window, int hop);
// The fast path of api.hip's windows_call, which fills one WindowsTopnArgs for both forms.  The two launchers are one helper
// (monitor.hip: launch_windows -- bounds, LDS opt-in and size, fp32 / fp16 instantiation) over their own kernel pair.
int launch_match_windows(const WindowsArgs &a, hipStream_t s);
// the n best songs of every window (results unused: top[windows][n], n_found or null)
static constexpr int WIN_TOPN_FAST = 64;    // longest ranked list the windowed kernel keeps (its per-window lists live in LDS)
struct WindowsTopnArgs : WindowsArgs {
    int n; pfann_match_result *top; int *n_found;
};
int launch_match_windows_topn(const WindowsTopnArgs &a, hipStream_t s);
int launch_expand_windows(const int64_t *rstart, const int32_t *rlen, int64_t nR, int window, int hop, const int64_t *wfirst,
                          int64_t nW, int64_t *qstart, int32_t *qlen, hipStream_t s);

// ---- dense.hip: every alignment of every window, no nomination (pfann_match_windows_dense) ----------------
// One argument type for every form of the tile kernel (match_windows_dense_kernel<RANKED, STATS, SHARD>) and its select and
// decode; an instantiation reads the groups of its form and nothing else.
struct DenseArgs {
    // ---- every call
    const float *db; int64_t ntotal; int d;     // fp32 rows of this handle; ntotal, song_pos, n_songs: the WHOLE database
    const int64_t *song_pos; int n_songs;
    const float *q;
    const int64_t *rstart; const int32_t *rlen; int64_t nR;
    int window, hop;        // window 1..64
    const int64_t *wfirst;  // [nR + 1]
    int64_t nW;             // wfirst[nR], from the caller
    const int32_t *excl;    // [nR] song whose alignments are no candidates (-1: none), or null
    // ---- unranked: the running-best words go to results (whole handle: [nW], decoded in place) or to words (SHARD, below)
    pfann_match_result *results;
    pfann_dense_stats *stats;   // [nW] the count and the two fixed-point sums of every window's full pieces, or null: no moments
                                // (also read by the ranked form of a whole handle: pfann_match_windows_dense_topn_stats)
    // ---- SHARD only (pfann_match_windows_dense_part / _topn_part): db holds the GLOBAL rows [row_lo, row_lo + nrows), whole
    // songs [song_lo, song_lo + n_owned).  A whole handle has row_lo = 0, nrows = ntotal, song_lo = 0, n_owned = n_songs.
    int64_t row_lo, nrows;
    unsigned long long *words;  // unranked: [nW] raw running-best words, not decoded.  It stands here, behind results, stats,
                                // row_lo, nrows, because beside results the unranked part kernel compiles 0.3 % slower.
                                // The members' ORDER decides the kernels' argument loads: after adding or moving a member, run
                                // tools/ubench/match_windows_dense_ab.py against the build before it
    int song_lo, n_owned;
    // ---- ranked: one chunk of row-tile slots [slot_lo, slot_lo + slot_n) of the call.  The tile kernel leaves every song's best
    // packed word of every window of the chunk in ws, the select kernel ranks them.
    unsigned long long *ws; // [slot_n][wps][songs] packed words; songs = n_songs, or n_owned (indexed by song - song_lo) under SHARD
    int64_t slot_lo, slot_n;
    int wps;                // window starts one slot can hold: ceil((128 - (window-1)) / hop)
    int n; pfann_match_result *top; int32_t *n_found;   // top[nW][n]; n_found[nW] or null
    float *song_scores;     // [nW][n_songs][2] or null; whole handle only
};
// Both launchers zero what the kernels accumulate into (results or words, stats, ws); the rows and songs that size the work are
// shard ? nrows : ntotal and shard ? n_owned : n_songs.
// unranked: stats == nullptr picks the form without moments; a whole handle's words are decoded in place.  songs_with_rows:
// songs of the whole database with len > 0 (n_cand; unused for a shard)
int launch_dense_unranked(const DenseArgs &a, bool shard, int64_t songs_with_rows, hipStream_t s);
// ranked: one chunk.  stats != nullptr (whole handle) picks the form that also keeps the moments; the CALLER zeroes stats once,
// before its first chunk: the kernel adds into the windows of the call
int launch_dense_ranked(const DenseArgs &a, bool shard, hipStream_t s);
int dense_topn_wps(int window, int hop);
int64_t dense_topn_slots(int64_t nW, int64_t nR, int window, int hop);
// pfann_match_windows_dense_merge: words[n_parts][nW] (and part_stats[n_parts][nW], or both stats pointers null) -> what the
// whole database's call writes; every size is global
struct DenseMergeArgs {
    const int64_t *song_pos; int n_songs; int64_t ntotal, songs_with_rows;
    const unsigned long long *words; const pfann_dense_stats *part_stats; int n_parts;
    const int32_t *rlen; int64_t nR; int window; const int64_t *wfirst; int64_t nW; const int32_t *excl;
    pfann_match_result *results; pfann_dense_stats *stats;
};
int launch_dense_merge(const DenseMergeArgs &a, hipStream_t s);
// pfann_match_windows_dense_topn_merge: tops[n_parts][nW][n], nf_parts[n_parts][nW] (null exactly when n_found is)
int launch_dense_topn_merge(const pfann_match_result *tops, const int32_t *nf_parts, int n_parts, int64_t nW, int n,
                            pfann_match_result *top, int32_t *n_found, hipStream_t s);
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device): the attribute is per device
int ensure_dyn_lds(const void *func, int bytes);

// ---- dense_songs.hip: every alignment of the songs a query's list names (pfann_match_songs_dense) ----------------
// Its own argument type: DenseArgs' member order is part of the tile kernel's timing (above).
struct SongsDenseArgs {
    const float *db; int d;                 // fp32 rows of the WHOLE database
    const int64_t *song_pos; int n_songs;
    const float *q;
    const int64_t *qstart; const int32_t *qlen; int64_t nQ;
    const pfann_match_result *cand; int m;  // [nQ][m]; only .song is read
    pfann_match_result *top;                // [nQ][m]; between the two kernels the score fields hold the slots' packed words
    int32_t *n_found;                       // [nQ] or null
};
int launch_match_songs_dense(const SongsDenseArgs &a, hipStream_t s);

// ---- nominate.hip: the songs that can still be the dense winner, on the fp16 MFMA (pfann_nominate_songs_dense) ----------------
// Its own argument type, like SongsDenseArgs.
struct NominateArgs {
    const void *dbh; int64_t ntotal; int d;     // fp16 copy of the rows of the WHOLE database
    float xnorm_max;
    const int64_t *song_pos; int n_songs;
    const float *q;
    const int64_t *qstart; const int32_t *qlen; int64_t nQ;
    int max_qlen;                               // 1..64: the slot of a query in a 128-row tile
    // ---- one chunk of queries [q_lo, q_lo + q_n) and its scratch (nominate_scratch_layout)
    int64_t q_lo, q_n;
    unsigned *ws;                               // [q_n][n_songs] ordered bits of every song's best approximate total, 0: none
    int *bad;                                   // [q_n] the query has a row outside fp16's range (behind ws: zeroed with it)
    void *qh;                                   // [q_n][max_qlen][d] fp16 query rows, zeros past qlen
    float *eps, *norm;                          // [q_n][max_qlen] the bound and the norm of each row
    int n; pfann_match_result *cand;            // cand[nQ][n]
    int32_t *n_found, *n_close;                 // [nQ] or null
};
size_t nominate_query_bytes(int n_songs, int max_qlen, int d);
size_t nominate_scratch_bytes(int64_t q_n, int n_songs, int max_qlen, int d);
void nominate_scratch_layout(NominateArgs &a, void *base);  // needs q_n, n_songs, max_qlen, d
int launch_nominate_songs_dense(const NominateArgs &a, hipStream_t s);

// ---- nominate_windows.hip: the nomination for every window of long recordings, over tiles the windows share
// (pfann_nominate_windows_dense) ----------------
// Its own argument type, like NominateArgs.
struct NominateWindowsArgs {
    const void *dbh; int64_t ntotal; int d;     // fp16 copy of the rows of the WHOLE database
    float xnorm_max;
    const int64_t *song_pos; int n_songs;
    const float *q;
    const int64_t *rstart; const int32_t *rlen; int64_t nR;
    int window, hop;                            // window 1..64
    const int64_t *wfirst;                      // [nR + 1]
    int64_t nW;                                 // wfirst[nR], from the caller
    const int32_t *excl;                        // [nR] song whose alignments are no candidates (-1: none), or null
    // ---- once per call (nominate_windows_scratch_layout): row i of recording r is row
    // (wfirst[r] * hop / SI + r) * SI + r * (window-1) + i, SI = 128 - (window-1).  Recording r owns
    // wfirst[r+1] * hop / SI - wfirst[r] * hop / SI + 1 slots, more than nw * hop / SI, so its SI rows per slot and its halo
    // hold the (nw-1) * hop + min(window, rlen[r]) rows that its nw windows read
    int64_t n_rows;                             // nominate_windows_rows(nW, nR, window, hop)
    void *qh;                                   // [n_rows][d] fp16 rows
    float *eps, *norm;                          // [n_rows] the bound and the norm of each row
    int *bad;                                   // [n_rows] the row is outside fp16's range (its image is zeros)
    // ---- one chunk of row-tile slots [slot_lo, slot_lo + slot_n) of the call
    unsigned *ws;                               // [slot_n][wps][n_songs] ordered bits of every song's best approximate total, 0: none
    int64_t slot_lo, slot_n;
    int wps;                                    // window starts one slot can hold: dense_topn_wps(window, hop)
    int n; pfann_match_result *cand;            // cand[nW][n]
    int32_t *n_found, *n_close;                 // [nW] or null
};
int64_t nominate_windows_rows(int64_t nW, int64_t nR, int window, int hop);
size_t nominate_windows_image_bytes(int64_t n_rows, int d);         // the rows' share of the scratch; the chunk's ws lies behind it
void nominate_windows_scratch_layout(NominateWindowsArgs &a, void *base);   // needs n_rows, d; base 256-byte aligned
int launch_nominate_windows_prep(const NominateWindowsArgs &a, hipStream_t s);   // once per call, before its first chunk
int launch_nominate_windows_dense(const NominateWindowsArgs &a, hipStream_t s);  // one chunk: zeroes ws, tiles, select

// ---- dbstore.hip: what an update of a loaded handle needs (pfann_db_append / pfann_db_remove_songs) ----------------
struct DbRun { int64_t src, dst, len; };    // kept rows [src, src + len) go to [dst, dst + len), dst <= src
// atomic maximum of the row norms (the per-row arithmetic of rows_to_half_kernel) into song_max[song - song_base]; row r of x
// is global row row0_global + r; song_max holds non-negative floats (zeroed by the caller)
int launch_song_norm_max(const float *x, int64_t n, int d, int64_t row0_global, const int64_t *song_pos, int n_songs,
                         int song_base, float *song_max, hipStream_t s);
// destination rows [dst0, dst0 + n_rows) of the move, gathered into stage; runs_dev[0].dst <= dst0, ascending
int launch_gather_rows(const void *src, void *stage, const DbRun *runs_dev, int n_runs, int64_t dst0, int64_t n_rows,
                       int64_t row_bytes, hipStream_t s);
int64_t db_kept_runs(const std::vector<int64_t> &song_pos, const std::vector<char> &gone, std::vector<DbRun> &runs, int64_t *first);

// one per translation unit with device code (pfann_prewarm)
int prewarm_mel();
int prewarm_encoder();
int prewarm_encoder_fused();
int prewarm_search();
int prewarm_search_f16();
int prewarm_rerank();
int prewarm_monitor();
int prewarm_dense();
int prewarm_dense_songs();
int prewarm_dbstore();

}  // namespace pfann
