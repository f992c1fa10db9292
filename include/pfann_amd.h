/* pfann_amd C ABI -- the drop-in boundary of the MI355X hot path.
 *
 * Plain C: pointers, sizes, opaque handles.  No torch / C++ types cross this boundary.
 * Every function returns 0 (or a value documented below) on success and a negative code
 * on failure; pfann_last_error() returns the message of the last failure on this thread.
 * No exception ever crosses the boundary.  Pointers named *_dev are device (HBM)
 * pointers, e.g. torch.Tensor.data_ptr(); *_host are host pointers; `stream` is a
 * hipStream_t passed as void* (0 = the null stream).
 *
 * Reference interfaces these entry points replace (paths relative to the reference repo):
 *   version, seq_score      cpp/seqscore.cpp:27-43 (bound by ctypes at database.py:15-32,
 *                           called at database.py:178-189)
 *   pfann_melspec           datautil/melspec.py:33-50  MelSpec.forward
 *   pfann_encode            model.py:148-153           FpNetwork.forward(x, norm)
 *   pfann_segment_embed     builder.py:88-100 / matcher.py:110-128 emit loops fused with
 *                           datautil/musicdata.py:82-88 (pad, unfold, mean removal)
 *   pfann_pcm16_to_mono     datautil/musicdata.py:48,72-80
 *   pfann_resample_to_mono  datautil/musicdata.py:28-65 (julius.ResampleFrac, minute-wise) + 72-80
 *   pfann_db_*              database.py:75-109 Database.__init__ (index + song_pos)
 *   pfann_search_topk       database.py:121  index.search(query, top_k)  (exact flat IP)
 *   pfann_match             database.py:117-166 query_embeddings_base (search + rerank)
 *   pfann_match_windows_dense  database.py:129-163 with every row's label list = the whole database (no counterpart)
 *   pfann_match_windows_dense_stats  the same answer, and the moments of every window's full candidates (no counterpart)
 *   pfann_match_windows_dense_topn  the same candidates, the n best songs per window and the per-song block (no counterpart)
 *   pfann_match_windows_dense_topn_stats  the ranked lists and the moments from one pass (no counterpart)
 *   pfann_match_windows_dense_part / _merge, _topn_part / _topn_merge  the three above over song-sharded handles (no counterpart)
 */
#ifndef PFANN_AMD_H
#define PFANN_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFANN_SEQSCORE_VERSION 20220625002LL

/* ---- the reference's native seam, byte-identical signatures ------------------------ */

/* cpp/seqscore.cpp:27-30.  database.py:30 exits unless this equals 20220625002. */
long long version(void);

/* cpp/seqscore.cpp:32-43.  `index` is a pfann_db* (the reference passes a faiss::Index*;
 * only d + row fetch are used there).  All other pointers are HOST pointers, exactly as
 * database.py:178-189 passes them.  song_scores must arrive zeroed (database.py:176);
 * offsets are written in frames.  Returns the best song id, or -1 with no candidate. */
int seq_score(void *index, const int64_t *song_pos, int n_songs, const float *query,
              int query_len, const int64_t *labels, int top_k, float *song_scores,
              int frame_shift_mul, float score_alpha);

/* ---- errors ------------------------------------------------------------------------- */
const char *pfann_last_error(void);

/* ---- front-end + encoder ------------------------------------------------------------- */
typedef struct pfann_ctx pfann_ctx;

typedef struct pfann_config {
    /* front-end (config keys sample_rate, stft_n, stft_hop, n_mels, segment_size)        */
    int32_t segment_len;    /* samples per segment = int(sample_rate * segment_size)      */
    int32_t stft_n;         /* FFT size, power of two, 64..4096                            */
    int32_t stft_hop;
    int32_t n_mels;
    int32_t power;          /* 2 (default) or 1 (naf_mode), melspec.py:27                  */
    int32_t pad_reflect;    /* 1 reflect (default) / 0 constant zeros, melspec.py:28       */
    int32_t log_mode;       /* 1 natural log (default), 2 log10, 0 none, melspec.py:43-46  */
    int32_t spec_norm_max;  /* 0: L2 normalise (default); 1: 'max' mode, melspec.py:35,48  */
    float   log_eps;        /* 1e-8 (default) or 0.06 (naf_mode), melspec.py:38-41         */
    /* encoder (config key "model") */
    int32_t d, h, u;
    int32_t fuller;         /* 1: full conv2, 0: depthwise, model.py:26-29                 */
    int32_t activation;     /* 0 ReLU, 1 ELU, model.py:7-12                                */
    int32_t relu_after_bn;  /* model.py:58-72                                              */
    int32_t stride_t[8];    /* conv1 stride along T per block (default 2), model.py:83-85  */
    int32_t stride_f[8];    /* conv2 stride along F per block (default 2)                  */
    int32_t max_batch;      /* segments processed per internal pass (workspace size)       */
} pfann_config;

/* Creates a context on HIP device `device`; NULL on failure (see pfann_last_error). */
pfann_ctx *pfann_create(const pfann_config *cfg, int device);
void pfann_destroy(pfann_ctx *ctx);

/* Mel filterbank fb[n_freqs][n_mels] (host, row-major), n_freqs = stft_n/2+1.  The host
 * mirror builds it (pfann_amd/melspec.py) so any bank torchaudio would build can be used. */
int pfann_set_melbank(pfann_ctx *ctx, const float *fb_host, int n_freqs, int n_mels);

/* One tensor of FpNetwork.state_dict() by its reference name (e.g.
 * "f.convs.3.conv2.weight", "g.linear1.bias"), host pointer, PyTorch layout.  The library
 * re-lays it out for its kernels.  Returns -2 for an unknown name, -3 for a size mismatch. */
int pfann_load_weight(pfann_ctx *ctx, const char *name, const float *host, int64_t numel);
/* Number of state_dict tensors still missing (0 = ready). */
int pfann_weights_missing(pfann_ctx *ctx);

/* MelSpec.forward: segs_dev[b*seg_stride + i], i < segment_len  ->  out_dev[B][n_mels][T],
 * T = 1 + segment_len/stft_hop.  remove_mean=1 additionally subtracts each segment's mean
 * first (musicdata.py:88), letting callers pass overlapping windows of one waveform
 * (seg_stride = hop) instead of a materialised unfold. */
int pfann_melspec(pfann_ctx *ctx, const float *segs_dev, int64_t B, int64_t seg_stride,
                  int remove_mean, float *out_dev, void *stream);

/* The launch pfann_melspec (and the front end of pfann_segment_embed*) gives a call of B windows, without launching:
 * out = {group_out, parts, lds_bytes, radix8}: frames per output group (0: the whole [n_mels][T] tile leaves at once),
 * workgroups per window, dynamic LDS bytes, 1 if the 8x8x8 register FFT runs (stft_n == 1024) and 0 for the radix-2 FFT
 * in LDS.  PFANN_MEL_GROUP is honoured as in the launch.  Needs the mel bank (its nonzero count sizes the LDS).  0 / <0. */
int pfann_melspec_plan(pfann_ctx *ctx, int64_t B, int out[4]);

/* FpNetwork.forward(x, norm): mel_dev[B][n_mels][T] -> emb_dev[B][d]. */
int pfann_encode(pfann_ctx *ctx, const float *mel_dev, int64_t B, float *emb_dev,
                 int normalize, void *stream);

/* Fused segmenter tail + MelSpec + FpNetwork: B windows of wav_dev at stride seg_stride. */
int pfann_segment_embed(pfann_ctx *ctx, const float *wav_dev, int64_t B, int64_t seg_stride,
                        float *emb_dev, int normalize, void *stream);

/* Same, with explicit window starts: window b = wav_dev[starts_dev[b] .. +segment_len)
 * (many queries concatenated in one buffer; windows never straddle two recordings). */
int pfann_segment_embed_at(pfann_ctx *ctx, const float *wav_dev, const int64_t *starts_dev,
                           int64_t B, float *emb_dev, int normalize, void *stream);

/* int16 interleaved PCM -> float32 mono (x/32768, fake-stereo fix, channel mean). */
int pfann_pcm16_to_mono(pfann_ctx *ctx, const int16_t *pcm_dev, int64_t n_frames, int n_ch,
                        float *wav_dev, void *stream);

/* Many MONO files at the model's rate in one call (the per-song loop of builder.py:75-103 / matcher.py:87-110 spends its
 * host time per file): file i = n_samples[i] int16 samples at host_pcm[i] (pinned host memory uploads asynchronously)
 * is copied to pcm_dev[dst_off[i] ..] and the whole slab pcm_dev[0 .. total) is converted to wav_dev (x/32768) by ONE
 * launch.  Gaps between files (zero padding of short files, slots other paths fill afterwards) are the caller's. */
int pfann_pcm16_files_to_mono(pfann_ctx *ctx, const void *const *host_pcm, const int64_t *n_samples, const int64_t *dst_off,
                              int n_files, int16_t *pcm_dev, int64_t total, float *wav_dev, void *stream);

/* ---- host-side WAV input (no GPU involved): the reference's decode workers (DataLoader(num_workers=4) over
 * MusicDataset, builder.py:66; datautil/audio.py:130-149: `wave` module, 16-bit PCM only) as native threads that fill
 * one pinned slab per launch group.  pfann_wav_probe walks each file's RIFF chunks ("fmt " then "data", other chunks
 * skipped) and reports the frames that are really in the file; pfann_wav_read reads file i's n_frames*n_ch interleaved
 * samples to dst + dst_off[i] (int16 units).  status: 0 ok, or one of the codes below (such a file is what the reference
 * logs as a load error and treats as a 0-segment song, musicdata.py:95-101).  Both return 0, or <0 on bad arguments
 * (-2: a file does not fit dst_cap). */
typedef struct pfann_wav_info {
    int64_t n_frames;      /* per channel */
    int64_t data_pos;      /* byte offset of the samples in the file */
    int32_t n_ch;
    uint32_t sample_rate;  /* as the header states it, unsigned like the `wave` module reads it; 0 and absurd rates included */
    int32_t status;
    int32_t reserved;
} pfann_wav_info;
#define PFANN_WAV_EOPEN (-1)    /* cannot open / stat */
#define PFANN_WAV_EFORMAT (-2)  /* not RIFF/WAVE, or fmt / data chunk missing */
#define PFANN_WAV_ECODEC (-3)   /* not PCM (format tag != 1), or no channels */
#define PFANN_WAV_EWIDTH (-4)   /* not 16-bit samples */
#define PFANN_WAV_EREAD (-5)    /* read error */
int pfann_wav_probe(const char *const *paths, int n, int n_threads, pfann_wav_info *info);
int pfann_wav_read(const char *const *paths, int n, int n_threads, pfann_wav_info *info, const int64_t *dst_off,
                   int16_t *dst, int64_t dst_cap);

/* Files at another sample rate (datautil/musicdata.py:28-65: `julius.ResampleFrac(file_sr, sample_rate)`, applied to 60 s
 * pieces that start every 59 s, half a second dropped at the inner seams), then the same mono conversion.
 *   pcm_dev      int16 interleaved [n_in][n_ch]
 *   kernels_dev  float [new_rate][2*width + old_rate]: the resampler's polyphase filters for the gcd-reduced rates
 *                (pfann_amd/resample.py builds them as julius does)
 *   plan_dev     int64 [n_pieces][5] = {in_start, in_len, out_skip, out_keep, out_off} per piece, in samples
 *   tmp_dev      float [n_ch][n_out] scratch;  wav_dev float [n_out] result.
 * julius is an un-vendored, unpinned dependency of the reference: this path is restated from its published algorithm. */
int pfann_resample_to_mono(pfann_ctx *ctx, const int16_t *pcm_dev, int n_ch, const float *kernels_dev, int old_rate,
                           int new_rate, int width, const int64_t *plan_dev, int n_pieces, int64_t n_out, float *tmp_dev,
                           float *wav_dev, void *stream);

/* Debug/verification taps: copy the activation after sub-layer `idx` (0..15) of the LAST
 * pfann_encode call's first `B` samples to host as NCHW floats.  Returns numel or <0. */
int64_t pfann_debug_activation(pfann_ctx *ctx, int idx, int64_t B, float *host, int64_t cap);
/* Enable keeping those taps (costs one D2D copy per sub-layer; off by default): pfann_debug_keep_at(ctx, on, 0). */
void pfann_debug_keep(pfann_ctx *ctx, int on);
/* Taps mode and position.  mode 0: off.  mode 1: all 16 taps; the fused path then materialises the first conv instead
 * of folding it into sub-layer 1's loader, i.e. it runs ANOTHER plan than production for sub-layers 0 and 1.  mode 2: the
 * taps are taken beside the production plan, which is left exactly as it is (first conv folded, same kernels, same
 * embeddings bit for bit): taps 1..15 are kept and tap 0, where that plan folds the first conv and never materialises it,
 * is reported absent by pfann_debug_activation with an error that says so (a plan that does not fold it -- the unfused
 * path, PFANN_NO_FOLD_FIRST, a first conv of more than 256 channels -- has all 16 in either mode).  first_sample: the taps
 * are those of the 8 consecutive samples of the chunk that start there, clamped to the chunk (a chunk of B samples keeps
 * [min(first_sample, B - 8), ...), all of a chunk of 8 or fewer); pfann_debug_activation's sample 0 is the first kept
 * one.  Taps are defined for single-stream calls (pfann_set_streams 1) of at most max_batch samples.  Returns mode, <0 on
 * bad arguments. */
int pfann_debug_keep_at(pfann_ctx *ctx, int mode, int64_t first_sample);

/* Selects the LayerNorm-fused encoder path (default: on whenever the model supports it, i.e.
 * every conv2 is a full conv; off = separate LayerNorm kernels).  Returns the state now in
 * effect (1 fused / 0 unfused).  Both paths are parity-tested. */
int pfann_set_fused_layernorm(pfann_ctx *ctx, int on);

/* Arithmetic of the fused conv GEMMs.  0 (default): fp32 MFMA, bitwise an fmaf chain.  1: every operand as two
 * fp16 terms (x = hi + lo to 2^-22 relative; weights pre-scaled by a power of two), three fp16 MFMAs per product
 * (hi*hi + lo*hi + hi*lo) with fp32 accumulation -- fp32-grade results (embeddings within ~1e-6 of mode 0,
 * far inside the 1e-4 parity bar) at 3/16 of the MFMA cycles.  Needs the fused path.  Returns the mode now in
 * effect.  New capability: the reference computes these convolutions in fp32 (model.py:54-73). */
int pfann_set_encoder_precision(pfann_ctx *ctx, int mode);

/* Makes the HIP runtime initialise `device` and load every code object of this library now (one empty launch per
 * translation unit) instead of at each unit's first real launch: about 0.45 s that the drop-in tools spend on a thread
 * while the interpreter is still importing torch.  Needs no context; safe to call more than once.  0 / -1. */
int pfann_prewarm(int device);

/* Kernel-variant plan of the encoder.  By default every call picks its GEMM tile size, the split-K path and the
 * small-batch head from its OWN batch size, which makes the last bits of a fingerprint depend on the batch it was
 * computed in (different summation orders; all within 5e-6 of the fp32 reference).  pfann_set_plan_batch(ctx, n) with
 * n > 0 makes every later call pick the variants a batch of n segments would get (n < 65 is raised to 65), whatever
 * its own size: a segment then has bit-identical fingerprints in every batch -- the drop-in CLIs set n = their launch
 * group size, which is what makes their outputs byte-identical for any number of ranks and any grouping.  n = 0
 * restores the default.  Returns the value in effect.  New capability (the reference's PyTorch kernels make no such
 * promise either way; SURVEY 8a "batch independence"). */
int64_t pfann_set_plan_batch(pfann_ctx *ctx, int64_t n);

/* Number of internal HIP streams (1..8) a batch is split over inside pfann_encode /
 * pfann_segment_embed*: the MFMA-bound GEMMs of one sub-batch overlap the HBM-bound passes
 * of another.  Work is forked from and joined back into the caller's stream.  Returns n.
 * A call of B samples (at most max_batch) runs on min(n, B / 128) streams, in chunks of B / streams samples (the first
 * B % streams one larger).  The stream count changes no kernel choice: every chunk runs the kernel variants the whole call
 * would run on one stream -- the fingerprints are bit-identical for every n, pinned plan or not -- and owns a slice of the
 * split-K scratch.  A layer whose partials for one chunk would pass 256 MiB is not split (a rule of the layer and the chunk
 * alone, whatever earlier calls allocated), so n streams hold at most n x 256 MiB of it; if the scratch cannot be allocated
 * the call fails instead of running other kernels. */
int pfann_set_streams(pfann_ctx *ctx, int n);

/* The launches of one pfann_encode chunk as text, from the functions the launchers themselves execute
 * (csrc/encoder_plan.h); needs no device and no context.  cfg: the model (max_batch <= 0: 512); B: samples of the call
 * (above max_batch: the first chunk); plan_batch: as pfann_set_plan_batch; precision: as pfann_set_encoder_precision;
 * fused: 1 / 0 as pfann_set_fused_layernorm, -1 the context's default; taps: the mode of pfann_debug_keep_at; n_streams: as
 * pfann_set_streams.  Per stream chunk one line `chunk K b0= B= splitk_offset= splitk_bytes=`, then one line per launch:
 * `NAME grid= block= lds= layer= tile= n_splits= first= out_P=` -- the kernel with its template arguments as a kernel
 * trace prints it, workgroups, workgroup size, dynamic LDS bytes, the sub-layer (-1: the head) and, for the fused conv
 * layers, tile, split-K chunks (0: not split), whether the first conv is folded in and the LayerNorm partial slots per
 * sample of the output.  Last line: `flags fused= precision= plan_batch= fold_first= chunks= splitk_bytes= part_slots=`
 * (the call's split-K scratch and the partial slots pfann_create allocates).  Returns the text's length, -2 when buf is
 * too small, -1 on bad arguments. */
int pfann_encode_plan(const pfann_config *cfg, int64_t B, int64_t plan_batch, int precision, int fused, int taps, int n_streams,
                      char *buf, int len);

/* ---- database: device-resident fingerprints, exact search, sequence match ------------ */
typedef struct pfann_db pfann_db;

pfann_db *pfann_db_create(int d, int device);
void pfann_db_destroy(pfann_db *db);
int pfann_db_dim(pfann_db *db);
int64_t pfann_db_ntotal(pfann_db *db);

/* Loads rows emb[n][d] (host pointer if emb_is_device==0, else device pointer; copied) and
 * the int64 prefix sums song_pos_host[n_songs+1] (database.py:84-86).  `label_base` is
 * added to every label this shard reports (song-sharded multi-GPU: global row id of local
 * row 0); song_pos stays GLOBAL and the shard must start and end on song boundaries. */
int pfann_db_load(pfann_db *db, const float *emb, int emb_is_device, int64_t n,
                  const int64_t *song_pos_host, int n_songs, int64_t label_base);

/* ---- Database updates: songs are added to and taken out of a loaded handle without a reload.
 *
 * State contract.  After a successful pfann_db_append or pfann_db_remove_songs the handle answers EVERY later call --
 * search, masked search, both sharded halves, pfann_match*, the windowed, ranked and dense matchers (the dense statistics of
 * pfann_match_windows_dense_stats among them), seq_score, the
 * pfann_search_plan text, pfann_db_ntotal / _bytes / _owned_songs / _row_norm_max -- exactly, bit for bit, as a fresh
 * handle of the same storage mode and pre-filter setting that was pfann_db_load-ed with the resulting rows and song_pos.
 * After a failed call (< 0) the handle is unchanged: arguments are validated before anything is touched, and what has to
 * grow is allocated first and the old buffer freed only on success.  (A device error in the middle of a removal's move is
 * the one exception: the rows are moved in place.)
 *
 * Both are BLOCKING MAINTENANCE calls: they synchronise the device on entry and are complete on return.  They must not
 * overlap queries on the same handle (no query in flight on any stream, none issued from another thread meanwhile).
 * Both refuse a shard of a song-sharded database (label_base != 0 or not all songs owned) with -1; nothing is changed.
 *
 * pfann_db_reserve: capacity of at least `rows` rows and `songs` songs, never shrinks, contents unchanged.  On a handle
 *   without rows the request is noted and honoured by the first append (an empty handle holds no matrix, like a fresh one).
 * pfann_db_capacity: rows the matrices can hold without reallocation.
 * pfann_db_row_norm_max: the largest row norm the search uses for its fp16 error margin (0 when no fp16 rows were asked for).
 * pfann_db_append: n_new_songs songs with song_rows_host[i] >= 0 rows each (sum == n_rows, else -1) get the ids n_songs,
 *   n_songs + 1, ...; their rows emb[n_rows][d] (host or device pointer) go behind the last row.  Within the capacity the
 *   cost is proportional to the NEW rows: old rows are neither copied nor converted again, the fp16 copy is extended by
 *   converting the tail.  Beyond it the matrices grow geometrically (at least 1.5x), one device-to-device copy each.
 *   fp16-only storage: the fp32 rows pass through the bounded staging buffer of pfann_db_load; rows whose norm does not fit
 *   (>= 6e4) refuse the call with -3.  fp32 storage: a norm >= 1e4 drops the fp16 copy as a fresh load would.
 * pfann_db_remove_songs: the listed songs (any order, duplicates allowed; an id outside 0..n_songs-1 refuses the call) lose
 *   their rows, later rows move down in order, every song keeps its id: a removed song becomes a song without rows.  Rows
 *   before the first removed song are not touched.  The move walks the matrix in ascending chunks -- per chunk one gather
 *   launch into a bounded staging buffer and one copy down (csrc/dbstore.hip) -- whatever the number of songs; chunk size:
 *   the 64 MB of the load's staging, or PFANN_DB_MOVE_ROWS=<rows> (read at every call).  fp16 rows are moved, never
 *   converted again.  The norm maximum is taken again from per-song maxima kept since the load / append. */
int pfann_db_reserve(pfann_db *db, int64_t rows, int songs);
int64_t pfann_db_capacity(pfann_db *db);
float pfann_db_row_norm_max(pfann_db *db);
int pfann_db_append(pfann_db *db, const float *emb, int emb_is_device, int64_t n_rows,
                    const int32_t *song_rows_host, int n_new_songs);
int pfann_db_remove_songs(pfann_db *db, const int32_t *songs_host, int n);

/* Storage precision of the shard's rows; call BEFORE pfann_db_load.  Returns the mode in effect, <0 on error.
 *   PFANN_DB_F32 (default): fp32 rows (+ an fp16 copy for the pre-filter below); every result is exact fp32.
 *   PFANN_DB_F16: ONLY fp16 rows are kept (n*d*2 bytes, half the HBM footprint and half the bytes per scan
 *     pass).  Search returns the k best s16 = sum_i fl16(q_i)*fl16(x_i) (exact products, fp32 accumulation on
 *     v_mfma_f32_32x32x16_f16) with no fp32 re-scoring; the sequence matcher scores against the stored fp16
 *     rows.  Approximate with respect to the fp32 path.  This goes FURTHER than the reference's only fp16
 *     precedent, faiss' GpuMultipleClonerOptions.useFloat16 (database.py:101-104; cpp/faisscputest.cpp:97-108):
 *     there only the GPU search index is fp16 and the rerank still reconstructs fp32 rows from the CPU index
 *     (database.py:148-152); here the rerank scores -- and so tie / argmax decisions between near-equal
 *     candidates -- also carry fp16 rounding of the database rows (measured: 99.85 % identical decisions on
 *     BASELINE config 5).  Keep PFANN_DB_F32 when the reference's exact scores are wanted.  d % 8 == 0. */
#define PFANN_DB_F32 0
#define PFANN_DB_F16 1
int pfann_db_set_storage(pfann_db *db, int mode);

/* Batches of more than 64 query rows are scanned on the fp16 matrix cores with a rigorous error
 * margin and re-scored in exact fp32 (csrc/search_f16.hip): the result is the exact fp32 top-k
 * either way.  on=0 forces the all-fp32 scan.  Returns 1 if the pre-filter is now in use. */
int pfann_db_set_prefilter(pfann_db *db, int on);

/* Exact inner-product top-k of q_dev[nq][d] over the shard: D_dev[nq][k] descending,
 * I_dev[nq][k] int64 labels (+label_base); unfilled slots D=-FLT_MAX, I=-1.  Asynchronous on `stream`: the
 * call never synchronises with the host (rows whose survivor lists overflow -- thousands of ties at the k-th
 * score -- are recomputed exactly by a device-side fallback kernel). */
int pfann_search_topk(pfann_db *db, const float *q_dev, int64_t nq, int k, float *D_dev,
                      int64_t *I_dev, void *stream);

/* pfann_search_topk with one range of rows left out per query row (self-match: a song queried against its own database
 * leaves its own rows out).  excl_lo_dev / excl_hi_dev: int64 [nq] on the device, in the space of I_dev (row + label_base).
 *   - Row m gets the exact top-k over the shard's rows whose label is not in [excl_lo[m], excl_hi[m]).
 *   - Ranges are clipped to the shard; lo >= hi excludes nothing.  They are independent per query row (they may differ
 *     inside one 128-row query tile), and a row's result does not depend on the other rows' ranges.
 *   - Everything else is pfann_search_topk's contract: descending output with ties to the lower row; D = -FLT_MAX, I = -1
 *     padding when fewer than k rows remain (also when the range covers the whole shard); fully asynchronous on `stream`, no
 *     host synchronisation (one exception, as for the fp16 query buffer of pfann_search_topk: a call with more query
 *     rows than any before it on this handle frees and regrows the range buffers, and waits for `stream` before it
 *     does); rows whose survivor lists overflow are recomputed by the device fallback, which leaves the
 *     same rows out; nq > 16384 is walked in chunks; where pfann_search_topk returns the canonical fp32 scores
 *     (canonical_scores of the plan) so does this call, bit for bit.
 *   - With both pointers NULL (the call then IS pfann_search_topk), or every range empty, D and I are bit for bit those of
 *     pfann_search_topk.  One pointer NULL and the other not: -1.
 *   - fp32 rows, fp32 rows with their fp16 copy and fp16-only storage are all served, on every path of the plan
 *     (pfann_search_plan_excl prints it).  The excluded rows never reach a group maximum, a threshold or a survivor list,
 *     so thresholds come from rows that count: this is NOT a post-filter of pfann_search_topk's answer, which would come
 *     back with fewer than k rows whenever the range holds some of the k best.
 *   - The sharded halves (pfann_search_bound / _bounded) have no such form. */
int pfann_search_topk_excl(pfann_db *db, const float *q_dev, int64_t nq, int k, const int64_t *excl_lo_dev,
                           const int64_t *excl_hi_dev, float *D_dev, int64_t *I_dev, void *stream);

/* The same search split around ONE collective, for a database sharded over several GPUs (pfann_amd/dist.py; the
 * reference has no counterpart: database.py:101-104 replicates the index).  nq <= 16384 per call.
 *   pfann_search_bound        : query preparation + the sampled pass only; lb_dev[nq][m] = for every query row the m
 *                               best sampled scores of THIS shard (one per group of rows, so m different real rows),
 *                               each lowered to a bound of its exact inner product; -inf padding (all -inf where the
 *                               path taken has no sampled threshold: tiny shards, <= 32 query rows, k > 128).
 *   -- the caller gathers the ranks' values; the k-th largest of their union bounds the k-th best over all shards
 *      from below (dist.py sends m = 2k/ranks + 8 values per row and rank) --
 *   pfann_search_topk_bounded : finishes the search started by pfann_search_bound for the SAME (q_dev, nq, k) on the
 *                               same handle (nothing else may use the handle's search in between), lb_dev[nq] = the
 *                               reduced bound; rows that cannot reach it are not emitted, so D / I may hold fewer than k entries
 *                               (D = -FLT_MAX, I = -1 padding).  pfann_topk_merge of the shards' lists is the exact
 *                               global top-k.  Without a matching pfann_search_bound call it is pfann_search_topk. */
int pfann_search_bound(pfann_db *db, const float *q_dev, int64_t nq, int k, int m, float *lb_dev, void *stream);
int pfann_search_topk_bounded(pfann_db *db, const float *q_dev, int64_t nq, int k, const float *lb_dev,
                              float *D_dev, int64_t *I_dev, void *stream);

/* What a search call with this shape launches, as text, without touching a GPU (no handle: the shape is all it depends
 * on, besides the PFANN_* A/B switches of the process).  storage: 0 = fp32 rows only (also: pre-filter off), 1 = fp32 rows
 * with their fp16 copy, 2 = fp16-only storage; phase: 0 = pfann_search_topk, 1 = pfann_search_bound (mtop = its m),
 * 2 = pfann_search_topk_bounded, with resume_with_lb = 1 when it follows the pfann_search_bound of the same (q_dev, nq, k).
 * nq is one chunk (<= 16384 rows).  One line per launch in order -- `<kernel> grid=<workgroups> block=<threads> lds=<dynamic
 * bytes>`, the kernel named as a kernel trace prints it without return type, namespace and parameter list -- then one
 * `flags ...` line: path, q_prep (none / launch / folded), fallback (none / launch / tail), canonical_scores, error.  A shape
 * the search rejects gives the flags line alone, error=<which>.  Returns the length of the whole text (buf receives at most
 * len - 1 characters of it), -1 for an unknown storage or phase. */
int pfann_search_plan(int64_t n, int d, int64_t nq, int k, int storage, int phase, int resume_with_lb, int mtop,
                      char *buf, int len);
/* ... and what pfann_search_topk_excl (with ranges) launches for it: the same path on the masked kernels.  An export of
 * its own beside pfann_search_plan, whose signature and text stay as they are: new ABI surface, there so that a test can
 * assert the path a masked shape takes.  Same text format and return value; phase 0 only. */
int pfann_search_plan_excl(int64_t n, int d, int64_t nq, int k, int storage, char *buf, int len);

/* Exact top-k of arbitrary (score,label) lists: in[nq][m] -> out[nq][k] (merging per-shard
 * top-k lists after an all-gather).  Entries with label<0 are ignored. */
int pfann_topk_merge(pfann_db *db, const float *S_dev, const int64_t *L_dev, int64_t nq, int m,
                     int k, float *D_dev, int64_t *I_dev, void *stream);

/* The two reductions of the sharded search in the layouts the collectives deliver, one wavefront per query row:
 *   pfann_bound_reduce     : cands_dev[n_ranks][nq][m] (the all-gathered pfann_search_bound outputs) -> lb_dev[nq], the k-th
 *                            largest of each row's n_ranks * m values (-inf entries are absent; fewer than k present:
 *                            -FLT_MAX) -- what pfann_search_topk_bounded wants.  n_ranks * m <= 1024.
 *   pfann_topk_merge_lists : D_lists_dev / I_lists_dev[n_lists][nq][k] (every shard's list for these query rows, as the
 *                            all-to-all delivers them; label < 0 = padding) -> the exact top-k of the union, ordered like
 *                            pfann_topk_merge over the shard-major concatenation (ties: lower list first, then list order).
 *                            k <= 128, n_lists * k <= 1024. */
int pfann_bound_reduce(pfann_db *db, const float *cands_dev, int n_ranks, int64_t nq, int m, int k, float *lb_dev,
                       void *stream);
int pfann_topk_merge_lists(pfann_db *db, const float *D_lists_dev, const int64_t *I_lists_dev, int n_lists, int64_t nq,
                           int k, float *D_dev, int64_t *I_dev, void *stream);

/* Result of the sequence matcher for one query. */
typedef struct pfann_match_result {
    int32_t song;        /* best song id (global), -1 if no candidate                     */
    int32_t offset;      /* best offset in sub-query frames (t), python path              */
    int32_t shift;       /* frame shift of the best candidate                             */
    int32_t n_cand;      /* unique candidates scored                                       */
    double  score;       /* python path: fp32 dot / sub_len in double (database.py:157)   */
} pfann_match_result;

/* Candidate generation + sequence score + argmax for nQ queries at once, given labels.
 * Query j owns rows [qstart[j], qstart[j]+qlen[j]) of q_dev / labels_dev[.][k].
 * mode 0 = python path (database.py:129-163), mode 1 = native path (seqscore.cpp:49-135,
 * fp32 divide, offsets t*fsm-shift, score_alpha honoured).
 * results_dev[nQ]; song_scores_dev[nQ][n_songs][2] may be NULL; when given it must be
 * zeroed by the caller and receives (score, offset-in-frames) of songs owned by the shard.
 * only_owned: bit 0 restricts candidates to songs of this shard (multi-GPU rerank); bit 1 (PFANN_MATCH_OWNED_BLOCK,
 * only together with bit 0) makes song_scores_dev a [nQ][owned songs][2] block (pfann_db_owned_songs) instead of
 * [nQ][n_songs][2]: the shard's columns of the matcher's `.bin` matrix and nothing else.
 * max_qlen = largest qlen[j]: candidate lists of up to 8192 (qlen*k) entries are sorted in LDS,
 * longer ones (e.g. a 60 s query at k=100) in a per-query HBM slab the handle grows on demand;
 * a query longer than max_qlen gets song=-2. */
int pfann_match(pfann_db *db, const float *q_dev, const int64_t *labels_dev, int k,
                const int64_t *qstart_dev, const int32_t *qlen_dev, int64_t nQ, int max_qlen,
                int frame_shift_mul, float score_alpha, int mode, int only_owned,
                pfann_match_result *results_dev, float *song_scores_dev, void *stream);

#define PFANN_MATCH_ONLY_OWNED 1
#define PFANN_MATCH_OWNED_BLOCK 2

/* Ranked answers: the n best SONGS of every query, 1 <= n <= 64 (anything else: -1 with a message), selected on the
 * device from the matcher's own candidate list -- no [nQ][n_songs] block exists.  Asynchronous on `stream`, never
 * synchronises with the host.  top_dev[nQ][n]; n_found_dev[nQ] may be NULL.
 *   Candidates, order and scores are exactly those of pfann_match for the same arguments.  mode 0: candidates ordered by
 *     (shift, song, offset), score = fp32 dot / sub_len in double.  mode 1: ordered by (song, offset, shift), score = the
 *     fp32 score, score_alpha honoured.  only_owned bit 0 restricts candidates to the shard's songs; bit 1
 *     (PFANN_MATCH_OWNED_BLOCK) has no meaning here and is rejected (-1).
 *   Per-song best: among a song's candidates the first one in candidate order with the largest score wins, compared with
 *     a strict > in double -- the rule of the result argmax, not the float32 comparison of the per-song block.
 *   Ranking: songs by score descending; ties go to the song whose best candidate comes first in candidate order.
 *   Entry i of a query is the i-th song of that ranking: song, offset, shift and score of that song's best candidate;
 *     n_cand = the number of distinct candidates of that song (how many alignments voted for it).
 *   Entry 0 therefore equals pfann_match's result in song, offset, shift and score.
 *   Padding: entries beyond the number of candidate songs are {song -1, offset 0, shift 0, n_cand 0, score -inf}.
 *   n_found[j] = the number of distinct candidate songs of query j, not capped at n.
 *   A query longer than max_qlen is refused: entry 0 gets song = -2 (and n_cand = -1, as in pfann_match), the rest are
 *     padding, n_found = -1.
 *   fp32 and fp16 storage are both supported, and -- as with pfann_match, whose launch plans and thresholds this call
 *     shares -- a result's bits do not depend on which launch plan served the call. */
int pfann_match_topn(pfann_db *db, const float *q_dev, const int64_t *labels_dev, int k,
                     const int64_t *qstart_dev, const int32_t *qlen_dev, int64_t nQ, int max_qlen,
                     int frame_shift_mul, float score_alpha, int mode, int only_owned, int n,
                     pfann_match_result *top_dev /* [nQ][n] */, int32_t *n_found_dev /* [nQ], may be NULL */,
                     void *stream);

/* Monitor mode: the sequence matcher over EVERY window of nR long recordings, given the labels of all their rows.
 * Recording r owns rows [rstart[r], rstart[r]+rlen[r]) of q_dev / labels_dev[.][k].  Its windows start at rows 0, hop,
 * 2*hop, ... while w0 + window <= rlen[r]; a recording with 0 < rlen < window has exactly one window that covers all its
 * rows (the answer pfann_match gives for the whole recording); rlen == 0: none.  wfirst_dev[nR+1] = prefix sums of the
 * windows per recording (the caller computes them by this rule); window w0/hop of recording r is results_dev[wfirst[r] +
 * w0/hop], and results_dev has wfirst[nR] entries.
 * Every result is FIELD FOR FIELD what pfann_match returns for the query (qstart = rstart[r] + w0, qlen = window): song,
 * offset relative to the window's first row, shift, n_cand (the unique candidates nominated by that window's OWN rows),
 * score.  An alignment is a candidate of a window only if a top-k label of one of the window's rows nominates it (the
 * reference's rule, database.py:133-140 on emb[w0:w0+window]) even where another alignment would score higher; order and
 * tie-break are the reference's (np.unique order, strict >, first wins); rows outside the song contribute 0 and the
 * divisor stays sub_len.
 * mode 0, frame_shift_mul 1, score_alpha 0 (the default family), fp32 or fp16 storage: ONE kernel (csrc/monitor.hip)
 * builds the candidate alignments once per chunk of neighbouring windows, computes every needed (alignment, row) inner
 * product once and forms all window sums from them; fully asynchronous on `stream`.  A window's score bits are a
 * function of the window's rows and the candidate alone -- not of hop, the chunking, the other windows / recordings of
 * the call or the storage plan: each row dot is one fixed-layout fp32 reduction ((p0+p1)+(p2+p3) per lane, then the
 * wave butterfly), a window adds its row dots in ascending row order in fp32, and the total is divided by sub_len in
 * double.  (pfann_match sums a window as ONE long dot, so on real-valued rows the two agree to fp32 rounding -- within
 * 1e-6 of the float64 score -- and bit for bit wherever fp32 is exact.)
 * Everything else -- mode 1, score_alpha != 0, frame_shift_mul > 1, k * (window + hop - 1) > 8192 or window > 256 (no
 * chunk fits the in-LDS list), or PFANN_WINDOWS_GENERAL=1 in the environment -- takes the general path: the windows
 * are expanded to (qstart, qlen) pairs on the device and run through pfann_match in bounded launches.  That path reads
 * wfirst[nR] back first: one synchronisation with `stream`.
 * The handle must hold the WHOLE database (label_base 0, all songs): a recording is not sharded over GPUs (-1). */
int pfann_match_windows(pfann_db *db, const float *q_dev, const int64_t *labels_dev, int k,
                        const int64_t *rstart_dev, const int32_t *rlen_dev, int64_t nR,
                        int window, int hop, int frame_shift_mul, float score_alpha, int mode,
                        const int64_t *wfirst_dev, pfann_match_result *results_dev, void *stream);

/* Monitor mode, ranked: the n best SONGS of every window, 1 <= n <= 64 (anything else: -1 with a message, nothing is
 * launched).  Windows, wfirst_dev, short and empty recordings and the whole-database requirement on the handle (a shard:
 * -1, the same message) are exactly those of pfann_match_windows.  top_dev[wfirst[nR]][n]; n_found_dev[wfirst[nR]] may
 * be NULL.
 * The list of window w0 of recording r is FIELD FOR FIELD what pfann_match_topn returns for the query (qstart = rstart[r]
 * + w0, qlen = window, or the length of a shorter recording) with only_owned = 0: candidates are the alignments that the
 * window's OWN rows nominate; per song the first candidate in candidate order with the largest score wins (strict >);
 * songs rank by score descending, ties to the song whose best candidate comes first in candidate order; n_cand of an
 * entry = the distinct candidates of that song in that window; entries past the candidate songs are {song -1, offset 0,
 * shift 0, n_cand 0, score -inf}; n_found = the distinct candidate songs of the window, not capped at n.
 * Entry 0 of every window equals pfann_match_windows' result for the same arguments in song, offset, shift and score,
 * bit for bit, on whichever path served the call (n_cand differs by definition: here the candidates of that song only).
 * mode 0, frame_shift_mul 1, score_alpha 0, a chunk that fits (pfann_match_windows' condition) and n <= N_FAST = 64 --
 * every legal n: ONE kernel (csrc/monitor.hip, profiling tag seq_match_windows_topn), fully asynchronous on `stream`, no
 * scratch memory.  It forms every (alignment, window) total exactly as pfann_match_windows' kernel does, so the score
 * bits follow the same summation order and a window's entries are a function of the window's rows and the candidate
 * alone -- not of hop, the chunking, n, the other windows / recordings of the call or fp32 / fp16 storage; the entries
 * for n = a are the first a entries for n = b > a.
 * Everything else (the cases pfann_match_windows lists, PFANN_WINDOWS_GENERAL=1 among them) takes the general path: the
 * windows are expanded on the device and run through pfann_match_topn in bounded launches, after ONE read-back of
 * wfirst[nR] that synchronises with `stream`. */
int pfann_match_windows_topn(pfann_db *db, const float *q_dev, const int64_t *labels_dev, int k,
                             const int64_t *rstart_dev, const int32_t *rlen_dev, int64_t nR,
                             int window, int hop, int frame_shift_mul, float score_alpha, int mode,
                             const int64_t *wfirst_dev, int n,
                             pfann_match_result *top_dev /* [wfirst[nR]][n] */,
                             int32_t *n_found_dev /* [wfirst[nR]], may be NULL */, void *stream);

/* Dense matcher: EVERY alignment of every window, no top-k nomination (csrc/dense.hip; no reference counterpart: the
 * reference scores only what its per-row search nominates, database.py:133-140).  Mode 0, frame_shift_mul 1, score_alpha 0.
 * Recordings, windows, wfirst_dev, short recordings (one window of n = rlen rows) and empty ones follow pfann_match_windows'
 * rule; n_windows = wfirst[nR], passed by the caller; results_dev[n_windows].
 * The answer of a window of n rows Q[0..n) is what pfann_match returns for that slice when every row's label list is the
 * whole database (k = ntotal):
 *   candidates  every (song s with len_s > 0, offset o) with -(n-1) <= o <= len_s - 1;
 *   total(s, o) sum over t with 0 <= o + t < len_s of dot(Q[t], db[song_pos[s] + o + t]); rows outside the song add +0;
 *   score       (double)total / (double)n;
 *   winner      the largest score, strict >, first wins in (song, offset) ascending order (np.unique order of mode 0);
 *   n_cand      sum over the songs with rows of (len_s + n - 1); shift 0;
 *   no candidate (empty database, or everything excluded): song -1, offset 0, shift 0, n_cand 0, score -inf.
 * excl_song_dev[nR] (or NULL): one song id per recording, -1 for none, whose alignments are no candidates and do not
 * count in n_cand (self-match).
 * One MFMA kernel (v_mfma_f32_32x32x2_f32) forms 128 x 128 tiles of row dots in LDS, recording rows x database rows,
 * neighbouring tiles overlapping by window - 1 rows both ways; every diagonal stretch is cut at the song boundaries into
 * candidate totals; per (window, tile) one 64-bit atomicMax of (order-preserving bits of the total, 0xFFFFFFFF - id) into
 * the result slot's score field, id(s, o) = song_pos[s] + s * (n-1) + o + (n-1); a last small kernel decodes the slots in
 * place.  Fully asynchronous on `stream`: no read-back, no host synchronisation, no allocation.
 * SUMMATION ORDER: a row dot is the MFMA's fmaf chain from +0 over k ascending; a total adds its row dots in ascending
 * row order from +0 in fp32; no sliding or prefix sums.
 * BYTE CONTRACT: a window's 24 result bytes are a function of the window's rows, the database and its recording's excluded
 * song alone -- not of hop, the other windows or recordings of the call, the tiling or the run.
 * Returns -1 with a message, and launches nothing, when the handle is a shard (pfann_match_windows' message), the storage
 * is fp16-only (this form scores fp32 rows), window is outside 1..64, hop < 1, d % 4 != 0, or
 * ntotal + n_songs * (window - 1) >= 2^32 (the packed id). */
int pfann_match_windows_dense(pfann_db *db, const float *q_dev,
                              const int64_t *rstart_dev, const int32_t *rlen_dev, int64_t nR,
                              int window, int hop, const int64_t *wfirst_dev, int64_t n_windows,
                              const int32_t *excl_song_dev /* [nR] or NULL */,
                              pfann_match_result *results_dev, void *stream);

/* Dense matcher with background statistics: pfann_match_windows_dense's answer, and per window the first two moments of the
 * totals of its FULL candidates, from the same pass over the database (csrc/dense.hip).  Arguments, the window rule, short and
 * empty recordings, excl_song_dev and the asynchrony follow pfann_match_windows_dense; results_dev[n_windows] gets, byte for
 * byte, what that call writes for the same arguments; stats_dev[n_windows] gets, for a window of n rows,
 *   n_full    the candidates whose n rows all lie inside their song, 0 <= o <= len_s - n: the sum over the songs s other than
 *             the recording's excluded song with len_s >= n of (len_s - n + 1).  Candidates that hang over a song's edge, and
 *             every candidate of a song shorter than n, have fewer rows in their total and enter no sum (their numbers per
 *             overlap length follow from the song lengths alone: pfann_amd/significance.py);
 *   sum_q     the sum over those candidates of rint((double)total * 2^PFANN_DENSE_STATS_SUM_SHIFT);
 *   sumsq_q   the sum over those candidates of rint((double)total * (double)total * 2^PFANN_DENSE_STATS_SQ_SHIFT);
 * total = the fp32 total of pfann_match_windows_dense (SUMMATION ORDER there); both products are exact in double, so rint is
 * the only rounding, and the sums are 64-bit integer additions (wave shuffles, LDS, one 64-bit atomicAdd per non-zero entry
 * of a (window, tile)).  mean = sum_q / 2^24 / n_full, mean square = sumsq_q / 2^18 / n_full.
 * BYTE CONTRACT: integer addition is associative, so a window's 24 stats bytes, like its 24 result bytes, are a function of the
 * window's rows, the database and its recording's excluded song alone -- not of hop, the other windows or recordings of the
 * call, the tiling or the run.
 * RANGE: with unit-norm rows |total| <= 64, so a candidate adds at most 2^30 to either sum in magnitude, and with fewer than
 * 2^32 candidates neither sum can wrap.  Outside that range the sums wrap in two's complement, deterministically.
 * The call zeroes stats_dev with hipMemsetAsync on `stream`; no read-back, no host synchronisation, no allocation.
 * Returns -1 with a message, launches nothing and writes nothing, when stats_dev is NULL and in every case in which
 * pfann_match_windows_dense does.  After pfann_db_append / pfann_db_remove_songs the call answers as a fresh handle would. */
#define PFANN_DENSE_STATS_SUM_SHIFT 24
#define PFANN_DENSE_STATS_SQ_SHIFT  18
typedef struct { int64_t n_full, sum_q, sumsq_q; } pfann_dense_stats;
int pfann_match_windows_dense_stats(pfann_db *db, const float *q_dev,
                                    const int64_t *rstart_dev, const int32_t *rlen_dev, int64_t nR,
                                    int window, int hop, const int64_t *wfirst_dev, int64_t n_windows,
                                    const int32_t *excl_song_dev /* [nR] or NULL */,
                                    pfann_match_result *results_dev,
                                    pfann_dense_stats *stats_dev /* [n_windows] */, void *stream);

/* Dense matcher, ranked: the n best SONGS of every window over every alignment, 1 <= n <= 64 (csrc/dense.hip).  Recordings,
 * windows, wfirst_dev, n_windows, short and empty recordings and excl_song_dev follow pfann_match_windows_dense.
 * top_dev[n_windows][n]; n_found_dev[n_windows] and song_scores_dev[n_windows][n_songs][2] may be NULL.
 *   candidates, totals   exactly those of pfann_match_windows_dense: every (song s with rows, offset o) with
 *                 -(n_rows-1) <= o <= len_s - 1; total(s, o) adds the row dots in ascending row order from +0 in fp32, a row
 *                 dot is the MFMA's fmaf chain over ascending k; score = (double)total / (double)n_rows;
 *   per-song best  among a song's candidates the largest total, strict >, first wins in offset order: ties to the smaller offset;
 *   ranking       songs by score descending, ties to the lower song id.  Entry i = the i-th song: song, offset and score of
 *                 its best candidate, shift 0, n_cand = the distinct candidates of THAT song, len_s + n_rows - 1: field for
 *                 field what pfann_match_topn returns for the slice (mode 0, frame_shift_mul 1, score_alpha 0) when every
 *                 row's label list is the whole database;
 *   entry 0       equals pfann_match_windows_dense's result for the same arguments in song, offset, shift and score, bit for
 *                 bit (n_cand differs by definition);
 *   prefix        the entries for n = a are the first a entries for n = b > a;
 *   padding       entries past the songs are {song -1, offset 0, shift 0, n_cand 0, score -inf}; n_found = the songs with rows,
 *                 not counting the excluded song, not capped at n; a window without a candidate: all padding, n_found 0;
 *   song_scores   when given, EVERY slot of every window is written: ((float)score, (float)offset) of the song's best
 *                 candidate by the rule above where that score, rounded to float32, is > 0, and (0, 0) everywhere else
 *                 (songs without rows, the excluded song, scores <= 0: the reference's zero-initialised block records only
 *                 scores above it, database.py:125,158).  Offsets are frames; pfann_song_scores_to_seconds converts them.
 *                 ONE DELIBERATE DIFFERENCE from pfann_match's block: that block compares a song's candidates after rounding
 *                 the score to float32, this one compares totals; the two differ only where two different totals of one song
 *                 round to the same float32 score (then the offsets may differ, the scores do not).
 * BYTE CONTRACT: a window's n * 24 result bytes, its n_found and its row of the block are a function of the window's rows,
 * the database, its recording's excluded song and n (through the prefix rule only) -- not of hop, the other windows or
 * recordings of the call, the tiling, how the call was chunked, or the run.
 * The tile kernel of pfann_match_windows_dense reduces the candidate totals of every (window, tile) per SONG in LDS and
 * leaves each song's best packed word with one 64-bit atomicMax in a workspace [windows of a chunk][n_songs] that the
 * handle owns (8 bytes per pair, zeroed per chunk, at most 256 MB unless one row-tile slot of windows needs more); a select
 * kernel, one workgroup per window, lists the n largest words -- word order is the ranking -- and fills n_found and the
 * block.  Longer calls walk chunks of whole row-tile slots; PFANN_DENSE_TOPN_WINDOWS=<windows> in the environment (read at
 * every call) lowers the windows per chunk, rounded up to whole slots.
 * Fully asynchronous on `stream`, with ONE exception: a call that has to grow the workspace waits for `stream` first (the rule
 * of pfann_search_topk_excl's range buffers).  The workspace is sized from the handle's n_songs at every call, so after
 * pfann_db_append / pfann_db_remove_songs the call answers as a fresh handle would ("Database updates").
 * Returns -1 with a message, launches nothing and writes nothing, when n is outside 1..64, the handle is a shard
 * (pfann_match_windows' message), the storage is fp16-only, window is outside 1..64, hop < 1, d % 4 != 0, or
 * ntotal + n_songs * (window - 1) >= 2^32 (the packed id). */
int pfann_match_windows_dense_topn(pfann_db *db, const float *q_dev,
                                   const int64_t *rstart_dev, const int32_t *rlen_dev, int64_t nR,
                                   int window, int hop, const int64_t *wfirst_dev, int64_t n_windows,
                                   const int32_t *excl_song_dev /* [nR] or NULL */, int n,
                                   pfann_match_result *top_dev /* [n_windows][n] */,
                                   int32_t *n_found_dev /* [n_windows] or NULL */,
                                   float *song_scores_dev /* [n_windows][n_songs][2] or NULL */,
                                   void *stream);

/* Dense matcher, ranked, with background statistics: pfann_match_windows_dense_topn's lists and pfann_match_windows_dense_stats'
 * moments from ONE pass over the database (csrc/dense.hip: the ranked tile kernel also counts).  Arguments, the window rule,
 * short and empty recordings, excl_song_dev, n and the chunking follow pfann_match_windows_dense_topn.
 *   ranked outputs   top_dev, n_found_dev and song_scores_dev get, byte for byte, what pfann_match_windows_dense_topn writes for
 *                    the same arguments;
 *   statistics       stats_dev[n_windows] gets, byte for byte, what pfann_match_windows_dense_stats writes for them: n_full,
 *                    sum_q, sumsq_q of every window's full candidates, as defined there.  A stretch of a tile's diagonal is a
 *                    full candidate exactly when no song boundary cuts it, its song exists and is not the excluded one; it adds
 *                    the integers 1, rint((double)total * 2^24), rint((double)total * (double)total * 2^18) from the very total
 *                    that is packed into its word, by wave shuffles, one LDS entry per live window start and one 64-bit
 *                    atomicAdd per non-zero entry of a (window, tile) into the window of the CALL.
 * BYTE CONTRACT: both byte contracts carry over: a window's n * 24 result bytes, its n_found, its row of the block and its 24
 * stats bytes are a function of the window's rows, the database, its recording's excluded song and n (through the prefix rule
 * only) -- not of hop, the other windows or recordings of the call, the tiling, how the call was chunked
 * (PFANN_DENSE_TOPN_WINDOWS), or the run.  Every (window, tile) pair belongs to exactly one chunk and everything after the rint
 * is integer addition, so the call zeroes stats_dev ONCE, with hipMemsetAsync on `stream` before its first chunk.
 * Asynchrony as for pfann_match_windows_dense_topn: the one wait when the workspace grows.  After pfann_db_append /
 * pfann_db_remove_songs the call answers as a fresh handle would.
 * Returns -1 with a message, launches nothing and writes nothing, when stats_dev is NULL and in every case in which
 * pfann_match_windows_dense_topn does, in that call's order.  Whole handles only: there is no song-sharded form. */
int pfann_match_windows_dense_topn_stats(pfann_db *db, const float *q_dev,
                                         const int64_t *rstart_dev, const int32_t *rlen_dev, int64_t nR,
                                         int window, int hop, const int64_t *wfirst_dev, int64_t n_windows,
                                         const int32_t *excl_song_dev /* [nR] or NULL */, int n,
                                         pfann_match_result *top_dev /* [n_windows][n] */,
                                         int32_t *n_found_dev /* [n_windows] or NULL */,
                                         float *song_scores_dev /* [n_windows][n_songs][2] or NULL */,
                                         pfann_dense_stats *stats_dev /* [n_windows] */, void *stream);

/* Rescoring stage (csrc/dense_songs.hip): every alignment of the few songs a list names for each query, and nothing else.
 * cand_dev has the layout pfann_match_topn writes, so the two calls chain without glue: the nominated matcher names up to m
 * songs, this call scores each of them the way the dense matcher would.  Only the `song` field of an input entry is read.
 * Query j owns rows [qstart[j], qstart[j] + qlen[j]) of q_dev.
 *   listed songs  of query j: the distinct cand[j][i].song with 0 <= song < n_songs and at least one row.  Every other entry
 *                 is ignored: padding -1, a refusal's -2, an id out of range, a song without rows.  A song listed twice
 *                 counts once.  The list need not be sorted;
 *   per song      for a listed song s and a query of n rows, 1 <= n <= PFANN_SONGS_DENSE_MAX_ROWS, the definition is that of
 *                 pfann_match_windows_dense_topn for a window of those n rows: candidates are the offsets
 *                 -(n-1) <= o <= len_s - 1; total(s, o) is +0 plus, in ascending t, every dot(Q[t], db[song_pos[s] + o + t])
 *                 with 0 <= o + t < len_s, in fp32; a row dot is the fmaf chain from +0 over k = 0 .. d-1; the largest total
 *                 wins, ties go to the smaller offset; the entry is {song s, offset o, shift 0, n_cand = len_s + n - 1,
 *                 score = (double)total / (double)n};
 *   output        top[j] holds the listed songs' entries by score descending, ties to the lower song -- the ranked dense
 *                 matcher's order; the rest is padding {-1, 0, 0, 0, -inf}; n_found[j] = the number of listed songs;
 *   qlen[j] == 0  all padding, n_found = 0;
 *   qlen[j] > PFANN_SONGS_DENSE_MAX_ROWS   the query is not rescored: its m input entries are copied to its output unchanged
 *                 and n_found = -1.
 * BYTE CONTRACT: the bytes of a (query, song) entry are a function of the query's rows, the song's rows and n alone.  They do
 * not depend on m, the position in the list, the other songs of the list, the other queries of the call, the launch shape or
 * the run; they are the bytes pfann_match_windows_dense_topn gives that song for a one-window recording of the same rows.
 * Asynchronous on `stream`, never synchronises with the host, and allocates nothing: between its two kernels a slot's
 * running best lies in the score field of top_dev.  cand_dev and top_dev must not overlap.
 * Returns -1 with a message, launches nothing and writes nothing -- the first of these that applies is reported --: the
 * handle holds a shard (pfann_match_windows' message), the storage is fp16-only, m is outside 1..64; then d % 4 != 0, nQ < 0,
 * a null cand_dev or top_dev, a song of 2^31 - 64 rows or more. */
#define PFANN_SONGS_DENSE_MAX_ROWS 64
int pfann_match_songs_dense(pfann_db *db, const float *q_dev,
                            const int64_t *qstart_dev, const int32_t *qlen_dev, int64_t nQ,
                            const pfann_match_result *cand_dev /* [nQ][m] */, int m,
                            pfann_match_result *top_dev /* [nQ][m] */,
                            int32_t *n_found_dev /* [nQ], may be NULL */, void *stream);

/* Dense song nomination on the fp16 MFMA (csrc/nominate.hip): for each query the n songs with the best APPROXIMATE dense score,
 * in the layout pfann_match_topn writes, so it chains into pfann_match_songs_dense without glue -- dense-grade answers without a
 * search and without the fp32 dense pass --, and per query a certificate that the dense matcher's winner is among them.
 * Query j owns rows [qstart[j], qstart[j] + n_j) of q_dev, n_j = qlen[j], and is one window over all of them.
 *   candidates    the dense matcher's: every (song s with rows, offset o) with -(n_j-1) <= o <= len_s - 1, counting the rows
 *                 0 <= o + t < len_s;
 *   tot16(s, o)   +0 plus, in ascending t, S16[t][song_pos[s] + o + t], in fp32.  S16[t][g] is the fp32 accumulator of
 *                 v_mfma_f32_32x32x16_f16 over the k-blocks of 16 in ascending order from +0; its operands are the
 *                 round-to-nearest fp16 image of query row t and row g of the handle's fp16 copy.  No sliding or prefix sums;
 *   A_j(s)        the largest tot16(s, o) of song s;
 *   output        cand[j] ranks the songs with rows by A descending, ties to the lower song: entry i = {song, offset 0, shift 0,
 *                 n_cand = len_s + n_j - 1, score = (double)A / (double)n_j} -- the offset is not tracked --, the rest is
 *                 padding {-1, 0, 0, 0, -inf}; n_found[j] = the number of songs with rows, not capped at n;
 *   margin        eps_t = 1.05e-3 ||q_t|| X + 3.1e-8 sqrt(d) (||q_t|| + X) in fp32, X = pfann_db_row_norm_max (the fp16 scan's
 *                 bound of one row dot); B_j = X sum_t ||q_t||; E_j = sum_t eps_t + 2^-22 (d + n_j) B_j, in double from those
 *                 fp32 values.  |tot16 - T| <= E_j for every candidate, T being the dense matcher's fp32 total;
 *   n_close[j]    the number of songs with rows and (double)A_j(s) >= (double)max_s A_j(s) - 2 E_j.  n_close[j] <= n PROVES that
 *                 the dense matcher's best song is listed: after pfann_match_songs_dense, entry 0 is then byte for byte entry 0
 *                 of pfann_match_windows_dense_topn for a one-window recording of the same rows;
 *   qlen[j] == 0  all padding, n_found = 0, n_close = 0;
 *   qlen[j] > max_qlen, or a row with norm >= 6e4 or a NaN   all padding, n_found = -1, n_close = -1.
 * BYTE CONTRACT: a query's cand row, n_found and n_close are a function of its rows and the database alone: not of nQ,
 * max_qlen, the other queries, the chunking (PFANN_NOMINATE_QUERIES, read per call, lowers the queries per chunk), the launch
 * shape or the run.  The entries for n = a are the first a entries for n = b > a.
 * Asynchronous on `stream`, no read-back; allocates nothing apart from growing the handle's scratch on demand (which drains the
 * stream once).  Returns -1 with a message, launches nothing and writes nothing -- the first that applies is reported --: the
 * handle holds a shard (pfann_match_windows' message), the storage is fp16-only (the rescoring that follows needs fp32 rows),
 * the handle keeps no fp16 copy of its rows (d % 8 != 0, PFANN_NO_F16_PREFILTER at load, or row norms >= 1e4), n outside 1..64,
 * max_qlen outside 1..64, nQ < 0, a null cand_dev. */
int pfann_nominate_songs_dense(pfann_db *db, const float *q_dev,
                               const int64_t *qstart_dev, const int32_t *qlen_dev, int64_t nQ, int max_qlen,
                               int n, pfann_match_result *cand_dev /* [nQ][n] */,
                               int32_t *n_found_dev /* [nQ] or NULL */, int32_t *n_close_dev /* [nQ] or NULL */,
                               void *stream);

/* Windowed dense nomination (csrc/nominate_windows.hip): pfann_nominate_songs_dense for every window of long recordings -- monitor
 * mode's form of it.  Recordings, windows, wfirst_dev, n_windows, short recordings (one window of rlen rows) and empty recordings
 * follow pfann_match_windows_dense.  Window w of recording r is the query of rows [rstart[r] + w * hop, .. + wl),
 * wl = min(window, rlen[r]); its outputs are row wfirst[r] + w of cand_dev[n_windows][n], n_found_dev and n_close_dev.
 *   excl_song_dev NULL   a window's cand row, n_found and n_close are byte for byte what pfann_nominate_songs_dense writes for that
 *                 query: tot16, A, eps_t, E (summed in ascending t, in double) and the ranking keep their definitions and their
 *                 summation order;
 *   excl_song_dev[r] = s   the candidates of song s are no candidates of the windows of recording r (-1: none): s is not ranked
 *                 and not counted in n_found or n_close.  n_close <= n then proves that the best song of
 *                 pfann_match_windows_dense_topn called WITH THE SAME EXCLUSION is listed;
 *   a row with norm >= 6e4 or a NaN   every window that contains it is all padding, n_found = -1, n_close = -1; the windows that do
 *                 not contain it are unaffected;
 *   prefix        the entries for n = a are the first a entries for n = b > a.
 * Disjoint queries packed into tiles compute every row dot once per window; here a tile is 128 consecutive recording rows
 * against 128 database rows with a halo of window-1 rows both ways, as in csrc/dense.hip, and the 128 - (window-1) window starts
 * it owns share its row dots: at window 19, hop 2 that is 55 windows per tile product instead of 6.  A prep kernel writes ONE
 * fp16 image of the call's rows with their eps_t, norms and flags; the tile kernel leaves each song's best total per (window,
 * tile) with one 32-bit atomicMax in a workspace [windows of a chunk][n_songs] (4 bytes per pair, zeroed per chunk, at most
 * 256 MB unless one row-tile slot of windows needs more); a select kernel, one workgroup per window, ranks, counts n_close and
 * writes.  Longer calls walk chunks of whole row-tile slots; PFANN_NOMINATE_WINDOWS=<windows> in the environment (read at every
 * call) lowers the windows per chunk, rounded up to whole slots.
 * BYTE CONTRACT: a window's cand row, n_found and n_close are a function of its rows, the database and its recording's excluded
 * song alone: not of hop, the window's position, its neighbours, the other recordings, the chunking, the launch shape or the run.
 * Asynchronous on `stream`, no read-back; the only wait is growing the handle's scratch on demand (which drains the stream once).
 * Returns -1 with a message, launches nothing and writes nothing -- the first that applies is reported --: first
 * pfann_nominate_songs_dense's refusals in its order (a shard, fp16-only storage, no fp16 copy of the rows, n outside 1..64),
 * then window outside 1..64, hop < 1, nR < 0 or n_windows < 0, a null cand_dev. */
int pfann_nominate_windows_dense(pfann_db *db, const float *q_dev,
                                 const int64_t *rstart_dev, const int32_t *rlen_dev, int64_t nR,
                                 int window, int hop, const int64_t *wfirst_dev, int64_t n_windows,
                                 const int32_t *excl_song_dev /* [nR] or NULL */, int n,
                                 pfann_match_result *cand_dev /* [n_windows][n] */,
                                 int32_t *n_found_dev /* [n_windows] or NULL */,
                                 int32_t *n_close_dev /* [n_windows] or NULL */, void *stream);

/* Song-sharded dense matcher (csrc/dense.hip): the three calls above refuse a handle that holds a shard; these four split them
 * into a PART per handle and a MERGE, so that N handles that cut the song list into contiguous ranges -- N GPUs, each with 1/N
 * of the rows -- give, byte for byte, what one handle of the whole database gives.
 * WHY THE MERGE IS EXACT.  A candidate is (song, offset) and songs are never split, so every candidate belongs to exactly one
 * part.  Its total adds the row dots of rows of its own song only, in the summation order above: the part computes the very
 * float the whole database computes.  The packed word is (order-preserving bits of the total, 0xFFFFFFFF - id) with id formed
 * from the GLOBAL song_pos and song number, which every handle carries: words of different parts compare as they do inside one
 * handle, and the largest over the parts is the word the whole database's atomicMax leaves, ties included.  The statistics
 * are 64-bit integer sums over full candidates; their sum over the parts is the whole sum, bit for bit.
 *
 * pfann_match_windows_dense_part: any fp32 handle -- a shard (label_base, owned songs, global song_pos) or a whole database.
 * Recordings, windows, wfirst_dev, n_windows, short and empty recordings, excl_song_dev, the summation order and the asynchrony
 * follow pfann_match_windows_dense; the candidates are that call's, restricted to the handle's owned songs.  The tile kernel's
 * columns run over the handle's global rows [label_base, label_base + n): tile j starts at label_base + j * SI - (window-1),
 * SI = 128 - (window-1); rows outside the range are zeros without a song.  words_dev[n_windows] gets the raw running-best
 * word of every window (0: no candidate here), stats_dev[n_windows] (or NULL) the three integers over this handle's full
 * candidates.  A handle without rows launches no tile: zeros.
 *
 * pfann_match_windows_dense_merge: any handle of the database (only its song_pos is read).  words_dev[n_parts][n_windows],
 * part_stats_dev[n_parts][n_windows] or NULL; stats_dev is NULL exactly when part_stats_dev is.  One small kernel, one thread
 * per window: the maximum word, the two's-complement sums, then pfann_match_windows_dense's decode, n_cand from the global
 * sizes.  CONTRACT: for any cut of the song list into contiguous ranges, the parts in any order, results_dev and stats_dev get
 * the 24 + 24 bytes per window that pfann_match_windows_dense / _stats write for the same arguments on the whole database.
 *
 * pfann_match_windows_dense_topn_part: the ranked form over the handle's owned songs: workspace [windows of a chunk][owned
 * songs], top_dev[n_windows][n] with global song ids and n_cand = len_s + n_rows - 1, n_found_dev (or NULL) = the owned songs
 * with rows, not counting the excluded one.  No per-song block.  Chunks, PFANN_DENSE_TOPN_WINDOWS and the one wait when the
 * workspace grows follow pfann_match_windows_dense_topn.
 *
 * pfann_match_windows_dense_topn_merge: tops_dev[n_parts][n_windows][n], n_found_parts_dev[n_parts][n_windows] or NULL (exactly
 * when n_found_dev is).  Per window the n best of the n_parts * n entries by score descending, then song ascending, padding
 * last; n_found = the sum.  That order is the word order of the whole database's select: (double)total / (double)n_rows is
 * injective on fp32 totals for n_rows <= 64, so equal scores are equal totals, and the songs of different parts are disjoint, so
 * between equal totals the lower song is the smaller id.  CONTRACT: the bytes of pfann_match_windows_dense_topn on the whole
 * database, the prefix rule and "entry 0 equals the merged unranked answer" included.
 *
 * All four return -1 with a message, launch nothing and write nothing, when an output (or words_dev / tops_dev) is NULL, the
 * stats / n_found pair is mismatched, n_parts < 1, n is outside 1..64, window is outside 1..64, hop < 1, or the id bound fails on
 * the GLOBAL sizes, song_pos[n_songs] + n_songs * (window - 1) >= 2^32; the parts also when the storage is fp16-only or
 * d % 4 != 0. */
int pfann_match_windows_dense_part(pfann_db *db, const float *q_dev,
                                   const int64_t *rstart_dev, const int32_t *rlen_dev, int64_t nR,
                                   int window, int hop, const int64_t *wfirst_dev, int64_t n_windows,
                                   const int32_t *excl_song_dev /* [nR] or NULL */,
                                   uint64_t *words_dev /* [n_windows] */,
                                   pfann_dense_stats *stats_dev /* [n_windows] or NULL */, void *stream);
int pfann_match_windows_dense_merge(pfann_db *db, const uint64_t *words_dev /* [n_parts][n_windows] */,
                                    const pfann_dense_stats *part_stats_dev /* [n_parts][n_windows] or NULL */, int n_parts,
                                    const int32_t *rlen_dev, int64_t nR, int window, const int64_t *wfirst_dev,
                                    int64_t n_windows, const int32_t *excl_song_dev /* [nR] or NULL */,
                                    pfann_match_result *results_dev,
                                    pfann_dense_stats *stats_dev /* NULL exactly when part_stats_dev is */, void *stream);
int pfann_match_windows_dense_topn_part(pfann_db *db, const float *q_dev,
                                        const int64_t *rstart_dev, const int32_t *rlen_dev, int64_t nR,
                                        int window, int hop, const int64_t *wfirst_dev, int64_t n_windows,
                                        const int32_t *excl_song_dev /* [nR] or NULL */, int n,
                                        pfann_match_result *top_dev /* [n_windows][n] */,
                                        int32_t *n_found_dev /* [n_windows] or NULL */, void *stream);
int pfann_match_windows_dense_topn_merge(pfann_db *db, const pfann_match_result *tops_dev /* [n_parts][n_windows][n] */,
                                         const int32_t *n_found_parts_dev /* [n_parts][n_windows] or NULL */, int n_parts,
                                         int64_t n_windows, int n, pfann_match_result *top_dev /* [n_windows][n] */,
                                         int32_t *n_found_dev /* [n_windows] or NULL */, void *stream);

/* Songs whose rows all live in this shard: [*song_lo, *song_hi) (either pointer may be NULL); returns their number. */
int pfann_db_owned_songs(pfann_db *db, int *song_lo, int *song_hi);

/* pfann_db_load derives the owned songs from the shard's row range; songs WITHOUT rows (unreadable files: builder.py
 * writes a 0 into landmarkKey) that sit at a shard boundary are then ambiguous.  A caller that cut the song list itself
 * (pfann_amd/dist.py: shard_songs) states its cut here, after pfann_db_load: [song_lo, song_hi) must span exactly the
 * shard's rows (-3 otherwise).  Owner-side matching (PFANN_MATCH_ONLY_OWNED) and the owned score block
 * (PFANN_MATCH_OWNED_BLOCK) then use this range. */
int pfann_db_set_owned_songs(pfann_db *db, int song_lo, int song_hi);

/* In place, for n_pairs (score, alignment) pairs of a song_scores block written by pfann_match: the alignment slot
 * goes from fine frames (t * frame_shift_mul - shift) to seconds.  native_path 0: (t - shift / frame_shift_mul) * hop_size
 * computed in double and stored as float32 -- what database.py:148,160 leaves in song_score[:, 1]; native_path 1: the
 * float32 multiply of database.py:193, song_score[:, 1] *= hop_size / frame_shift_mul.  Asynchronous on `stream`. */
int pfann_song_scores_to_seconds(pfann_db *db, float *song_scores_dev, int64_t n_pairs, int frame_shift_mul,
                                 double hop_size, int native_path, void *stream);

/* Song-sharded multi-GPU retrieval, winner selection without the host (no reference counterpart):
 * pfann_match_pack turns this rank's results_dev[nQ] (from pfann_match with only_owned=1, python path) into one
 * 128-bit key per query, keys_dev[nQ][2] = (hi, lo) uint64, whose unsigned lexicographic order is the reference's
 * preference -- higher score first, ties to the smallest (shift, song, offset), the order of its np.unique-sorted
 * candidate list (database.py:129,140,158-163); a query without candidates gets all ones.  After an all-gather of the
 * keys (16 bytes per query and rank), pfann_match_pick reduces keys_dev[n_ranks][nQ][2] to the winners, out_dev[nQ]
 * (n_cand = 0).  Both are asynchronous on `stream`. */
int pfann_match_pack(pfann_db *db, const pfann_match_result *results_dev, int64_t nQ, uint64_t *keys_dev, void *stream);
int pfann_match_pick(pfann_db *db, const uint64_t *keys_dev, int n_ranks, int64_t nQ, pfann_match_result *out_dev,
                     void *stream);

/* Bytes of the shard's fingerprint matrix as stored (n*d*4, or n*d*2 with fp16 storage). */
int64_t pfann_db_bytes(pfann_db *db);

/* Timing hooks for bench.py: HIP events on the caller's stream around a tagged region.
 * With profiling enabled every kernel launch is bracketed by an event pair tagged with
 * the kernel's name ("conv_gemm", "scan_topk", "ln_act", ...); pfann_prof_elapsed_ms sums
 * all completed brackets of that tag since pfann_prof_reset, returning their count in *count. */
void pfann_prof_enable(int on);
/* Launches an empty kernel named pfann_bench_region_marker on `stream`: bench.py brackets its
 * timed region with two of them so a rocprofv3 trace can be cut to exactly that region. */
void pfann_prof_marker(void *stream);
void pfann_prof_reset(void);
double pfann_prof_elapsed_ms(const char *tag, int64_t *count);
/* Sum of the algorithmic work (flops for the MFMA-bound GEMM kernels, HBM bytes for the
 * streaming ones) of all launches recorded under `tag` since the last reset. */
double pfann_prof_work(const char *tag);
/* Comma-separated tags recorded since the last reset; returns their number or -1. */
int pfann_prof_tags(char *out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* PFANN_AMD_H */
