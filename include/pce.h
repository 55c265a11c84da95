/*
 * pce.h -- C ABI of the MI355X prosody-extraction engine ("pce").
 *
 * Drop-in boundary for the prosody + alignment hot path of
 * hi-paris/Prosody-Control-French-TTS.  The reference has no FFI of its own
 * (its boundary is Python call signatures); every entry
 * point below names the reference call it replaces.  Plain C: pointers and
 * sizes only, no C++/torch types.  The library (libpce.so) is built by hipcc
 * for gfx950 only and has NO CPU fallback: pce_create fails when no GPU is
 * present.
 *
 * Conventions
 *   - return value: 0 (PCE_OK) or a negative pce_status; text via pce_last_error.
 *   - one context per process per GPU, not thread-safe, one call in flight.
 *   - the caller owns every host buffer; the library owns device memory only.
 *   - *_run calls only enqueue kernels on the context's HIP stream; *_fetch
 *     calls synchronise that stream and copy results to host buffers.
 *   - audio is 16-bit PCM, mono; clips are concatenated, clip i occupying
 *     samples [offsets[i], offsets[i+1]) of the buffer.
 *   - a slice addresses samples [begin, end) of one clip in clip coordinates;
 *     indices outside [0, clip length) are "virtual" samples equal to zero,
 *     which is what both Praat's Sound_extractPart and pydub's silence padding
 *     produce.  Converting (t0, t1) seconds or ms to sample indices is host
 *     logic (pydub / Praat rules) and lives in the Python shim.
 */
#ifndef PCE_H
#define PCE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libpce.so is built with -fvisibility=hidden: the functions declared between this pragma and its pop are the library's ONLY exported
 * symbols (tests/test_abi_and_shard.py compares `nm -D` with this header, both ways). */
#pragma GCC visibility push(default)

/* PCE_API_VERSION changes when an existing entry point changes its signature or is removed; PCE_API_MINOR counts additive changes and
 * changes of observable defaults:  1 = round 4's default operand mode (fp16 operands + fp16 residual stream), decode loop without the
 * n_text_ctx pre-check;  2 = round 5: pce_levenshtein, pce_whisper_align_paths_enqueue / _wait, no frame limit in pce_pitch_run, the 256 x 256
 * GEMM for every batch size (a clip's Whisper results no longer depend on what it is batched with), unknown PCE_WHISPER_OPERANDS rejected,
 * pce_whisper_sample_keys (temperature sampling keyed by the caller's clip ids instead of batch positions);  3 = round 6: the encoder-output
 * cross-attention of a decoding step always cuts a clip's frames into the same four ranges (minor 2's promise now holds for every batch size: the
 * round-5 kernel cut them by the number of workgroups per clip, which followed the batch size), pce_whisper_align_paths_enqueue on a slot that
 * still holds an un-waited fetch is PCE_E_STATE, and no kernel carries the packed fp32 operand selection that returns wrong lanes beside MFMA waves
 * of other streams / contexts / processes (results no longer depend on what else runs on the device: tools/isa_guard.py); pce_selftest_xattn;
 * 4 = Whisper large-v3 / turbo widths on the decoding kernels: the encoder-output cross-attention of a decoding step (and pce_selftest_xattn) at
 * d = 1280 with 20 heads, and the single-query attention kernels of an incremental step for up to 32 heads (before, more than 16 heads fell back to
 * the K / V form without a word);  5 = pce_selftest_gemm_tiled, pce_selftest_layernorm; the LayerNorm kernels hold n_state up to 2048 (before, widths
 * above 1280 loaded and returned wrong numbers) and every loader refuses a width its run path cannot compute (see the dims structs);
 * 6 = pce_dtw_series (DTW of pairs of fp64 series, tiled over the whole device) and its two kernel ids;
 * 7 = pce_intensity_plan / _run / _fetch (Praat's Sound_to_Intensity over slices, with per-slice summaries) and their two kernel ids;
 * 8 = pce_selftest_attn1 (the single-query attention kernels of a decoding step) and pce_selftest_attention_ragged; pce_selftest_attention launches
 * through the product's rule (one query block: the streaming instantiation);
 * 9 = pce_silence_run / _shape / _fetch (pydub's detect_silence over slices, exact integers) and their three kernel ids;
 * 10 = pce_seqmatch / pce_seqmatch_align (difflib.SequenceMatcher's matched totals for batches of string pairs, and the fuzzy alignment of
 * "Compare Breaks" on them) and their two kernel ids;
 * 11 = pce_whisper_detect_language (openai-whisper's detect_language for the encoded batch: the language rows of the output projection only);
 * 12 = pce_selftest_gemm_resid; the 16-bit-stream encoder adds its residuals in the attention-projection / fc2 GEMM epilogues (same bits; a context
 * created with PCE_RESID_EPILOGUE=0 keeps the stored branch outputs and the adds in the LayerNorm passes; =2 fuses fc2 only, for A/B runs);
 * 13 = pce_crepe_load / _run / _shape / _fetch, pce_selftest_crepe_layer and pce_selftest_crepe_decode (CREPE pitch tracking of the resident batch) and their seven kernel
 * ids, which sit in front of PCE_K_SEQMATCH: the numeric values of PCE_K_SEQMATCH / PCE_K_SEQMATCH_ALIGN moved by seven (pce_kernel_name follows);
 * 14 = pce_selftest_align_matrix (the three kernels between the forced alignment's queries and its DTW, stage by stage through the run's own launches);
 * 15 = pce_ctc_align (CTC forced alignment of a batch of clips: trellis, path and token frames) and its three kernel ids, which sit in
 * front of PCE_K_SEQMATCH as minor 13's do: the numeric values of PCE_K_SEQMATCH / PCE_K_SEQMATCH_ALIGN moved by three (pce_kernel_name follows);
 * 16 = pce_w2v_check / _load / _run / _shape / _fetch / _device, pce_w2v_window_plan and pce_selftest_w2v_wave / _lngelu / _posconv (the wav2vec2 / MMS CTC
 * forward pass of the resident batch: the emissions pce_ctc_align reads in place) and their four kernel ids, which sit behind minor 13's and in
 * front of minor 15's: the numeric values of PCE_K_CTC .. PCE_K_SEQMATCH_ALIGN moved by four (pce_kernel_name follows);
 * 17 = pce_selftest_decode_rules (the kernels that turn a decoding step's logits into tokens and carry them into the loop's tables, on host arrays
 * through the decoding calls' own launches);
 * 18 = pce_selftest_logmel_image (the 16-bit time-major log-mel image the conv stem reads, copied out as the last run left it);
 * 19 = pce_selftest_xattn_stages (pce_selftest_xattn with the skip list and the buffers between its three kernels copied out: Q' as hi + lo, the nodes' U
 * and (m, l));
 * 20 = pce_wx_align (whisperX's forced alignment of a batch of segments: wildcard trellis and beam back-track) and its three kernel ids, which
 * sit behind minor 16's and in front of minor 15's: the numeric values of PCE_K_CTC .. PCE_K_SEQMATCH_ALIGN moved by three (pce_kernel_name follows);
 * 21 = pce_w2v_run_segments, pce_w2v_segments_plan, pce_w2v_segment_frames and pce_selftest_w2v_wave_segments / _posconv_segments (the wav2vec2 forward pass over
 * segments of unequal length, each alone and unpadded: whisperX's emissions, which pce_wx_align reads in place).  No kernel id: its launches
 * count under minor 16's four;
 * 22 = pce_pyin_fetch_observations (the observation lists the last pce_pyin_run left for a clip) and pce_selftest_pyin_viterbi (k_pyin_viterbi on given
 * observation lists through the run's own launch); out-of-band predecessors of the pYIN decoding tie on the rounded sum V + log(tiny), as the dense
 * argmax does (before: on V, which could name another predecessor where two values lay within a few ulp);
 * 23 = pce_pitch_fetch_candidates (the refined candidates, their counts and the intensities the last pce_pitch_run left for every frame) and
 * pce_selftest_pitch_path (k_pitch_delta, k_pitch_path and the two median kernels on given candidates through the run's own launches); the seeded
 * refinement replays Praat's iterates for candidates above 10.5 x the pitch floor too (before: up to 5e-6 relative from Praat's frequency on candidates
 * of short lag at 44.1 / 48 kHz, above a 600 Hz ceiling except between 525 and 600 Hz at a 50 Hz floor), and a slice without a peak (all zeros, a constant) stores intensity 0, not NaN, per frame;
 * 24 = pce_ivl_match (the text matching of the aligner evaluation, Code/whisper_testing/splitting.py: batches of claim problems over class tables
 * of (gold tier, predicted tier) pairs) and its two kernel ids, which sit behind minor 13's and in front of minor 16's: the numeric values of
 * PCE_K_W2V .. PCE_K_SEQMATCH_ALIGN moved by two (pce_kernel_name follows);
 * 25 = pce_lufs_fetch_stages and pce_lufs_stage_sizes (the chunk and block tables, the coefficients, the power table, the per-chunk states and
 * energies, the per-block mean squares and the peaks the last pce_lufs_run left).  No kernel changed;
 * 26 = pce_selftest_encoder_walk (the encoder layer walk Whisper's tiled encoder, BERT and wav2vec2 share, on host arrays through the loaders' weight
 * packer, with the buffer behind every launch copied out).  No kernel changed. */
#define PCE_API_VERSION 1
#define PCE_API_MINOR 26

typedef struct pce_ctx pce_ctx;

enum pce_status {
    PCE_OK = 0,
    PCE_E_INVALID = -1,   /* bad argument                                  */
    PCE_E_DEVICE = -2,    /* HIP runtime error (text in pce_last_error)    */
    PCE_E_NOMEM = -3,     /* host or device allocation failed              */
    PCE_E_STATE = -4,     /* call order violated (fetch before run, ...)   */
    PCE_E_LIMIT = -5      /* input exceeds a documented engine limit       */
};

/* per-slice status codes written to int32 status arrays */
enum pce_slice_status {
    PCE_SLICE_OK = 0,
    PCE_SLICE_TOO_SHORT = 1,  /* Praat would throw / pyloudnorm raises ValueError */
    PCE_SLICE_EMPTY = 2       /* zero samples                                      */
};

typedef struct pce_slice {
    int32_t clip;     /* index into the uploaded batch                               */
    int32_t flags;    /* reserved, 0                                                 */
    int64_t begin;    /* first sample (clip coordinates, may be < 0)                 */
    int64_t end;      /* one past the last sample (may exceed the clip length)       */
    double  x1;       /* time of sample `begin` in seconds (Praat Sound.x1); only
                         the pitch analysis reads it                                 */
} pce_slice;

/* ---- context ---------------------------------------------------------- */

/* stream: a hipStream_t to enqueue on (e.g. torch.cuda.current_stream().cuda_stream)
 * or NULL for a private stream.  Returns NULL on failure with text in err. */
pce_ctx *pce_create(int device, void *stream, char *err, size_t errlen);
void pce_destroy(pce_ctx *ctx);
const char *pce_last_error(const pce_ctx *ctx);
int pce_sync(pce_ctx *ctx);
int pce_api_version(void);
int pce_api_minor(void);
int pce_device_info(pce_ctx *ctx, char *name, size_t namelen, int32_t *compute_units, int64_t *hbm_bytes);

/* ---- batch residency ---------------------------------------------------
 * Replaces the per-call full-file decode of the reference closures
 * (AudioSegment.from_file / parselmouth.Sound(path) in
 * Code/audioPipeline.py:319,327,340,361): a batch is decoded once by the host,
 * uploaded once and stays resident in HBM for every measurement. */
int pce_upload_pcm_s16(pce_ctx *ctx, const int16_t *pcm, const int64_t *offsets, int32_t n_clips, int32_t sample_rate);
/* zero-copy variant: d_pcm is a device pointer that stays valid until the next
 * upload/bind/destroy; it must be 16-byte aligned and followed by >= 16 readable bytes. */
int pce_bind_pcm_s16_device(pce_ctx *ctx, const void *d_pcm, const int64_t *offsets, int32_t n_clips, int32_t sample_rate);
int pce_num_clips(const pce_ctx *ctx);

/* ---- sample-rate conversion of the resident batch -------
 * Stands in for the ffmpeg decode-to-16-kHz inside whisper.load_audio
 * (Code/Aligners/use_whisper_timestamped.py:139): y = upfirdn(taps, x, up, down)[n_pre_remove : n_pre_remove + n_out],
 * n_out = ceil(n_in * up / down), fp64 accumulation, round-half-even to int16.  The low-pass
 * `taps` (already scaled by `up`, zero padded as scipy.signal.resample_poly does) is host logic
 * (hostrules.resample_filter).  The resampled batch REPLACES the resident batch. */
int pce_resample_run(pce_ctx *ctx, int32_t up, int32_t down, const double *taps, int32_t n_taps, int64_t n_pre_remove);
/* copy the resident batch back: pcm may be NULL to query offsets[n_clips+1] / sample_rate only */
int pce_download_pcm_s16(pce_ctx *ctx, int16_t *pcm, int64_t *offsets, int32_t *sample_rate);

/* ---- frame-level short-time energy (the energy detector of the aligner's VAD) ----
 * Replaces the per-window energy of auditok.split(energy_threshold=50), which whisper-timestamped runs because the
 * aligner asks for `"vad": "auditok"` (Code/Aligners/use_whisper_timestamped.py:152; packages absent from
 * /root/reference: restated from their published behaviour, parity unpinned).  Frame k of a clip of n samples covers
 * [k*hop, min(k*hop + window, n)), k = 0 .. ceil(n/hop)-1: with hop == window these are auditok's analysis windows
 * (0.05 s; the last one short).  sum_sq[k] = exact integer sum of squares, count[k] = samples in the frame; the
 * mean / sqrt / 20 log10 / threshold are host logic (Aligners/vad.py).  requantize != 0 first applies, per sample,
 * whisper-timestamped's float32 round trip: (int16)((float32)(x / 32768) * 32767), truncated toward zero. */
int pce_frame_energy_run(pce_ctx *ctx, int32_t window, int32_t hop, int32_t requantize);
int pce_frame_energy_shape(pce_ctx *ctx, int32_t clip, int64_t *n_frames);
int pce_frame_energy_fetch(pce_ctx *ctx, int32_t clip, int64_t *sum_sq /* [n_frames] or NULL */, int32_t *count /* [n_frames] or NULL */);

/* ---- R3 / R7: short-time energy, peak, silence gate --------------------
 * Replaces _calculate_loudness (Code/Pipeline/compute_loudness_adjustments.py:8-25),
 * _check_audio_content (Code/Aligners/use_whisper_timestamped.py:197-229 and its
 * inline copy :581-599) and the np.abs(samples).max() of get_lufs
 * (Code/audioPipeline.py:349).  All fields are exact integers; the few
 * floating-point finishing operations (sqrt/log10) are host logic. */
typedef struct pce_energy {
    int64_t n;              /* samples in the slice, virtual zeros included           */
    int64_t sum_sq;         /* sum of x*x (true integer squares)                      */
    int64_t sum_sq_wrap16;  /* sum of (int16)(x*x): numpy int16 ** 2 wraparound (R3)  */
    int64_t n_loud;         /* count of (int16)abs(x) > loud_threshold  (R7; abs(-32768) wraps to -32768) */
    int32_t peak_abs;       /* max |x| as a true integer (0..32768)                   */
    int32_t reserved;
} pce_energy;
int pce_energy_run(pce_ctx *ctx, const pce_slice *slices, int32_t n_slices, int32_t loud_threshold);
int pce_energy_fetch(pce_ctx *ctx, pce_energy *out /* n_slices */);

/* ---- R4: BS.1770 integrated loudness -----------------------------------
 * Replaces pyloudnorm.Meter(rate).integrated_loudness(samples / peak) as called
 * by get_lufs (Code/audioPipeline.py:338-358): peak normalisation, K-weighting
 * biquads designed for the batch's sample rate, 400 ms / 75 % blocks, -70 LKFS and
 * -10 LU gates.  status[i] = PCE_SLICE_TOO_SHORT where pyloudnorm raises
 * ValueError (n < 0.4 * rate); the whole-file fallback is the caller's.
 * pce_lufs_set_meter_rate: the reference builds ONE meter from the natural recording's frame rate
 * (Code/audioPipeline.py:372,493: pyln.Meter(AudioSegment.from_file(wav).frame_rate)) and measures the raw synthesis with
 * it as well, whatever that file's own rate is (Azure's default RIFF output is 16 kHz, the recordings are 44.1 kHz):
 * filter design, the 0.4 s block length in samples and the too-short test all use the METER's rate.  rate > 0 makes
 * the following pce_lufs_run calls do the same; 0 (default) = the batch's rate. */
int pce_lufs_set_meter_rate(pce_ctx *ctx, int32_t rate);
int pce_lufs_run(pce_ctx *ctx, const pce_slice *slices, int32_t n_slices);
int pce_lufs_fetch(pce_ctx *ctx, double *lufs /* n_slices */, int32_t *status /* n_slices */);

/* Test hooks (tests/test_gpu_lufs_stages.py).  Since minor 25.
 * pce_lufs_fetch_stages: what the host plan and the four kernels of the last pce_lufs_run left (read only; joins the run's side stream; nothing
 * is computed or changed).  The loudness chain cuts every slice into chunks of at most 256 samples whose borders hold every gating-block
 * bound of pyloudnorm; k_lufs_pass1 leaves the end state of every chunk run from a zero state, k_lufs_scan the true begin states, k_lufs_pass2
 * the sum of squares of the K-weighted samples, k_lufs_gate the mean square z of every gating block.
 *   coef [13]: b[3], a[3] of the high shelf, c[3], d[3] of the high pass (a[0] = d[0] = 1) and 1 / (0.4 * meter rate), as the kernels took them;
 *   apow [257][16]: the powers 0 .. 256 of the cascade's zero-input transition matrix (row major 4 x 4; state order: shelf z0, z1, high-pass w0, w1);
 *   chunks [n_chunks]: rel = first sample relative to the slice's begin; state_end: pass 1; state_init: the scan; energy: pass 2;
 *   slices [n_slices]: chunk and block ranges (blocks' c0, c1 count chunks from the slice's first_chunk), the status, and peak = the integer the
 *     run divided the samples by (max |x| of the slice's real samples; 1 where that is 0);
 *   blocks [n_blocks]: the block sums chunks [c0, c1) of its slice; z = coef[12] * (their energies added in chunk order).
 * Any pointer may be NULL.  pce_lufs_stage_sizes gives the three counts.  PCE_E_STATE: before a pce_lufs_run, or when the run took its peaks from a
 * pce_energy_run of the same slices and a pce_energy_run of other slices has replaced them since. */
typedef struct pce_lufs_chunk {
    int64_t rel;
    int32_t len, slice;
    double state_end[4], state_init[4], energy;
} pce_lufs_chunk;
typedef struct pce_lufs_slice_plan {
    int32_t first_chunk, n_chunks, first_block, n_blocks, status, peak;
} pce_lufs_slice_plan;
typedef struct pce_lufs_block {
    int32_t c0, c1;
    double z;
} pce_lufs_block;
int pce_lufs_stage_sizes(pce_ctx *ctx, int32_t *n_slices, int64_t *n_chunks, int64_t *n_blocks);
int pce_lufs_fetch_stages(pce_ctx *ctx, double *coef, double *apow, pce_lufs_chunk *chunks, pce_lufs_slice_plan *slices, pce_lufs_block *blocks);

/* ---- R1 / R2: Praat autocorrelation pitch ------------------------------
 * Replaces parselmouth Sound.to_pitch(pitch_floor, pitch_ceiling) followed by
 * selected_array["frequency"] and the voiced median (get_median_pitch,
 * Code/audioPipeline.py:326-335) or the voiced geometric mean
 * (calculate_pitch_segment, Code/Pipeline/compute_pitch_adjustments.py:167-208). */
typedef struct pce_pitch_params {
    double  time_step;            /* <= 0: 0.75 / pitch_floor                    */
    double  pitch_floor;
    double  periods_per_window;   /* 3.0                                         */
    int32_t max_candidates;       /* 15                                          */
    int32_t reserved;
    double  silence_threshold;    /* 0.03 */
    double  voicing_threshold;    /* 0.45 */
    double  octave_cost;          /* 0.01 */
    double  octave_jump_cost;     /* 0.35 */
    double  voiced_unvoiced_cost; /* 0.14 */
    double  pitch_ceiling;
} pce_pitch_params;

typedef struct pce_pitch_summary {
    int64_t n_frames;     /* 0 when status != PCE_SLICE_OK                             */
    int64_t n_voiced;     /* frames with f0 > 0                                        */
    double  median_f0;    /* np.median of voiced f0, 0.0 when none                     */
    double  mean_log_f0;  /* mean of ln(f0) over voiced frames (exp -> geometric mean) */
    double  t1;           /* centre time of the first frame                            */
    int32_t status;       /* pce_slice_status                                          */
    int32_t reserved;
} pce_pitch_summary;

/* Host-only sizing: frame_offsets[n_slices+1] (prefix sum of frame counts). */
int pce_pitch_plan(pce_ctx *ctx, const pce_pitch_params *p, const pce_slice *slices, int32_t n_slices,
                   int64_t *frame_offsets, int32_t *status);
int pce_pitch_run(pce_ctx *ctx, const pce_pitch_params *p, const pce_slice *slices, int32_t n_slices);
/* How k_pitch_refine searches a candidate's maximum (Praat: NUMimproveMaximum -> NUMminimize_brent on the sinc-interpolated
 * autocorrelation).  PCE_REFINE_SEEDED (default): successive parabolic interpolation seeded with the three samples around the peak,
 * Praat's own iterates only where the two could differ (within 0.03 lag of a sample, when a safeguard trips, or at a lag so short that the
 * tolerance of Praat's minimiser, 3e-8 of the position lag + half window, exceeds 1e-6 of the lag: frequencies above 10.5 x the floor, since
 * minor 23): every candidate's frequency agrees with Praat's to 1e-6 relative, its strength to 1e-6.  PCE_REFINE_PRAAT: NUMminimize_brent's iterates replayed for every candidate (iterate for iterate; about
 * 2.5 x the refinement time).  The environment variable PCE_PITCH_REFINE=praat at pce_create selects the second as the context's default. */
enum { PCE_REFINE_SEEDED = 0, PCE_REFINE_PRAAT = 1 };
int pce_pitch_set_refine(pce_ctx *ctx, int32_t mode);
/* f0 / strength: ragged [frame_offsets[n_slices]], either may be NULL. */
int pce_pitch_fetch(pce_ctx *ctx, double *f0, double *strength, pce_pitch_summary *summary /* n_slices */);
/* Test hooks (tests/test_gpu_pitch_stages.py).  Since minor 23.
 * pce_pitch_fetch_candidates: what k_pitch_frames and k_pitch_refine left for every frame of the last pce_pitch_run (read only; joins the run's
 * tail first), in the order of pce_pitch_fetch: ncand [frames] (1 = the voiceless candidate alone), intensity [frames], and the refined candidates
 * cand_f / cand_s [frames][16] (frequency, strength).  Slot 0 reads 0 / 0; slots at or beyond ncand are not written on the device and keep what the
 * caller put there.  Any pointer may be NULL.
 * pce_selftest_pitch_path: Pitch_pathFinder and the voiced summaries on the caller's candidates, through the launches of pce_pitch_run (the same
 * function: same grids, list capacities and LDS).  Slice i holds frames frame_off[i] .. frame_off[i + 1]; ncand, intensity [frames] and cand_f,
 * cand_s [frames][16] as the fetch above returns them (slot 0 is the voiceless candidate whatever it holds; slots >= ncand are never read); `p`
 * supplies the five costs and thresholds and the ceiling, which is taken as given (no clamp to a Nyquist frequency), dt the frame step of the
 * time-step correction.  Out: f0, strength [frames]; psi [frames][16], the back-pointers of the frames with more than one candidate (0 elsewhere);
 * summary [n_slices] (t1 = 0).  Each may be NULL.  PCE_E_INVALID for ncand outside 1 .. 16, PCE_E_LIMIT for max_candidates > 16.  Works in the
 * context's pitch buffers: a pce_pitch_fetch after it is PCE_E_STATE until the next pce_pitch_run, which plans afresh. */
int pce_pitch_fetch_candidates(pce_ctx *ctx, int32_t *ncand, double *intensity, double *cand_f, double *cand_s);
int pce_selftest_pitch_path(pce_ctx *ctx, const pce_pitch_params *p, double dt, int32_t n_slices, const int64_t *frame_off, const int32_t *ncand,
                            const double *intensity, const double *cand_f, const double *cand_s, double *f0, double *strength, uint8_t *psi,
                            pce_pitch_summary *summary /* n_slices */);

/* ---- Praat intensity ------------------------------------------------------
 * Replaces parselmouth Sound.to_intensity() as Code/visualisation/Compare_speech_noenhanced.py calls it (extract_mean_volume :19-26, the
 * 'volume' branch of plot_zscore_feature / plot_raw_feature :166-168, :300-302): Praat's Sound_to_Intensity over slices of the resident
 * batch, sample values x / 32768, everything in fp64.  parselmouth and the Praat sources are absent: restated from the published
 * algorithm, parity with Praat unpinned (checked by known answers only).
 *   window = 6.4 / pitch_floor, half = window / 2, hs = floor(half / dx): 2 hs + 1 taps
 *   taps[k + hs] = I0f((2 pi^2 + 0.5) sqrt(max(0, 1 - (k dx / half)^2))), I0f = Praat's NUMbessel_i0_f (Abramowitz-Stegun 9.8.1 / 9.8.2);
 *   the table is host logic (hostrules.intensity_window) and is handed to the run call: n_taps != 2 hs + 1 is PCE_E_INVALID;
 *   frames by Sampled_shortTermAnalysis (the rule of the pitch plan entry) with this window and dt = time_step: window > n dx is
 *   PCE_SLICE_TOO_SHORT, no samples PCE_SLICE_EMPTY, n_frames = floor((n dx - window) / dt) + 1;
 *   frame f: centre = the sample nearest t1 + f dt, span = centre +- hs CLIPPED to the slice (Praat clips here: the weight sum shrinks
 *   with the clip; samples of the slice that lie outside its clip are zeros as everywhere else); with subtract_mean the unweighted mean of
 *   the span is removed first (exact integer numerator: a constant signal gives exactly zero);
 *   I = sum (a - mean)^2 w / sum w / 4e-10;  value = -300 when I < 1e-30, else 10 log10 I.
 * A frame's bits depend on its own samples and the table only (lane-strided sums, a fixed reduction tree, no atomics), not on the batch.
 * Limit: at most 6145 taps (pitch_floor >= 50 Hz at 48 kHz, >= 16.7 Hz at 16 kHz); more is PCE_E_LIMIT from the run call. */
typedef struct pce_intensity_params {
    double  pitch_floor;      /* 100.0 (Praat: minimum pitch)                 */
    double  time_step;        /* <= 0: 0.8 / pitch_floor                      */
    int32_t subtract_mean;    /* 1                                            */
    int32_t reserved;
} pce_intensity_params;

typedef struct pce_intensity_summary {
    int64_t n_frames;         /* 0 when status != PCE_SLICE_OK                             */
    int64_t n_positive;       /* frames with a value > 0                                   */
    double  mean_positive;    /* mean of those values (fixed order), NaN when none         */
    double  t1;               /* centre time of the first frame                            */
    int32_t status;           /* pce_slice_status                                          */
    int32_t reserved;
} pce_intensity_summary;

/* Host-only sizing: frame_offsets[n_slices+1] (prefix sum of frame counts); status may be NULL. */
int pce_intensity_plan(pce_ctx *ctx, const pce_intensity_params *p, const pce_slice *slices, int32_t n_slices,
                       int64_t *frame_offsets, int32_t *status);
int pce_intensity_run(pce_ctx *ctx, const pce_intensity_params *p, const double *taps, int32_t n_taps, const pce_slice *slices,
                      int32_t n_slices);
/* values: ragged [frame_offsets[n_slices]] dB, may be NULL (a corpus run downloads 40 bytes per slice); summary [n_slices], may be NULL. */
int pce_intensity_fetch(pce_ctx *ctx, double *values, pce_intensity_summary *summary);

/* ---- silence detection (pydub.silence) --------------------------------------
 * Replaces pydub.silence.detect_silence, the loop under split_on_silence(audio, min_silence_len=1000, silence_thresh=-50, keep_silence=300)
 * of Code/Preprocessing/preprocess_audio.py:41-46 and under detect_nonsilent (Code/audioPipeline.py:720, :786-797).  pydub 0.25.1 is third party
 * and absent: the range bookkeeping is restated from its published source, parity unpinned; the window test is the arithmetic of stdlib
 * audioop.rms, the function pydub calls.  For a slice of n frames (channels interleaved samples each) at the batch's frame rate:
 *   len_ms = round-half-even(1000 * (n / rate));  b(m) = (int64)((double)m * (rate / 1000.0)) frames, the fp64 product of pydub's slicing;
 *   windows start at i = 0, seek_step, 2 seek_step, ... <= last = len_ms - min_silence_len, and at `last` itself where seek_step does not
 *   divide it; none when len_ms < min_silence_len.  Window i covers frames [b(i), b(i + min_silence_len)); frames at or beyond n are zeros that
 *   count (pydub's silence padding) and samples of the slice outside its clip are zeros as everywhere else;
 *   window i is silent iff  sum x^2 < (rms_max + 1)^2 * samples in the window  (<=> audioop.rms(window) <= threshold for rms_max =
 *   floor(threshold): no square root, no floating point in the decision; the dB -> rms_max rule is host logic, hostrules.silence_rms_max);
 *   a silent start s opens a new range iff there is no silent start p before it or (s != p + seek_step and s > p + min_silence_len); a range is
 *   [its first start, its last start + min_silence_len] in milliseconds.
 * Slice bounds are in interleaved samples and must be multiples of `channels`.  status[i]: PCE_SLICE_EMPTY for a slice without samples.
 * PCE_E_INVALID: min_silence_len < 1, seek_step < 1, channels < 1, an rms_max < 0, misaligned slice bounds; PCE_E_LIMIT: a slice longer than
 * 2^31 - 1 ms; PCE_E_STATE: _shape / _fetch before _run.  A slice has at most len_ms / (min_silence_len + 1) + 1 ranges.  All integer: a slice's
 * ranges depend on its own samples only, not on the batch.  Since minor 9. */
typedef struct pce_silence_params { int32_t min_silence_len, seek_step, channels, reserved; } pce_silence_params;
int pce_silence_run(pce_ctx *ctx, const pce_silence_params *p, const pce_slice *slices, const int32_t *rms_max /* [n_slices] */, int32_t n_slices);
int pce_silence_shape(pce_ctx *ctx, int64_t *range_offsets /* [n_slices + 1] */, int32_t *len_ms /* [n_slices] or NULL */, int32_t *status /* [n_slices] or NULL */);
/* ranges: (start_ms, end_ms) pairs, slice after slice: [2 * range_offsets[n_slices]] */
int pce_silence_fetch(pce_ctx *ctx, int32_t *ranges);

/* ---- R10: STFT magnitude in dB -----------------------------------------
 * Replaces librosa.amplitude_to_db(np.abs(librosa.stft(y, n_fft, hop_length)),
 * ref=np.max) (Code/visualisation/app.py:69-72, acoustic_analysis.py:76-90):
 * periodic Hann, centred frames with zero padding, float32, amin 1e-5, top_db 80.
 * One [n_fft/2+1, 1+n/hop] row-major float32 matrix per uploaded clip. */
int pce_stft_db_run(pce_ctx *ctx, int32_t n_fft, int32_t hop);
int pce_stft_db_shape(pce_ctx *ctx, int32_t clip, int32_t *n_bins, int32_t *n_frames);
int pce_stft_db_fetch(pce_ctx *ctx, int32_t clip, float *out);
/* device pointer + byte size of the resident result (all clips, concatenated) */
int pce_stft_db_device(pce_ctx *ctx, const void **d_ptr, int64_t *bytes);

/* ---- R10: probabilistic YIN -------------------------------------------------
 * Replaces librosa.pyin(audio, sr=sr, fmin=60, fmax=2000, hop_length=256) of the reference's viewers
 * (Code/visualisation/app.py:74-78, acoustic_analysis.py:76-94, visualisation_abtest/app.py:108-111): frame_length 2048,
 * win_length 1024, centred zero-padded frames, 100 thresholds with the beta(2, 18) prior, Boltzmann(2) trough prior,
 * 0.1-semitone pitch bins, triangular local transitions, switch probability 0.01, dense Viterbi (first maximum).
 * librosa is third party and absent: restated from its published implementation, parity unpinned.  The plan (periods,
 * bin counts, log constants) and the constant tables are host logic (visualisation/acoustic_analysis.py builds them
 * with numpy); the difference function is exact integer arithmetic on the int16 samples.  One decoded state per frame
 * (state < n_pitch_bins: voiced, f0 = fmin 2^(state / bins_per_octave)) and the voiced probability. */
typedef struct pce_pyin_plan {
    int32_t frame_length, hop_length, min_period, max_period, n_pitch_bins, trans_width, n_thresholds, reserved;
    double sr, fmin, bins_per_octave, no_trough_prob, log_tiny, log_p_init, tiny;
} pce_pyin_plan;
int pce_pyin_run(pce_ctx *ctx, const pce_pyin_plan *plan, const double *tables, int64_t n_tables);
int pce_pyin_shape(pce_ctx *ctx, int32_t clip, int64_t *n_frames);
/* states [n_frames] / voiced_prob [n_frames] / status (bit 0: a frame had more troughs than the engine keeps) may be NULL */
int pce_pyin_fetch(pce_ctx *ctx, int32_t clip, int32_t *states, double *voiced_prob, int32_t *status);
/* Test hooks of the two pYIN kernels.  An observation list is a row of PCE_PYIN_MAX_TROUGHS entries per frame, of which the first n[frame] count.
 * pce_pyin_fetch_observations: what k_pyin_frames left for `clip` in the last pce_pyin_run, per frame: n, status (1: more troughs than the engine keeps),
 * voiced_prob, log_unvoiced = log((1 - voiced_prob) / n_pitch_bins + tiny), and the voiced observations in trough (lag) order: bins [n_frames][512] and
 * log_probs [n_frames][512] = log(p + tiny); entries at and beyond n[frame] keep the caller's values.  Every output may be NULL.
 * pce_selftest_pyin_viterbi: k_pyin_viterbi on the caller's lists, through the launch of pce_pyin_run (same grid, block and LDS) and under its plan checks,
 * in buffers of its own (a resident run is left as it is; no batch need be uploaded).  n_clips >= 1 clips, clip i holding frames frame_off[i] ..
 * frame_off[i + 1] (frame_off[0] == 0, a clip may be empty); n, log_unvoiced, states_out [frames]; bins, log_probs [frames][512].  PCE_E_INVALID for
 * n outside 0 .. 512, a bin outside 0 .. n_pitch_bins - 1 or twice in one frame.  states_out: the decoded state of every frame.  Since minor 22. */
#define PCE_PYIN_MAX_TROUGHS 512
int pce_pyin_fetch_observations(pce_ctx *ctx, int32_t clip, int32_t *n, int32_t *status, double *voiced_prob, double *log_unvoiced, int32_t *bins,
                                double *log_probs);
int pce_selftest_pyin_viterbi(pce_ctx *ctx, const pce_pyin_plan *plan, const double *tables, int64_t n_tables, int32_t n_clips, const int64_t *frame_off,
                              const int32_t *n, const double *log_unvoiced, const int32_t *bins, const double *log_probs, int32_t *states_out);

/* ---- CREPE pitch tracking ----------------------------------------------------
 * Replaces torchcrepe.predict(audio, sr, hop, fmin, fmax, model, batch_size=..., return_periodicity=True) of Code/Pipeline/evaluate_voice.ipynb
 * (extract_f0_torchcrepe).  torchcrepe is third party and absent: restated from its published implementation, parity unpinned; no trained
 * weights are on hand either (the loader takes a user's own full.pth / tiny.pth through crepe_weights.py).  Per frame of 1024 samples at 16 kHz
 * (the batch padded by 512 zeros on both sides, frame t = samples [t hop, t hop + 1024), 1 + n / hop frames; mean removed, divided by
 * max(1e-10, unbiased std)): six blocks of zero padding (block 1: 254 + 254, others 31 + 32), convolution with bias (block 1: 512 taps, stride 4;
 * others 64 taps), ReLU, BatchNorm in inference form as (scale, shift), max-pool 2; the last activation flattened time-major then channel; Linear to
 * 360 bins, sigmoid = the salience.  Convolutions are GEMMs on MFMA with fp16 operands and fp32 accumulation over padded time-major images; every
 * stored activation is fp16, the classifier's weights and the salience fp32.
 *
 * Weight blob (float32), per block i = 1..6: conv weight [c_out][taps][c_in] (PyTorch's [c_out][c_in][taps][1] transposed), bias [c_out],
 * scale [c_out], shift [c_out]; then classifier weight [360][4 c_out[5]], classifier bias [360] (crepe_weights.py:tensor_order / fold).
 * Limits (else PCE_E_LIMIT at load): c_out[0] % 64 == 0, every c_out % 16 == 0, 4 c_out[5] % 256 == 0 and <= 4096.  The kernel of a block is
 * chosen by its N = c_out alone (N % 128 == 0: 128-column tiles, else 16-column tiles), never by the number of frames: a frame's results do not
 * depend on the chunk size or on what its clip is batched with, bit for bit.
 *
 * pce_crepe_run: the resident batch must be at 16 kHz (PCE_E_INVALID otherwise; PCE_E_STATE before pce_crepe_load).  Frames run in chunks of
 * frames_per_chunk (chunks span clip boundaries), clamped so that a chunk's activation images stay within PCE_CREPE_IMAGE_BUDGET bytes.
 * Decoding (torchcrepe.postprocess without its dither): salience bins outside [lo, hi) are masked; decoder 0 = Viterbi of
 * librosa.sequence.viterbi on the softmax of the masked salience, transition max(12 - |i - j|, 0) row-normalised, uniform initial state,
 * log(p + tiny), fp64, first maximum; decoder 1 = per-frame arg-max (first maximum).  f0 = 10 * 2^((20 bin + 1997.3794084376191) / 1200),
 * periodicity = salience[t][bin]. */
#define PCE_CREPE_BINS 360
#define PCE_CREPE_IMAGE_BUDGET ((int64_t)3 << 30)
typedef struct pce_crepe_dims { int32_t c_out[6]; int32_t reserved[2]; } pce_crepe_dims;
typedef struct pce_crepe_plan { int32_t hop, lo, hi, decoder, frames_per_chunk, reserved; } pce_crepe_plan;
int pce_crepe_load(pce_ctx *ctx, const pce_crepe_dims *dims, const float *weights, int64_t n_floats);
int pce_crepe_run(pce_ctx *ctx, const pce_crepe_plan *plan);
int pce_crepe_shape(pce_ctx *ctx, int32_t clip, int64_t *n_frames);
/* bins [n_frames] / f0 [n_frames] / periodicity [n_frames] / salience [n_frames][360]: any may be NULL */
int pce_crepe_fetch(pce_ctx *ctx, int32_t clip, int32_t *bins, double *f0, float *periodicity, float *salience);
/* One block (1..6) as pce_crepe_run launches it, on host arrays of fp16 bit patterns: x [n_frames][t_in][c_in] (block 1: t_in = 1024, c_in = 1;
 * block b >= 2: t_in = 128 >> (b - 2)), w [c_out][taps][c_in]; out [n_frames][t_in / 2 (block 1: 128)][c_out] =
 * fp16(max over row pairs of relu(acc + bias) * scale + shift). */
int pce_selftest_crepe_layer(pce_ctx *ctx, int32_t block, int32_t c_in, int32_t c_out, int32_t n_frames, const uint16_t *x, const uint16_t *w,
                             const float *bias, const float *scale, const float *shift, uint16_t *out);
/* The decoding of pce_crepe_run on a host salience [n_frames][360] taken as ONE clip (any float values: the decoder takes the softmax of what it
 * is given); bins / f0 / periodicity [n_frames], any may be NULL.  Overwrites the results of the last pce_crepe_run. */
int pce_selftest_crepe_decode(pce_ctx *ctx, const float *salience, int32_t n_frames, int32_t lo, int32_t hi, int32_t decoder, int32_t *bins, double *f0,
                              float *periodicity);

/* ---- R8: log-mel spectrogram + Whisper audio encoder --------------------
 * Replaces the device work of whisper_timestamped.transcribe before decoding
 * (Code/Aligners/use_whisper_timestamped.py:139,150-163; openai-whisper==20240930):
 * whisper.log_mel_spectrogram on the 30 s window starting at sample 0 of every
 * uploaded clip (16 kHz; shorter clips are zero padded, as whisper.pad_or_trim
 * does), then AudioEncoder.forward.  Matmuls run on MFMA in the context's
 * operand mode (pce_whisper_set_operands; default: fp16 operands and an fp16
 * residual stream, openai-whisper's own fp16 arithmetic) with fp32 accumulation
 * and fp32 LayerNorm / softmax statistics.
 *
 * Weight blob (float32, this order; Linear/Conv weights in PyTorch layout):
 *   conv1.weight[d][n_mels][3] conv1.bias[d] conv2.weight[d][d][3] conv2.bias[d]
 *   per layer: attn_ln.w[d] attn_ln.b[d] query.w[d][d] query.b[d] key.w[d][d]
 *              value.w[d][d] value.b[d] out.w[d][d] out.b[d] mlp_ln.w[d] mlp_ln.b[d]
 *              mlp.0.w[4d][d] mlp.0.b[4d] mlp.2.w[d][4d] mlp.2.b[d]
 *   ln_post.w[d] ln_post.b[d]
 * The sinusoidal positional embedding is generated inside the library. */
typedef struct pce_whisper_dims {
    int32_t n_mels;    /* 80 (128 for large-v3)          */
    int32_t n_ctx;     /* 1500                            */
    int32_t n_state;   /* d: 384/512/768/1024/1280; d % 128 == 0, d <= 2048 (the LayerNorm kernels), and where d % 256 == 0 the
                        * persistent GEMM runs fc1 (N = 4 d <= 6144): d <= 1536, unless the context was created with PCE_GEMM_FLAT=0.
                        * Other widths are PCE_E_LIMIT at load. */
    int32_t n_head;    /* d / 64                          */
    int32_t n_layer;
} pce_whisper_dims;
int pce_logmel_run(pce_ctx *ctx, int32_t n_mels);
/* window variant (whisper.transcribe slices the log-mel of the WHOLE recording, followed by 30 s of zeros, at its seek
 * position): frames start_frames[clip] .. +2999 of that spectrogram, samples beyond 30 s included, the max - 8 clamp from
 * the maximum over the whole recording.  start_frames[clip] * 160 must not exceed the clip length. */
int pce_logmel_run_at(pce_ctx *ctx, int32_t n_mels, const int64_t *start_frames /* [clips] */);
int pce_logmel_fetch(pce_ctx *ctx, int32_t clip, float *out /* [n_mels][3000] */);
/* Self-test, read-only: the time-major image [3002][n_mels] of `clip` that the last pce_logmel_run / pce_logmel_run_at left for the conv stem, as bit
 * patterns of the context's operand type (bf16 or fp16): rows 1 .. 3000 are frames 0 .. 2999, rows 0 and 3001 the stem's zero padding.  Nothing is
 * launched and nothing written: the copy shows what the encoder would read.  PCE_E_STATE before a run (of the selected operand build), PCE_E_INVALID
 * for a clip outside the run's batch.  Since minor 18. */
int pce_selftest_logmel_image(pce_ctx *ctx, int32_t clip, uint16_t *out /* [3002][n_mels] */);
int pce_whisper_load(pce_ctx *ctx, const pce_whisper_dims *dims, const float *weights, int64_t n_floats);
int pce_whisper_encode_run(pce_ctx *ctx);
/* Self-test of the GEMM kernel the encoder's projections run on (persistent 256 x 256 tiles, csrc/pce_gemm256.inc) on host arrays of bf16 bit
 * patterns: C = epilogue(A[M][K] B[N][K]^T + bias).  epilogue 0: bias; 1: bias + exact GELU; 2: bias, written transposed per clip
 * (rows_per_clip rows each, key axis padded to vt_sp): out[(clip N + n) vt_sp + t].  N % 256 == 0, K % 64 == 0. */
int pce_selftest_gemm(pce_ctx *ctx, const uint16_t *A, const uint16_t *B, const float *bias, int32_t M, int32_t N, int32_t K, int32_t epilogue,
                      int32_t rows_per_clip, int32_t vt_sp, uint16_t *out);
/* The same kernel with its residual epilogue, in place as the encoder's attention projection and fc2 run it on the 16-bit residual stream:
 * resid_inout[M][N] = r16(resid_inout + r16(A B^T + bias)) (r16: rounding to the context's 16-bit operand type; bit patterns in and out). */
int pce_selftest_gemm_resid(pce_ctx *ctx, const uint16_t *A, const uint16_t *B, const float *bias, uint16_t *resid_inout, int32_t M, int32_t N, int32_t K);
/* Self-test of the attention kernel (64-wide heads; csrc/pce_attention.inc k_attention_lean16) on host arrays of bf16 bit patterns: clips x
 * heads independent problems, q [clips][q_len][heads * 64], k and v [clips][k_len][heads * 64], out like q; softmax(q k^T / 8) v with the
 * causal mask when causal != 0.  mode 0: the kernel as the engine runs it (fixed softmax reference, exact fallback), 1: its exact
 * path only.  *fell_back (may be NULL): number of workgroups that had to take the exact path (mode 0). */
int pce_selftest_attention(pce_ctx *ctx, const uint16_t *q, const uint16_t *k, const uint16_t *v, int32_t clips, int32_t heads, int32_t q_len,
                           int32_t k_len, int32_t causal, int32_t mode, uint16_t *out, int32_t *fell_back);
/* The same kernel with per-clip lengths, through the launch the teacher-forced decoder makes (grid of the longest clip; one query block takes the
 * streaming instantiation): the rows of the clips lie back to back, q [sum q_len][heads * 64], k and v [sum k_len][heads * 64], q_len / k_len [clips]
 * >= 1.  out [out_rows][heads * 64], out_rows >= sum q_len, is read and written back whole: rows no query owns keep the caller's values.
 * pce_selftest_attention is this call with equal lengths and a zeroed out.  Since minor 8. */
int pce_selftest_attention_ragged(pce_ctx *ctx, const uint16_t *q, const uint16_t *k, const uint16_t *v, int32_t clips, int32_t heads, const int32_t *q_len,
                                  const int32_t *k_len, int32_t causal, int32_t mode, uint16_t *out, int64_t out_rows, int32_t *fell_back);
/* Self-test of the single-query attention kernels of an incremental decoding step (one query per clip and head, 64-wide heads, d = heads * 64) on
 * host arrays of 16-bit patterns of the context's operand type, through the launches the decoding step makes (head groups of at most 16 waves).
 *   form 0: k_cross_attn1w over given keys.  q [n][d]; k: key rows [.][d], clip i reads rows k_row0[i] .. + len[i]; v: the V^T image [n][d][span]
 *           WHOLE, padding columns included (span = its pitch, a multiple of 8; columns >= len[i] must be finite); 1 <= len[i] <= 1536.
 *   form 1: k_cross_attn1w appending.  q = q | k | v of the new position [n][3 d]; k: K cache [n][span][d]; v: V^T cache [n][d][512]; len[i] = the
 *           position (row / column the new key / value are written to; keys 0 .. len[i] are attended to); span = T_cap <= 512.  k_row0 unused.
 *   form 2: k_self_attn1w.  As form 1 with v: the row-major V cache [n][span][d].
 * skip [n] (may be NULL): a clip with skip != 0 is left alone.  out [n][d] is read and written back whole, and in forms 1 and 2 so are k and v (the
 * caches after the call): what a launch does not write keeps the caller's values.  PCE_E_INVALID, before anything is launched, for more than 32
 * heads, len out of range (form 0: < 1, > 1536 or past the image's pitch; forms 1 / 2: < 0 or >= span), span > 512 in forms 1 / 2, and arrays
 * (q_elems, k_elems, v_elems, out_elems: their lengths in elements) shorter than the shape needs.  Since minor 8. */
int pce_selftest_attn1(pce_ctx *ctx, int32_t form, int32_t n, int32_t heads, const uint16_t *q, int64_t q_elems, uint16_t *k, int64_t k_elems, uint16_t *v,
                       int64_t v_elems, const int32_t *k_row0, const int32_t *len, const int32_t *skip, int32_t span, uint16_t *out, int64_t out_elems);
/* Self-test of the forced alignment's matrix kernels (k_align_scores, k_align_colnorm, k_align_cost) on host arrays, through the launches and the
 * padding code of pce_whisper_align_run: n clips, 64-wide heads, d = heads * 64.  q [n][T_pad][d] (the decoder's cross-attention queries) and
 * k [n][k_rows][d] (audio keys; placed at the 1500-row pitch per clip the kernel assumes, k_rows >= every f_len) as 16-bit patterns of the context's
 * operand type; t_len / f_len [n]: tokens and frames per clip; heads_sel [n_sel]: the selected heads in the order of their slices (any order, repeats
 * allowed); T_pad = max t_len rounded up to 16, F_pad = max f_len rounded up to 64, N_max = max t_len - sot_len - 1.  The scores are launched once
 * for all selected heads (split == 0 or == n_sel) or twice as two layers would be: heads_sel[0 .. split) with sel0 = 0, then the rest with
 * sel0 = split.  The kernel's score scale is 0.125f * qk_scale (fp32 product), as in pce_whisper_align_run.
 *   w_soft [n][n_sel][T_pad][F_pad] fp32: softmax over s < f_len of q_t . k_s, after the score launches;
 *   w_norm, same shape: the same buffer after the in-place normalisation over t < t_len;
 *   cost [n][N_max][F_pad] fp64: -mean over heads of the median filter over time, rows t = sot_len .. t_len - 2.
 * w_soft and cost are read and written back whole: what no launch writes keeps the caller's values (in w_norm: the values w_soft came in with).
 * PCE_E_INVALID, before anything is launched, for what pce_whisper_align_run refuses (t_len < sot_len + 2 or > 448, f_len < 1, an even
 * medfilt_width or one above 15), f_len > 1500 or > k_rows, a selected head outside 0 .. heads - 1, more than 32 heads, split outside 0 .. n_sel and
 * arrays (q_elems, k_elems, w_soft_elems, w_norm_elems, cost_elems: their lengths in elements) shorter than the shape needs.  A context created
 * with PCE_ALIGN_GENERIC_MEDIAN set takes the insertion-sort filter at width 7 here as in the run.  Since minor 14. */
int pce_selftest_align_matrix(pce_ctx *ctx, int32_t n, int32_t heads, const uint16_t *q, int64_t q_elems, const uint16_t *k, int64_t k_elems, int32_t k_rows,
                              const int32_t *t_len, const int32_t *f_len, const int32_t *heads_sel, int32_t n_sel, int32_t split, int32_t sot_len,
                              int32_t medfilt_width, float qk_scale, float *w_soft, int64_t w_soft_elems, float *w_norm, int64_t w_norm_elems, double *cost,
                              int64_t cost_elems);
/* Self-test of the cross-attention of an incremental decoding step from the ENCODER OUTPUT (csrc/pce_xattn.inc: LayerNorm + query projection + Q' = q Wk,
 * one streaming pass over E with an online softmax per leaf of frames, the merge tree, out = Wv U + bv) for ONE layer on host arrays: resid [n][d] fp32,
 * ln_w / ln_b / bq / bv [d] fp32, wq / wk / wv [d][d] and E [n][k_cap][d] as 16-bit patterns of the context's operand type (rows of the weights = output
 * features; Whisper's key projection has no bias), k_len[n] valid frames per clip.  d in {128, 256, 384, 512, 768, 1024, 1280}, heads = d / 64.
 * workgroups_per_clip: 0 = what the batch size selects, or 1 / 2 / 4 -- the result must not depend on it (the frames are always cut into the same four
 * leaves and merged in the same tree).  d = 1280 with 20 heads (large-v3 / turbo) since minor 4.  out [n][d]: 16-bit patterns. */
int pce_selftest_xattn(pce_ctx *ctx, const float *resid, const float *ln_w, const float *ln_b, const uint16_t *wq, const float *bq, const uint16_t *wk,
                       const uint16_t *wv, const float *bv, const uint16_t *E, const int32_t *k_len, int32_t n, int32_t k_cap, int32_t d, int32_t heads,
                       int32_t workgroups_per_clip, uint16_t *out);
/* pce_selftest_xattn stage by stage: the same launch (k_xq_fused -> k_xattn_absorbed -> k_uv_absorb through the product's launch code), with the list of
 * ended clips and the buffers the launch writes between its kernels copied out.  Operands as pce_selftest_xattn; E holds e_elems >= n k_cap d elements.
 *   skip [n] (may be NULL): a clip with skip != 0 is left alone by all three kernels.
 *   out [n][d] (out_elems >= n d), 16-bit patterns.
 *   qp_hi, qp_lo [n][R][d] (qp_elems >= n R d each), R = heads rounded up to 16: Q'_h = (log2 e / 8) q_h Wk_h as a hi + lo pair of the operand type; rows
 *           >= heads are never written.
 *   u_part [n][nodes][R][d] fp32 and ml_part [n][nodes][R][2] fp32 (u_elems / ml_elems: at least that many): per node of the merge tree, over its frames t,
 *           U = sum_t 2^(s_t - m) E[t], the reference m and l = sum_t 2^(s_t - m), s_t = Q' . E[t].  *nodes_out (may be NULL) receives nodes: 4 where the
 *           launch wrote the four leaves (leaf i = tiles [i per, (i + 1) per) of the ceil(k_len / 16) 16-frame tiles, per = ceil(tiles / 4); an empty
 *           leaf is m = -1e30, l = 0, U = 0), 2 where it wrote the pair nodes L0 + L1 and L2 + L3 (d <= 768 with 1 or 2 workgroups per clip).  Rows >= heads
 *           are never written.  Arrays sized for 4 nodes always suffice; only the first n nodes R d (n nodes R 2) elements are used.
 * qp_hi / qp_lo and u_part / ml_part may be NULL in pairs (not copied out).  out, qp_hi, qp_lo, u_part and ml_part are read and written back whole (the
 * used part): the caller's values are uploaded first, and what no launch writes keeps them.  PCE_E_INVALID, before anything is launched, for what
 * pce_selftest_xattn refuses and for arrays shorter than the shape needs.  pce_selftest_xattn is this call with skip = NULL, a zeroed out and no stage
 * outputs.  Since minor 19. */
int pce_selftest_xattn_stages(pce_ctx *ctx, const float *resid, const float *ln_w, const float *ln_b, const uint16_t *wq, const float *bq, const uint16_t *wk,
                              const uint16_t *wv, const float *bv, const uint16_t *E, int64_t e_elems, const int32_t *k_len, const int32_t *skip, int32_t n,
                              int32_t k_cap, int32_t d, int32_t heads, int32_t workgroups_per_clip, uint16_t *out, int64_t out_elems, uint16_t *qp_hi,
                              uint16_t *qp_lo, int64_t qp_elems, float *u_part, int64_t u_elems, float *ml_part, int64_t ml_elems, int32_t *nodes_out);
/* Self-test of the tiled / few-row GEMM kernels the convolutions, the teacher-forced decoder, the decoding steps, BERT and the vocabulary logits run
 * on, through the product's own launch code: C = epilogue(A B^T + bias) for `batch` problems, A [batch] rows of K at pitch lda (a_batch apart; rows may
 * overlap: lda < K), B [N][K] and A as 16-bit patterns of the context's operand type, bias [N] fp32 (may be NULL).  epilogue 0: bias, 16-bit C;
 * 1: bias + exact GELU, 16-bit C; 2: GELU(bias + .) + pos[row % pos_T][n], fp32 C (pos [pos_T][N]); 3: C += . + bias, fp32 (C is read);
 * 4: columns [0, v_col0) as epilogue 0, columns [v_col0, N) written transposed to vt[(clip (N - v_col0) + n - v_col0) vt_sp + t], clip = row /
 * rows_per_clip, t = row % rows_per_clip (batch 1); 5: bias, fp32 C.  C [c_len] (element type of the epilogue) is read and written back, with
 * vt [vt_len]: what a launch does not write keeps the caller's values.  kernel: 0 = what the product's rule picks outside an incremental
 * decoding step, 1 = the few-row kernel, 2 = 128 x 256, 3 = 128 x 128 two-stage, 4 = 128 x 128 four-stage; *kernel_used (may be NULL) receives
 * the kernel that ran.  PCE_E_LIMIT where that kernel does not compute the shape (N % 128, K % 64 for 128 x 128; N % 256, K % 32 for 128 x 256;
 * batch 1, N % 32, K % 256, M <= 1024, N <= 4096 and epilogues 0 / 1 / 3 for the few-row kernel); PCE_E_INVALID where a launch would address
 * beyond a_len, c_len or vt_len.  Since minor 5. */
int pce_selftest_gemm_tiled(pce_ctx *ctx, int32_t kernel, int32_t epilogue, const uint16_t *A, int64_t a_len, int64_t lda, int64_t a_batch, int32_t batch,
                            const uint16_t *B, const float *bias, int32_t M, int32_t N, int32_t K, void *C, int64_t c_len, int64_t ldc, int64_t c_batch,
                            const float *pos, int32_t pos_T, int32_t v_col0, int32_t rows_per_clip, int32_t vt_sp, uint16_t *vt, int64_t vt_len,
                            int32_t *kernel_used);
/* Self-test of the LayerNorm kernels as the product launches them, rows x d (d % 4 == 0, d <= 2048), w / b [d] fp32.  form 0 / 1: LayerNorm of x
 * (fp32) to out (fp32 / 16-bit); flags bit 0: x is taken as rounded to 16 bits, bit 1: the fp32 result is also written over x (returned in
 * resid_out).  form 2 + 3 o + s: x (+ delta) (+ delta2), then LayerNorm -- out fp32 (o = 0) or 16-bit (o = 1); s = 0: x and the stream fp32,
 * 1: x fp32, the stream 16-bit, 2: x and the stream 16-bit (every sum rounded to 16 bits where the stream is); delta / delta2 [rows][d] 16-bit
 * (delta2 may be NULL); flags bit 2: the stream is written (resid_out receives the stream buffer, rows x d of its type); out_copy (may be NULL):
 * a 16-bit copy of the output.  Since minor 5. */
int pce_selftest_layernorm(pce_ctx *ctx, int32_t form, int32_t rows, int32_t d, const void *x, const uint16_t *delta, const uint16_t *delta2, const float *w,
                           const float *b, float eps, int32_t flags, void *out, void *resid_out, uint16_t *out_copy);
/* Self-test of the encoder layer walk that Whisper's audio encoder on the tiled kernels, BERT and wav2vec2 share: n_layers (1 or 2) layers over
 * M = n_items x rows_per_item rows of width d, item i holding len[i] rows from row i x rows_per_item, through the code the product runs (the loaders' weight
 * packer and upload, the callers' run description, the walk itself).  pre_ln 1: x += proj(MHA(LN1 x)); x += W2 gelu(W1 LN2 x); 0: x = LN1(x + proj(MHA x));
 * x = LN2(x + W2 gelu(W1 x)), each LayerNorm written to the stream and to its 16-bit image.  gemm_rule 0: the product's kernel choice, 1: wav2vec2's.
 * weights: the layers one after the other, fp32, PyTorch layouts -- pre_ln 1 with gemm_rule 0 (the Whisper encoder) in openai-whisper's order
 *   ln1.w,b  q.w,b  k.w [k.b]  v.w,b  out.w,b  ln2.w,b  fc1.w,b  fc2.w,b,
 * every other form in transformers' (q.w,b  k.w [k.b]  v.w,b  out.w,b  ln1.w,b  fc1.w,b  fc2.w,b  ln2.w,b); k.b only with key_bias.  stream [M][d] fp32: the
 * stream on entry; ln_in [M][d]: the 16-bit image the caller's opening LayerNorm leaves (pre_ln 0; else ignored, may be NULL).  Behind every launch the
 * buffer it wrote is copied, per layer l, to
 *   ln16 [l][3][M][d]   the LayerNorm image behind LN1 in front of the attention (slot 0, pre_ln 1), behind the LayerNorm in front of fc1 (1) and behind the layer's
 *                       last (2, pre_ln 0);
 *   qk [l][M][2 d], vt [l][n_items][d][vt_sp]  Q | K and the whole V^T image (zeroed once before the first layer, as every caller zeroes it);
 *   attn [l][M][d], hidden [l][M][inner]       the attention's output, gelu(fc1);
 *   x32 [l][4][M][d]    the fp32 stream behind the output projection (0), behind the LayerNorm in front of fc1 (1, pre_ln 0), behind fc2 (2) and behind the
 *                       layer's last LayerNorm (3, pre_ln 0).
 * All six are uploaded first and fetched back whole: what no launch writes keeps the caller's values, and the run's own buffers start with what the
 * caller's arrays hold for layer 0 (so attention rows at and behind len[i] keep them in every layer).  16-bit arrays are bit patterns of the context's
 * operand type.  *fit_out (may be NULL): whether every product was launched.  PCE_E_LIMIT for what the loaders refuse (d % 128, heads x 64 != d,
 * d > 2048, inner % 128), PCE_E_INVALID for len[i] outside 1 .. rows_per_item, rows_per_item > vt_sp (or % 4, or vt_sp % 64), a weight blob of another
 * size and arrays shorter than the shape needs -- all before anything is launched.  Since minor 26. */
int pce_selftest_encoder_walk(pce_ctx *ctx, int32_t pre_ln, int32_t gemm_rule, int32_t key_bias, int32_t d, int32_t heads, int32_t inner, int32_t n_layers,
                              int32_t n_items, int32_t rows_per_item, int32_t vt_sp, const int32_t *len, float eps, const float *weights, int64_t n_floats,
                              const float *stream, int64_t stream_elems, const uint16_t *ln_in, uint16_t *ln16, int64_t ln16_elems, uint16_t *qk, int64_t qk_elems,
                              uint16_t *vt, int64_t vt_elems, uint16_t *attn, int64_t attn_elems, uint16_t *hidden, int64_t hidden_elems, float *x32,
                              int64_t x32_elems, int32_t *fit_out);
int pce_whisper_encode_fetch(pce_ctx *ctx, int32_t clip, float *out /* [1500][n_state] */);

/* ---- R8: forced alignment of known text tokens (teacher-forced decoder + cross-attention DTW) ----
 * openai-whisper timing.py find_alignment, the mechanism whisper_timestamped's word timestamps rest on
 * (Code/Aligners/use_whisper_timestamped.py:163): TextDecoder.forward over the given token sequence
 * (sot sequence, no-timestamps, text tokens, eot), cross-attention logits of the alignment heads ->
 * softmax over the first num_frames/2 audio positions -> std/mean normalisation over tokens -> median filter
 * over time -> mean over heads -> DTW of -matrix[sot_len:-1].  Token ids -> words is tokenizer (host) logic.
 * Needs pce_whisper_encode_run on the same batch.  Decoder weight blob (float32, PyTorch layouts):
 *   token_embedding[n_vocab][d] positional_embedding[n_text_ctx][d]
 *   per layer: attn_ln.w,b  attn.{query.w,query.b,key.w,value.w,value.b,out.w,out.b}
 *              cross_attn_ln.w,b  cross_attn.{query.w,query.b,key.w,value.w,value.b,out.w,out.b}
 *              mlp_ln.w,b  mlp.0.w,b  mlp.2.w,b
 *   ln.w,b */
typedef struct pce_whisper_text_dims {
    int32_t n_vocab /* <= 52224 */, n_text_ctx /* <= 448 */, n_state, n_head /* <= 32 (n_state <= 2048): more is PCE_E_LIMIT */, n_layer;
} pce_whisper_text_dims;
int pce_whisper_decoder_load(pce_ctx *ctx, const pce_whisper_text_dims *dims, const float *weights, int64_t n_floats);
/* tokens: concatenated per clip (token_offsets[n_clips+1]); num_frames: mel frames of real audio per clip;
 * head_mask: [n_layer * n_head] bytes or NULL (all heads of the last half of the layers, whisper's default) */
int pce_whisper_align_run(pce_ctx *ctx, const int32_t *tokens, const int32_t *token_offsets, const int32_t *num_frames,
                          int32_t sot_len, const uint8_t *head_mask, int32_t medfilt_width, float qk_scale);
int pce_whisper_align_shape(pce_ctx *ctx, int32_t clip, int32_t *n_rows, int32_t *n_cols);
/* path arrays hold up to n_rows + n_cols entries; cost (nullable) is the [n_rows][n_cols] fp64 DTW input */
int pce_whisper_align_fetch(pce_ctx *ctx, int32_t clip, int32_t *text_idx, int32_t *time_idx, int32_t *path_len, double *cost);
/* Every clip's path of the last pce_whisper_align_run at once, asynchronously (the form a batch pipeline uses: what
 * whisper_timestamped hands back per segment, Code/Aligners/use_whisper_timestamped.py:163, for all utterances of the batch).
 * _enqueue queues the device-to-host copies behind the alignment on the context's stream into pinned staging memory and returns at
 * once (*n_clips, *path_stride = max rows + max columns of the batch: the row pitch of the index arrays); _wait blocks on those
 * copies only and writes path_len[n_clips] and the first path_len[i] entries of text_idx / time_idx [n_clips][path_stride] (either may
 * be NULL).  slot is 0 or 1 (two batches in flight); _enqueue on a slot whose previous fetch has not been waited for is PCE_E_STATE (its
 * copies may still be landing in the staging buffer).  The same indices as pce_whisper_align_fetch clip by clip. */
int pce_whisper_align_paths_enqueue(pce_ctx *ctx, int32_t slot, int32_t *n_clips, int32_t *path_stride);
int pce_whisper_align_paths_wait(pce_ctx *ctx, int32_t slot, int32_t *path_len, int32_t *text_idx, int32_t *time_idx);

/* ---- R8: free-running decoding, one step -------------------------------------
 * openai-whisper decoding.py at temperature 0 (a default DecodingTask with a GreedyDecoder, what whisper_timestamped's
 * transcribe runs first: Code/Aligners/use_whisper_timestamped.py:150-163): the text decoder over the sequences so far,
 * the logits of the last position through the tied output projection, the logit filters SuppressBlank / SuppressTokens /
 * ApplyTimestampRules and the arg-max (first maximum; a sequence whose last token is end-of-text stays there).
 * vocab_mask[n_vocab]: bit 0 = always suppressed (the suppress list and <|notimestamps|>), bit 1 = suppressed at the
 * first sampled position (the blank token and end-of-text).  The prompt (<|startoftranscript|><|fr|><|transcribe|>),
 * the loop and the stopping rule are host logic (Aligners/decoding.py); token ids in, token ids out (text needs the
 * checkpoint's vocabulary).  The cross-attention K / V of all layers are computed at the first step after
 * pce_whisper_encode_run and kept. */
typedef struct pce_whisper_decode_rules { int32_t eot, timestamp_begin, max_initial_timestamp_index /* < 0: none */, reserved; } pce_whisper_decode_rules;
int pce_whisper_decode_step(pce_ctx *ctx, const int32_t *tokens, const int32_t *token_offsets /* [clips + 1] */, int32_t sample_begin,
                            const pce_whisper_decode_rules *rules, const uint8_t *vocab_mask, int32_t *next_tokens /* [clips] */,
                            float *next_logprobs /* [clips] or NULL: log-probability of the choice under the filtered distribution (sum_logprobs) */);
/* The same step with the per-sequence controls whisper.transcribe needs around it (transcribe.py decode_with_fallback,
 * decoding.py DecodingTask): every sequence has its own prompt length (condition_on_previous_text prepends
 * <|startofprev|> + the previous windows' text), a temperature > 0 draws ONE sample from softmax(filtered logits /
 * temperature) as GreedyDecoder does (Gumbel-max over a counter-based generator keyed by (seed, clip, position): the
 * same call gives the same draw), and probe_token >= 0 also returns softmax(UNFILTERED logits of the last
 * position)[probe_token] -- run on the prefix that ends at <|startoftranscript|> this is no_speech_prob.
 * next_logprobs stays the log-probability at temperature 1 under the filtered distribution (sum_logprobs).
 * Sequences of different lengths keep their self-attention K / V cache: a call whose every prefix extends the
 * previous call's by exactly one token appends one position per sequence. */
typedef struct pce_whisper_decode_opts {
    const int32_t *sample_begin;   /* [clips] first sampled position of every sequence, or NULL: sample_begin_all for all */
    int32_t sample_begin_all;
    float temperature;             /* 0: arg-max (first maximum) */
    uint32_t seed_lo, seed_hi;
    int32_t probe_token;           /* < 0: no probe */
    int32_t flags;                 /* bit 0: do not use the self-attention K / V cache (re-run the decoder over the whole prefix: the check of the cache) */
} pce_whisper_decode_opts;
int pce_whisper_decode_step_ex(pce_ctx *ctx, const int32_t *tokens, const int32_t *token_offsets /* [clips + 1] */,
                               const pce_whisper_decode_rules *rules, const uint8_t *vocab_mask, const pce_whisper_decode_opts *opts,
                               int32_t *next_tokens /* [clips] */, float *next_logprobs /* [clips] or NULL */,
                               float *probe_prob /* [clips] or NULL */);

/* What the sampling noise of a clip is keyed by.  The draw at temperature > 0 is a function of (seed, key, position, token); without this
 * call the key is the clip's position in the encoded batch, so the same recording samples differently when it is batched with other
 * clips (another shard of a multi-rank run, another batch size).  keys[i]: any int32 that names clip i wherever it is batched (the mirror's
 * transcribe() passes a hash of the clip's samples and its window start); they hold for the batch now encoded -- the next
 * pce_whisper_encode_run drops them -- and n must be that batch's clip count (n = 0: drop them now).  PCE_E_STATE before an encoder run. */
int pce_whisper_sample_keys(pce_ctx *ctx, const int32_t *keys /* [n] */, int32_t n);

/* Self-test of the kernels that turn a decoding step's logits into tokens (k_decode_rules: vocabulary mask, blank and timestamp rules, the
 * timestamp-mass rule, first arg-max or Gumbel sampling, log-probability, probe) and carry them into the device-resident loop's tables
 * (k_step_advance), on host arrays through the launches pce_whisper_decode_step_ex and pce_whisper_decode_loop make; no model need be loaded.
 * logits [steps][n][ld] fp32, ld = n_vocab rounded up to 128 (the padding columns travel as given); tokens / token_offsets [n + 1]: the sequences so
 * far; sample_begin [n], or NULL: sample_begin_all for all; rules, vocab_mask [n_vocab], temperature, seed, probe_token (< 0: none) and
 * sample_keys [n] (or NULL: the batch position) as in pce_whisper_decode_step_ex / pce_whisper_sample_keys.  t_cap (1..448): the text context.
 *   form 0: one step (steps == 1) as pce_whisper_decode_step_ex launches it: the sequences as rows of T_pad ids (the longest rounded up to 16), entries
 *           past a sequence's length = pad_token.  out_tok / out_lp / probe_prob [out_elems >= n]: next token, its log-probability, the probe.
 *   form 1: the loop as pce_whisper_decode_loop runs it, probe-less: table [n][t_cap] receives the sequences (entries past their lengths keep the
 *           caller's values); for s = 0 .. steps - 1 (steps <= max_new) the rules on logits[s], then k_step_advance.  out_tok / out_lp [n][max_new];
 *           table: the final one; loop_state: len [n] | ended [n] | ct [8 n] (new token | . | . | . | key count | . | . | position) |
 *           n_ended [max_new] | step counter -- len, n_ended and the counter are initialised here (the lengths; zero), ended and ct start
 *           from the caller's values.
 * Every output is read and written back whole: what no launch writes keeps the caller's values.  The log-probability is the filtered, unscaled
 * log-softmax at the choice, computed as -log(sum exp(x - x[choice])): it is -inf when a sampled choice lies more than about 88 below the maximum.
 * PCE_E_INVALID, before anything is launched, for what the decoding calls refuse (eot / timestamp_begin order, temperature < 0,
 * probe_token >= n_vocab, n_vocab > 52224, a token outside the vocabulary), a sequence longer than t_cap, sample_begin outside 1 .. its length,
 * steps != 1 in form 0 or > max_new in form 1, and arrays (logits_elems, mask_elems, out_elems, table_elems, state_elems: their lengths in
 * elements) shorter than the shape needs.  Since minor 17. */
int pce_selftest_decode_rules(pce_ctx *ctx, int32_t form, int32_t n, int32_t n_vocab, int32_t steps, const float *logits, int64_t logits_elems,
                              const int32_t *tokens, const int32_t *token_offsets, int32_t pad_token, int32_t t_cap, const int32_t *sample_begin,
                              int32_t sample_begin_all, const pce_whisper_decode_rules *rules, const uint8_t *vocab_mask, int64_t mask_elems,
                              float temperature, uint32_t seed_lo, uint32_t seed_hi, int32_t probe_token, const int32_t *sample_keys, int32_t max_new,
                              int32_t *out_tok, float *out_lp, float *probe_prob, int64_t out_elems, int32_t *table, int64_t table_elems,
                              int32_t *loop_state, int64_t state_elems);

/* Operand type of every Whisper / BERT matrix product (round 3).  Default since round 4: PCE_OPERANDS_F16_RESID16 (below; PCE_WHISPER_OPERANDS=fp16
 * or bf16 in the environment at pce_create selects another default).  PCE_OPERANDS_FP16: fp16 operands, the reference's own
 * arithmetic (openai-whisper runs in half precision: transcribe's fp16=True default behind
 * Code/Aligners/use_whisper_timestamped.py:163).  PCE_OPERANDS_BF16 (PCE_WHISPER_OPERANDS=bf16 in the environment at pce_create, or
 * this call): bf16 operands, 8 instead of 11 significand bits, about 3 % faster end to end (the MFMA rate is the same; the clock is not).
 * fp32 accumulation, fp32 LayerNorm / softmax statistics and an fp32 residual stream in both.  The two builds keep separate state:
 * call this BEFORE pce_whisper_load / pce_whisper_decoder_load / pce_bert_load / pce_logmel_run, and load again after switching.
 * PCE_OPERANDS_F16_RESID16 (round 4): the fp16 build with the encoder's residual stream kept in fp16 as well -- openai-whisper's own
 * `x = x + attn(...)`, `x = x + mlp(...)` are fp16 + fp16 -> fp16, only LayerNorm computes in fp32 (model.py) -- which cuts the bytes of the
 * residual / LayerNorm passes from 22 to 16 per element and layer on the batched encoder path; same state slot as PCE_OPERANDS_FP16 (no
 * reload needed between the two), pce_whisper_get_operands returns the value that was set.  The 16-bit stream belongs to the 256 x 256 GEMM path,
 * which since round 5 runs for EVERY batch size when n_state is a multiple of 256 (base, small, medium, large); a model whose width is not (tiny:
 * 384; the miniatures of the tests) takes the tiled kernels with the fp32 stream in every mode, for every batch size alike. */
enum { PCE_OPERANDS_BF16 = 0, PCE_OPERANDS_FP16 = 1, PCE_OPERANDS_F16_RESID16 = 2 };
int pce_whisper_set_operands(pce_ctx *ctx, int32_t operand_type);
int pce_whisper_get_operands(pce_ctx *ctx);

/* The whole free-running loop on the device (round 3): what whisper.decoding.DecodingTask._main_loop does for a batch
 * (Code/Aligners/use_whisper_timestamped.py:150-163 -> whisper_timestamped.transcribe -> whisper.decode).  The prompts are uploaded
 * once; every later step takes the token it embeds, its position and the "ended" flags from device memory written by the previous
 * step; the host synchronises every `check_every` steps (<= 0: 4) to read ONE counter and once at the end for the results.
 * A sequence that has produced end-of-text keeps receiving it (log-probability 0), as GreedyDecoder.update pads finished
 * sequences; the loop stops when every sequence has ended or after max_new steps.  out_tokens / out_logprobs: [clips][max_new]
 * (entries of steps that did not run: eot / 0); *out_steps = steps run.  opts / probe_prob as pce_whisper_decode_step_ex (the probe
 * belongs to step 0).  Token for token the sequence of pce_whisper_decode_step_ex calls it replaces. */
int pce_whisper_decode_loop(pce_ctx *ctx, const int32_t *tokens, const int32_t *token_offsets /* [clips + 1] */,
                            const pce_whisper_decode_rules *rules, const uint8_t *vocab_mask, const pce_whisper_decode_opts *opts,
                            int32_t max_new, int32_t check_every, int32_t *out_tokens, float *out_logprobs /* or NULL */,
                            int32_t *out_steps, float *probe_prob /* [clips] or NULL */);

/* openai-whisper decoding.py detect_language for every clip of the encoded batch (what whisper.transcribe runs on the first 30 s window when no
 * language is given): the text decoder over the single token `sot` (<|startoftranscript|>), the logits of that position on the language tokens
 * alone -- every other token counts as -inf -- their softmax and the arg-max (first maximum).  Language tokens are the contiguous ids
 * lang_begin .. lang_begin + n_lang - 1 (lang_begin = sot + 1; n_lang = 99 for n_vocab 51 865, 100 for 51 866; 1..128 here).
 * ids[clips]: the winning token ids; probs[clips][n_lang]: the probabilities in id order (either may be NULL).  A clip's results do not depend on
 * what it is batched with.
 * Cost: one prefix pass of the decoder over one position per clip (and, at the first decoding call after pce_whisper_encode_run, the cross-attention
 * K / V of all layers, which are kept for the calls that follow), then n_lang rows of the tied output projection instead of n_vocab: no logits over
 * the vocabulary are formed.
 * Cache: the pass leaves position 0 of every clip's self-attention K / V cache filled for `sot`, and the record of what the cache holds is dropped:
 * the next pce_whisper_decode_step* / pce_whisper_decode_loop runs its prompts through the prefix pass, exactly as after a fresh
 * pce_whisper_encode_run, and returns the same bits as if this call had not been made.
 * PCE_E_STATE before pce_whisper_decoder_load or pce_whisper_encode_run; PCE_E_INVALID for n_lang < 1, n_lang > 128, or a token range that leaves
 * [0, n_vocab) (a vocabulary without language tokens has nothing to pass here: that is the caller's error to raise). */
int pce_whisper_detect_language(pce_ctx *ctx, int32_t sot, int32_t lang_begin, int32_t n_lang, int32_t *ids /* [clips] or NULL */,
                                float *probs /* [clips][n_lang] or NULL */);

/* ---- R8: dynamic time warping (alignment indices) ------------------------
 * The DTW of openai-whisper's timing.py (dtw_cpu) that whisper_timestamped's word alignment rests on
 * (Code/Aligners/use_whisper_timestamped.py:163): x is `batch` row-major [n_rows][n_cols] fp64 cost matrices
 * (tokens x frames, n_rows <= 1024); path_i / path_j receive up to n_rows + n_cols index pairs per matrix
 * (stride n_rows + n_cols), path_len their count.  The accumulated cost is float32, as dtw_cpu keeps it (every cell the
 * float64 sum of the input and the chosen predecessor, rounded to float32): indices bit-identical to that recurrence. */
int pce_dtw(pce_ctx *ctx, const double *x, int32_t n_rows, int32_t n_cols, int32_t batch, int32_t *path_i, int32_t *path_j,
            int32_t *path_len);

/* ---- DTW of pairs of series (scoring a synthesis against the recording) -------
 * The dynamic programme inside fastdtw(x, y, radius = 25), which Code/Pipeline/evaluate_voice.ipynb (cell 518367fb, compute_f0_rmse) runs on
 * the voiced log-F0 frames of an episode and of its synthesis: two 1-D series of 10^4 .. 10^5 points.  The fastdtw package is third party
 * and absent: restated from its published source, parity unpinned.  Pair q aligns a[a_off[q] .. a_off[q+1]) (rows, n of them) with
 * b[b_off[q] .. b_off[q+1]) (columns, m).  dt = |a[i] - b[j]|;  D[i+1][j+1] = min(D[i][j+1] + dt, D[i+1][j] + dt, D[i][j] + dt), the three
 * SUMS compared in this order (up, left, diagonal), the first minimum wins;  D[0][0] = 0, the rest of row 0 and column 0 is +inf.
 * win_lo / win_hi (both NULL: none) give every row of every pair, indexed like a, its columns [win_lo, win_hi), 0 <= lo <= hi <= m; cells
 * outside are +inf.  fp64 adds and compares only: path and distance are bit-identical to a CPU restatement of these lines (this is NOT
 * the recurrence of pce_dtw below: diagonal first on a dense matrix, float32 accumulator).
 * path_i / path_j: the path of pair q from (0, 0) to (n - 1, m - 1) starts at element a_off[q] + b_off[q] (room n + m), path_len[q] entries;
 * dist[q] = D[n][m].  status[q]: PCE_DTW_OK; PCE_DTW_EMPTY when n or m is 0 (path_len 0, dist NaN); PCE_DTW_NO_PATH when the window
 * leaves D[n][m] = +inf (path_len 0, dist +inf).  NaN / infinite inputs and malformed windows are PCE_E_INVALID.
 * No length limit: a pair is swept in tiles of PCE_DTW_SERIES_ROWS x PCE_DTW_SERIES_COLS cells, one launch per anti-diagonal of tiles over
 * all pairs, and a pair's tiling (hence its result) depends on its own n, m and window only.  The trace takes 2 bits per cell of a swept
 * tile (x 1.5 for the skewed layout); pairs are processed in groups whose traces fit PCE_DTW_TRACE_MB MiB together (environment, read at
 * pce_create; default 4096), and a single pair over that budget is PCE_E_LIMIT.  Since minor 6. */
#define PCE_DTW_SERIES_ROWS 1024
#define PCE_DTW_SERIES_COLS 2048
enum pce_dtw_status { PCE_DTW_OK = 0, PCE_DTW_EMPTY = 1, PCE_DTW_NO_PATH = 2 };
int pce_dtw_series(pce_ctx *ctx, const double *a, const int64_t *a_off, const double *b, const int64_t *b_off, const int32_t *win_lo,
                   const int32_t *win_hi, int32_t batch, int32_t *path_i, int32_t *path_j, int32_t *path_len, double *dist, int32_t *status);

/* ---- CTC forced alignment (the numeric core of Code/Aligners/CTCFA.py; whisperX.py runs its own programme: pce_wx_align below) ----
 * A CTC acoustic model gives frame-wise log-probabilities; the Viterbi pass over the 2 L + 1 blank-interleaved states of the transcript gives
 * the frame-to-label path.  The recurrence is the CPU implementation of torchaudio.functional.forced_align (third party and absent: restated
 * from its published source, parity unpinned).  State i carries `blank` (i even) or targets[i / 2] (i odd);  t = 0: alpha[0] = lp[0][blank],
 * alpha[1] = lp[0][targets[0]], the rest -inf;  t >= 1: x0 = alpha[i], x1 = alpha[i - 1] (-inf for i = 0), x2 = alpha[i - 2] where i is odd,
 * i != 1 and targets[i / 2] != targets[i / 2 - 1] (-inf otherwise);  x2 if x2 > x1 && x2 > x0 (back-pointer 2), else x1 if x1 > x0 && x1 > x2
 * (back-pointer 1), else x0 (so x1 == x2 > x0 takes x0);  alpha'[i] = fp32(chosen + lp[t][label(i)]).  The final state is 2 L if
 * alpha[2 L] > alpha[2 L - 1], else 2 L - 1; the trace walks the back-pointers to t = 0.  fp32 adds and compares only: every output is
 * bit-identical to a CPU restatement of these lines.
 * emissions: fp32 rows of n_vocab log-probabilities; clip q owns rows row_start[q] .. row_start[q] + n_frames[q] (ragged, or a padded
 * [B][T_max][V] tensor); emissions_on_device != 0: device memory of this context's device, read in place, never copied through the host.
 * Every other pointer is host memory.  targets[target_off[q] .. target_off[q + 1]) are clip q's vocabulary indices, 0 <= id < n_vocab and
 * id != blank (else PCE_E_INVALID, before anything is launched).
 * path / frame_score (either may be NULL): clip q's frames start at element sum of n_frames[0 .. q); path[t] = the label of frame t's state,
 * frame_score[t] = lp[t][path[t]] (a copy).  tok_first / tok_last, indexed like targets: first and last frame, inclusive, in the target's own
 * state.  score[q] = the final alpha.  status[q]: PCE_CTC_EMPTY (L = 0 or T = 0), PCE_CTC_TOO_SHORT (T < L + R, R = adjacent equal targets),
 * PCE_CTC_NO_PATH (the final alpha is -inf or NaN); such a clip has no path: path -1, frame_score NaN, token frames -1, score NaN (NO_PATH:
 * the final alpha).
 * form 0: a clip of up to PCE_CTC_REG_STATES states (2 L + 1) is swept with its states in registers (one wave for up to 256 states, several
 * such clips per workgroup; else one workgroup, the waves meeting at one barrier per frame), a longer one by the general form (alpha rows in
 * device memory, any L);  form 1: the register form, a clip over its limit is PCE_E_LIMIT;  form 2: the general form for every clip.  A clip's
 * outputs depend on its own emissions and targets only: not on the form, the batch, or its place in it.
 * The trace takes T x (2 L + 1) / 4 bytes (the states rounded up to the sweeping threads); clips are processed in groups whose traces fit
 * PCE_CTC_TRACE_MB MiB together (environment, read at pce_create; default 4096), and a single clip over that budget is PCE_E_LIMIT.  Since minor 15. */
#define PCE_CTC_REG_STATES 4096
typedef struct { int32_t blank; int32_t form; int32_t reserved[2]; } pce_ctc_params;   /* form: 0 auto, 1 register form, 2 general form */
enum pce_ctc_status { PCE_CTC_OK = 0, PCE_CTC_EMPTY = 1, PCE_CTC_TOO_SHORT = 2, PCE_CTC_NO_PATH = 3 };
int pce_ctc_align(pce_ctx *ctx, const float *emissions, int32_t emissions_on_device, const int64_t *row_start /* [n] */,
                  const int32_t *n_frames /* [n] */, int32_t n_vocab, const int32_t *targets, const int64_t *target_off /* [n+1] */,
                  int32_t n_clips, const pce_ctc_params *p,
                  int32_t *path /* [sum n_frames] or NULL */, float *frame_score /* [sum n_frames] or NULL */,
                  int32_t *tok_first, int32_t *tok_last /* [target_off[n]] */, float *score /* [n] */, int32_t *status /* [n] */);

/* ---- whisperX forced alignment (the numeric core of Code/Aligners/whisperX.py: whisperx.align's trellis, wildcard and beam back-track) ----
 * whisperX does not run the CTC recurrence above: it runs a trellis over the J characters of a transcript segment with no interleaved blanks,
 * gives characters the model's dictionary lacks a wildcard emission, and walks back with a beam search that reads the trellis values
 * themselves.  whisperx is third party and absent: restated from the published source of whisperx 3.3.x (alignment.py).  The trellis lines
 * are pinned bit for bit to torch's CPU operators (zeros / cumsum / maximum / where); the back-track's parity with the package is unpinned.
 * Per clip (one transcript segment): e[T][V] fp32 log-probabilities, tok[J] with -1 = wildcard, else 0 <= tok[j] < V; blank; beam width W.
 * Wildcard emission: wild(t, k) = e[t][k] for k >= 0; for k = -1 the max over v != blank of e[t][v] (-inf when V = 1).
 * Trellis, fp32 tr[T][J]:  tr[0][0] = 0;  for t >= 1, tr[t][0] = fp32(sum_{u = 1..t} (double) e[u][blank]), accumulated in fp64 in frame order,
 * each prefix rounded to fp32 (what torch.cumsum does for float32 on the CPU; a sequential fp32 sum differs);  tr[0][j] = -inf for j >= 1;
 * the wedge: tr[t][0] = +inf for t >= max(0, T - J + 1) when J >= 2, and for every t when J = 1 (Python's trellis[-J + 1:, 0] = inf, where
 * -0: is the whole column);  for t = 0 .. T - 2 and j >= 1:
 *     tr[t + 1][j] = max(fp32(tr[t][j] + e[t][blank]), fp32(tr[t][j - 1] + wild(t, tok[j])))
 * fp32 adds and a max only (no multiply: no FMA can form).  The wedge carries +inf along the diagonal and never reaches tr[T - 1][J - 1].
 * Beam back-track: a beam is (j, t, score) plus its path; all beams move in lock step, each step takes t to t - 1.  It starts with one beam
 * (J - 1, T - 1, tr[T - 1][J - 1]) whose path holds the point (token index J - 1, frame T - 1, lp = e[T - 1][blank]).  While beams exist and
 * the first beam has j > 0, for every beam in order: a beam with t <= 0 is dropped;  STAY: if tr[t - 1][j] is not +-inf, the candidate
 * (j, t - 1, tr[t - 1][j]) with the point (j, t - 1, lp = e[t - 1][blank]);  CHANGE: if j > 0 and tr[t - 1][j - 1] is not +-inf, the candidate
 * (j - 1, t - 1, tr[t - 1][j - 1]) with the point (j - 1, t - 1, lp = wild(t - 1, tok[j])): the emission belongs to the token being left (the
 * source's choice).  The candidates are ordered by score, descending, by a STABLE sort (equal scores keep their emission order, as Python's
 * sorted(..., reverse=True) does; stay from (t, j) and change from (t, j + 1) land on one cell with one score, so ties are structural), and
 * the first W are kept.  No beams left: PCE_WX_NO_PATH.  Otherwise the first beam wins; its remaining frames t - 1 .. 0 get the points
 * (j, ., lp = e[.][blank]).  Per frame: path_tok[t] (a token INDEX, 0 .. J - 1) and path_lp[t] (an fp32 copy of the emission named above; no
 * exp on the device).  It follows that J = 1 gives token 0 on every frame (score +inf: the wedge), that T = 1 with J >= 2 and J > T are
 * PCE_WX_NO_PATH, and that J = T changes at every step.  NaN emissions: the result is unspecified, but the call returns and every written
 * index is in range.
 * emissions, row_start, n_frames, n_vocab, emissions_on_device: exactly as pce_ctc_align takes them (ragged rows or a padded tensor; device
 * memory is read in place).  Every other pointer is host memory.  tokens[token_off[q] .. token_off[q + 1]) are clip q's tokens; a token may
 * equal blank.  PCE_E_INVALID, before anything is launched: a token outside {-1} u [0, n_vocab), beam_width outside 1 .. PCE_WX_MAX_BEAM, NULL
 * or decreasing offsets.  A clip of more than PCE_WX_MAX_TOKENS tokens is PCE_E_LIMIT: the sweep keeps a clip's row in the registers of one
 * workgroup and has no general form (whisperX aligns segments of at most 30 s, so J <= T <= 1 500 at wav2vec2's stride of 20 ms).
 * path_tok / path_lp (either may be NULL): clip q's frames start at element sum of n_frames[0 .. q).  trellis (or NULL): the stage hook, the
 * tables between the two kernels, clip-major, clip q's T_q x J_q row-major floats behind those of the clips before it.  score[q] =
 * tr[T - 1][J - 1].  status[q]: PCE_WX_EMPTY (J = 0 or T = 0; nothing is launched for the clip, score NaN), PCE_WX_NO_PATH (score keeps the
 * final cell); such a clip has path_tok -1 and path_lp NaN.  Clips are processed in groups whose tables (T x J fp32, J rounded up to 4) fit
 * PCE_CTC_TRACE_MB MiB together (environment, read at pce_create; default 4096); a single clip over that budget is PCE_E_LIMIT.  A clip's
 * outputs depend on its own emissions and tokens only: not on the batch, or on its place in it.  Since minor 20. */
#define PCE_WX_MAX_TOKENS 4096
#define PCE_WX_MAX_BEAM 8
typedef struct { int32_t blank; int32_t beam_width; int32_t reserved[2]; } pce_wx_params;
enum pce_wx_status { PCE_WX_OK = 0, PCE_WX_EMPTY = 1, PCE_WX_NO_PATH = 2 };
int pce_wx_align(pce_ctx *ctx, const float *emissions, int32_t emissions_on_device, const int64_t *row_start /* [n] */,
                 const int32_t *n_frames /* [n] */, int32_t n_vocab, const int32_t *tokens, const int64_t *token_off /* [n+1] */,
                 int32_t n_clips, const pce_wx_params *p,
                 int32_t *path_tok /* [sum n_frames] or NULL */, float *path_lp /* [sum n_frames] or NULL */,
                 float *trellis /* [sum T_q * J_q] or NULL */, float *score /* [n] */, int32_t *status /* [n] */);

/* ---- batched Needleman-Wunsch word alignment ------------------------------
 * Replaces needleman_wunsch (Code/Pipeline/NeedlemanWunschAlignement.py:27-81) for a batch of sequence pairs.
 * Pair b aligns a_ids[a_off[b] .. a_off[b+1]) (rows; any number since round 5) with b_ids[b_off[b] .. b_off[b+1]); the ids are
 * the host's integer codes of the normalised tokens (:43-47), equal ids = equal tokens.  Scores as the reference's
 * keyword arguments (match 1, mismatch -1, gap -1).  Output for pair b starts at element
 * sum_{p<b} (len_a[p] + len_b[p]) of out_i / out_j and has out_len[b] steps in alignment order: (i, j) = a
 * diagonal step, (i, -1) a gap in the second sequence, (-1, j) a gap in the first; ties resolve diagonal > up >
 * left as the reference's trace-back does (:69-80).  Integer arithmetic: identical alignments. */
int pce_nw_align(pce_ctx *ctx, const int32_t *a_ids, const int64_t *a_off, const int32_t *b_ids, const int64_t *b_off, int32_t batch,
                 int32_t match, int32_t mismatch, int32_t gap, int32_t *out_i, int32_t *out_j, int32_t *out_len);

/* ---- batched Levenshtein distance --------------------------
 * Replaces levenshtein_distance (Code/Aligners/levenshtein_dist_align_txtgrids.py:43-70) for a batch of string pairs.  Pair b
 * compares a_chars[a_off[b] .. a_off[b+1]) with b_chars[b_off[b] .. b_off[b+1]); the characters are Unicode code points (what a
 * Python str iterates over).  Unit insertion / deletion / substitution costs; out_dist[b] = the distance (len of the other string
 * when one is empty, :57-58).  Integer arithmetic: identical distances; no length limit.  The caller of the reference's function,
 * main()'s merge loop (:98-158), clamps its cursors (`min(i + 1, n1 - 1)`, :113) under `while i < n1 and j < n2` and therefore
 * never terminates: it has no output to reproduce and is not part of this interface. */
int pce_levenshtein(pce_ctx *ctx, const uint32_t *a_chars, const int64_t *a_off, const uint32_t *b_chars, const int64_t *b_off,
                    int32_t batch, int32_t *out_dist);

/* ---- batched difflib.SequenceMatcher and the fuzzy alignment of "Compare Breaks" -------------
 * sim() of Code/audioPipeline.py:970-971 is difflib.SequenceMatcher(None, a, b).ratio() = 2.0 * matches / (len(a) + len(b)) (1.0 for two
 * empty strings); pce_seqmatch returns `matches`, the summed sizes of get_matching_blocks, for pairs of strings of Unicode code points (any
 * uint32 values; equal values = equal elements).  The rules, with isjunk = None:
 *   popular    with autojunk != 0 and len(b) >= 200, an element that occurs more than len(b) / 100 + 1 times in b is popular: it never
 *              starts or continues a run of find_longest_match, but it is not junk: the extension runs over it;
 *   longest    find_longest_match(alo, ahi, blo, bhi): over i in [alo, ahi) ascending and the non-popular j in [blo, bhi) with
 *              b[j] == a[i] ascending, k = len[i-1][j-1] + 1, a run never continuing across blo; the best run is replaced on k > best
 *              only, so the winner has the largest k, then the smallest start in a, then the smallest start in b (k = 0: (alo, blo));
 *   extension  left while i > alo, j > blo and a[i-1] == b[j-1], then right in the same way within ahi / bhi (moves only where popular
 *              elements exist);
 *   blocks     a LIFO stack that starts with (0, la, 0, lb): pop a range, find its longest match; k > 0 adds k to `matches` and pushes
 *              (alo, i, blo, j) when alo < i and blo < j, then (i + k, ahi, j + k, bhi) when i + k < ahi and j + k < bhi.
 * Integer arithmetic: `matches` is exactly difflib's.  String s of a table is chars[off[s] .. off[s+1]), off[0] = 0.  Pair p compares string
 * pair_a[p] of the a table with string pair_b[p] of the b table; pair_a == pair_b == NULL: all n_a * n_b pairs, row-major (pair i * n_b + j =
 * a string i with b string j; n_pairs must equal n_a * n_b).  The result is not symmetric in a and b (difflib's is not).
 * Limits (PCE_E_LIMIT): a string has fewer than 2^30 elements, a call at most PCE_SEQMATCH_MAX_PAIRS pairs, and the scratch of one
 * workgroup of 4 waves -- per wave 4 bytes per element of the longest b string when that is longer than PCE_SEQMATCH_ROW_LDS, and 16 bytes
 * per stack entry, min(longest a, longest b) + 1 of them -- at most PCE_SEQMATCH_SCRATCH_MAX bytes, which strings of up to 2^23 elements
 * always meet.  PCE_E_INVALID: NULL or decreasing offsets, a pair index outside its table.  A range of b of up to PCE_SEQMATCH_ROW_LDS columns is swept with its row of run
 * lengths in LDS, a wider one through a global row; the stack holds PCE_SEQMATCH_STACK_LDS ranges in LDS and spills the rest: neither is a
 * limit, and a pair's result depends on its two strings only.
 *
 * pce_seqmatch_align: all pairs, then the alignment of Code/audioPipeline.py:973-998 on the device: sim[i][j] = 2.0 * matches / (la_i + lb_j)
 * in fp64 (1.0 for two empty strings); dp[0][.] = dp[.][0] = 0; match = dp[i-1][j-1] + sim[i-1][j-1]; dp[i][j] = dp[i-1][j] (up) if
 * dp[i-1][j] >= dp[i][j-1] and dp[i-1][j] >= match, else dp[i][j-1] (left) if dp[i][j-1] >= match, else match (diagonal).  The walk back from
 * (n_a, n_b) ends when i == 0 or j == 0; its diagonal steps (i-1, j-1), ascending, are match_a / match_b (room min(n_a, n_b)), *n_matches
 * their count.  sim: [n_a * n_b] row-major or NULL.  fp64 multiply, divide, add and compare only: bit-identical to the Python lines.
 * n_a == 0 or n_b == 0: PCE_OK with *n_matches = 0.  n_a * n_b > PCE_SEQMATCH_MAX_PAIRS: PCE_E_LIMIT.  Any number of rows.  Since minor 10. */
#define PCE_SEQMATCH_MAX_PAIRS ((int64_t)1 << 26)
#define PCE_SEQMATCH_ROW_LDS 2048
#define PCE_SEQMATCH_SCRATCH_MAX ((int64_t)1 << 30)
#define PCE_SEQMATCH_STACK_LDS 8
/* pairs (pair_a[p], pair_b[p]) of the two string tables; pair_a == pair_b == NULL: all n_a * n_b pairs, row-major (n_pairs must equal n_a * n_b) */
int pce_seqmatch(pce_ctx *ctx, const uint32_t *a_chars, const int64_t *a_off, int32_t n_a,
                 const uint32_t *b_chars, const int64_t *b_off, int32_t n_b,
                 const int32_t *pair_a, const int32_t *pair_b, int64_t n_pairs, int32_t autojunk, int32_t *out_matches);
/* all pairs + the DP of Code/audioPipeline.py:973-998; sim: [n_a * n_b] or NULL; match_a / match_b: [min(n_a, n_b)] */
int pce_seqmatch_align(pce_ctx *ctx, const uint32_t *a_chars, const int64_t *a_off, int32_t n_a,
                       const uint32_t *b_chars, const int64_t *b_off, int32_t n_b, int32_t autojunk,
                       double *sim, int32_t *match_a, int32_t *match_b, int32_t *n_matches);

/* ---- the text matching of the aligner evaluation (Code/whisper_testing/splitting.py:94-128) -------------
 * align_intervals pairs the word intervals of a hand-made gold tier with those of an aligner's tier by their normalised texts (normalize_text,
 * :90-92: host work).  Gold intervals are taken in list order; each takes, among the predicted intervals no earlier gold interval of the same
 * call has claimed, the one of the highest score above 0.4.  The score of a pair, in this order of tests:
 *   equal      1.0 (class 3) when the two texts are equal, code point by code point (two empty texts are equal);
 *   substring  0.8 (class 2) when either text occurs inside the other; the EMPTY string occurs inside every string, so a gold interval of
 *              punctuation alone, whose text normalises to nothing, claims the first unclaimed prediction;
 *   word       0.5 (class 1) when a whitespace-separated word of the gold text equals a word of the predicted text.  Words are integer ids
 *              which the caller interns per call: equal id = equal word;
 *   else 0 (class 0): never a match.
 * The best is replaced on a strict > only: among predicted intervals of one score the FIRST in list order wins.  A claim holds for the later
 * gold intervals of the same problem and for nothing else.
 * The score depends on the two texts alone, so one class table per TABLE PAIR (gold tier, predicted tier) serves every problem on that pair.
 * Table pair t owns gold intervals [pair_gold[t], pair_gold[t+1]) and predicted intervals [pair_pred[t], pair_pred[t+1]) of the concatenated
 * tiers (both range arrays [n_pairs + 1], from 0, not decreasing, ending at n_gold / n_pred).  Interval s of a tier has code points
 * chars[off[s] .. off[s+1]) and word ids words[woff[s] .. woff[s+1]), off[0] = woff[0] = 0.
 * Problem q walks the gold intervals gold_idx[prob_off[q] .. prob_off[q+1]) of pair prob_pair[q], indices local to the pair, in that order,
 * over the predicted intervals that are members: bit (j & 63) of word member[member_off[q] + (j >> 6)] for local index j, ceil(P / 64) words;
 * member_off == NULL or member_off[q] < 0: all of them.  A subset of a tier keeps the tier's order (the reference filters its lists), so the
 * first member in list order is the lowest member index.  out_match[prob_off[q] + i] = the local index of the predicted interval that gold
 * entry i claimed, or -1; out_class[..] = its class 3 / 2 / 1, or 0.  Integer work only: exactly the reference's pairs.  A problem's outputs
 * depend on its own lists and its table pair only: not on the batch, on its place in it, or on what ran before.
 * Table pairs run in groups of consecutive pairs whose class tables -- 24 bytes x gold intervals x ceil(P / 64) per pair that a problem walks --
 * fit PCE_IVL_TABLE_MB MiB together (environment, read at pce_create; default 2048, which holds a pair of 65 536 x 65 536 intervals: 1.5 GiB,
 * built by a fixed grid of waves that strides over the pair's tasks, so no launch grows with the tables); a single
 * pair over that budget is PCE_E_LIMIT, and so are a pair of more than PCE_IVL_MAX_PRED predicted intervals and a text of 2^30 code points.
 * PCE_E_INVALID: NULL or decreasing offsets or ranges, a pair or gold index outside its table.  n_problems == 0: PCE_OK, nothing written.
 * Since minor 24. */
#define PCE_IVL_MAX_PRED (1 << 18)
int pce_ivl_match(pce_ctx *ctx, const uint32_t *g_chars, const int64_t *g_off, const int32_t *g_words, const int64_t *g_woff, int32_t n_gold,
                  const uint32_t *p_chars, const int64_t *p_off, const int32_t *p_words, const int64_t *p_woff, int32_t n_pred,
                  const int32_t *pair_gold, const int32_t *pair_pred, int32_t n_pairs,
                  const int32_t *prob_pair, const int64_t *prob_off, const int32_t *gold_idx, const int64_t *member_off, const uint64_t *member,
                  int32_t n_problems, int32_t *out_match, int8_t *out_class);

/* ---- break-prediction token classifier --------------------
 * Forward pass of transformers.BertForTokenClassification, the model Code/baseline_models/pause_bert.py:127-132 trains
 * (bert-base-multilingual-uncased, num_labels = 2, MAX_LENGTH = 128; the reference has training code only: this is the
 * inference path a pipeline step would call).  weights: the float32 state_dict flattened in the order of
 * prosody-control-french-tts_amd/bert_weights.py:tensor_order.  Sequences are token ids (tokenisation is host logic and
 * needs the checkpoint's vocabulary); token_type_ids = 0, right padding is implicit in the offsets.  MFMA operands of
 * the context's operand mode (pce_whisper_set_operands: fp16 by default, bf16 on request), fp32 accumulation, LayerNorm /
 * residual stream / logits in fp32. */
/* n_state % 128 == 0 and <= 2048 (the LayerNorm kernels), n_head = n_state / 64, n_pos <= 512, n_labels <= 128: else PCE_E_LIMIT at load */
typedef struct pce_bert_dims { int32_t n_vocab, n_pos, n_type, n_state, n_head, n_layer, n_labels; } pce_bert_dims;
int pce_bert_load(pce_ctx *ctx, const pce_bert_dims *dims, const float *weights, int64_t n_floats);
int pce_bert_run(pce_ctx *ctx, const int32_t *input_ids, const int32_t *offsets /* [n_seq + 1] */, int32_t n_seq);
/* logits: [len][n_labels] or NULL; labels: [len] argmax (first maximum) or NULL */
int pce_bert_fetch(pce_ctx *ctx, int32_t seq, float *logits, int32_t *labels);

/* ---- wav2vec2 / MMS CTC acoustic model: the emissions of the forced alignment (the front half of Code/Aligners/CTCFA.py) ----
 * Forward pass of transformers.Wav2Vec2ForCTC in eval mode (no dropout, layerdrop or SpecAugment, no attention mask: all windows have one
 * length) over the resident batch, which must be at 16 kHz.  Both published forms: feat_norm 0 ("group": GroupNorm(C, C) behind the first
 * convolution, no other normalisation in the feature encoder) with post-LN encoder layers (stable_ln 0: encoder.layer_norm in front of them),
 * and feat_norm 1 ("layer": bias, LayerNorm and GELU behind every convolution) with pre-LN layers (stable_ln 1: encoder.layer_norm behind them).
 * weights: the float32 state_dict flattened in the order of prosody-control-french-tts_amd/w2v_weights.py:tensor_order (convolution weights
 * as [out][tap][in], the positional convolution's weight norm folded, its weights as [out][tap][in / groups]).
 * Windowing is that of ctc-forced-aligner's generate_emissions (Aligners/ctc_emissions.hf_emissions): samples are int16 / 32768; a clip gets
 * context_samples zeros in front and zeros behind to a whole number of windows, plus the context; windows of window_samples + 2 context_samples
 * sit at stride window_samples; the model runs per window; frames [cut, T - cut + 1) of a window are kept, cut = int(context seconds * 50) --
 * PCE_E_INVALID unless that is int(window seconds * 50) frames; the windows are joined and the first n_frames (pce_w2v_window_plan) kept;
 * log-softmax in fp32 over the n_vocab columns; with `star` one column of zeros follows (n_cols = n_vocab + 1).  The windows are never
 * materialised: the waveform layer reads the resident PCM and supplies the zeros itself.
 * Arithmetic: the waveform convolution, its normalisation (group statistics in fp64 over a fixed partition of the time axis, added in a fixed
 * order: no atomics) and every LayerNorm / softmax in fp32; every other product on MFMA operands of the context's operand mode
 * (pce_whisper_set_operands) with fp32 accumulation; the residual stream of the encoder in fp32.  Windows run in chunks of windows_per_chunk
 * (0: as many as keep one chunk's activation images within PCE_W2V_IMAGE_BUDGET bytes); every kernel is chosen by the model's widths alone and
 * none reduces across windows: a window's emissions are bit-identical whatever the chunk size and whatever it is batched with.
 * Limits (PCE_E_LIMIT at load): n_conv == 7; 10 taps at stride <= 8 on the waveform; conv_dim % 64 == 0 and <= 1024, % 128 == 0 behind the
 * waveform layer, conv_kernel[i] * conv_dim[i - 1] % 64 == 0; n_state % 128 == 0 and <= 2048, n_head * 64 == n_state, n_inter % 128 == 0;
 * pos_taps == 128 and n_state / pos_groups one of 16, 32, 48, 64.  PCE_E_STATE: run before load, shape / fetch / device before run.
 * PCE_E_INVALID: a batch that is not at 16 kHz, a blob of the wrong size.  Since minor 16. */
#define PCE_W2V_IMAGE_BUDGET ((int64_t)3 << 30)
typedef struct pce_w2v_dims {
    int32_t n_conv;                                        /* 7 */
    int32_t conv_dim[8], conv_kernel[8], conv_stride[8];
    int32_t feat_norm;                                     /* 0 "group", 1 "layer" */
    int32_t conv_bias, n_state, n_head, n_inter, n_layer, stable_ln, pos_taps, pos_groups, n_vocab;
    float ln_eps;
} pce_w2v_dims;
typedef struct pce_w2v_plan { int32_t window_samples, context_samples, windows_per_chunk /* 0 = by budget */, star /* append the zero column */; } pce_w2v_plan;
int pce_w2v_load(pce_ctx *ctx, const pce_w2v_dims *dims, const float *weights, int64_t n_floats);
/* the loader's conditions without a context (host arithmetic only): the status pce_w2v_load would return for these dims and this blob size, its
 * message in msg (cap bytes; may be NULL) */
int pce_w2v_check(const pce_w2v_dims *dims, int64_t n_floats, char *msg, size_t cap);
int pce_w2v_run(pce_ctx *ctx, const pce_w2v_plan *plan);
int pce_w2v_shape(pce_ctx *ctx, int32_t clip, int64_t *n_frames, int32_t *n_cols);
/* log_probs: [n_frames][n_cols] */
int pce_w2v_fetch(pce_ctx *ctx, int32_t clip, float *log_probs);
/* the packed emissions of the last run, device memory [sum n_frames][n_cols], and the host tables pce_ctc_align takes with it (row_start[q]: the
 * first row of clip q); all owned by the context and valid until its next pce_w2v_run / pce_w2v_load */
int pce_w2v_device(pce_ctx *ctx, const float **d_emissions, const int64_t **h_row_start, const int32_t **h_n_frames, int32_t *n_cols);
/* host arithmetic only (ctx-free): windows and kept frames of a clip of n_samples, as ctc_emissions.window_plan counts them */
int pce_w2v_window_plan(int64_t n_samples, int32_t window_samples, int32_t context_samples, int64_t *n_windows, int64_t *n_frames);
/* whisperX's emissions (whisperx 3.3.x alignment.py as Aligners/ctc_emissions.segment_emissions restates it; parity unpinned): segment j owns
 * samples [begin, end) of resident clip `clip`, int16 / 32768; one of fewer than min_samples samples (begin == end included) is followed by
 * zeros up to min_samples; the model runs on the segment ALONE (no context, no cut, no attention mask, no padding to a neighbour's length);
 * log-softmax in fp32 over the n_vocab columns, one column of zeros behind them with `star`.  pce_w2v_shape / _fetch / _device then read the
 * result indexed by SEGMENT, in the caller's order (row_start follows that order whatever order the chunks ran in).  Arithmetic and kernels
 * are pce_w2v_run's.  Segments run in chunks of similar length (csrc/pce_w2v_seg_plan.h): longest first, a chunk takes segments down to half
 * its longest one's padded frames, at most segments_per_chunk (0: as many as keep the chunk's images within PCE_W2V_IMAGE_BUDGET); its
 * launches cover all its segments, each in a slot of the longest one's rows.  No kernel reduces across segments and none is chosen by the row
 * count: a segment's emissions are bit-identical whatever it is batched with, in whatever order, and whatever ran before.
 * PCE_E_INVALID: a batch that is not at 16 kHz, a clip index out of range, 0 <= begin <= end <= clip length violated, a segment the model
 * gives no frame for (min_samples below its receptive field).  PCE_E_LIMIT: the 32-bit limits of pce_w2v_run, for the longest segment (2^26
 * samples; the attention's offsets).  PCE_E_STATE: as pce_w2v_run.  Since minor 21. */
typedef struct pce_w2v_segment { int32_t clip; int32_t reserved; int64_t begin, end; } pce_w2v_segment;   /* samples [begin, end) of a resident clip */
typedef struct pce_w2v_seg_plan { int32_t min_samples /* 400 */, segments_per_chunk /* 0 = by budget */, star; } pce_w2v_seg_plan;
int pce_w2v_run_segments(pce_ctx *ctx, const pce_w2v_segment *segments, int32_t n_segments, const pce_w2v_seg_plan *plan);
/* what the latest pce_w2v_run_segments cost: its chunks, the rows its launches covered (slots x slot rows, summed over the chunks) and the
 * frames among them that belong to a segment (PCE_E_STATE when the latest run was none) */
int pce_w2v_segments_plan(pce_ctx *ctx, int64_t *n_chunks, int64_t *rows_computed, int64_t *rows_valid);
/* host arithmetic only (ctx-free): frames the model of `dims` gives for a segment of n_samples run on max(n_samples, min_samples); 0 when that
 * is shorter than the feature encoder's receptive field */
int pce_w2v_segment_frames(const pce_w2v_dims *dims, int64_t n_samples, int32_t min_samples, int64_t *n_frames);
/* Stage self-tests: the three new stages through the run's own launches, 16-bit values as raw bits of the context's operand type.
 * _wave: the waveform layer over the windows of ONE clip: w [C][10], bias [C] or NULL, gamma / beta [C]; out [n_windows][T0][C],
 * T0 = (window + 2 context - 10) / stride + 1 (nothing is written when the window is shorter than the 10 taps).
 * _lngelu: LayerNorm over the C columns of 16-bit rows, then GELU where gelu != 0 (in place on the device, as the run launches it).
 * _posconv: out = x + GELU(conv(x) + bias) for n_win windows of T frames, x / out fp32 [n_win][T][d] (x is rounded to the operand type as it
 * is staged), w [d][128][d / groups] 16-bit. */
int pce_selftest_w2v_wave(pce_ctx *ctx, const int16_t *pcm, int64_t n_samples, int32_t window_samples, int32_t context_samples, int32_t feat_norm,
                          int32_t C, int32_t stride, const float *w, const float *bias, const float *gamma, const float *beta, uint16_t *out);
int pce_selftest_w2v_lngelu(pce_ctx *ctx, const uint16_t *x, int32_t rows, int32_t C, const float *w, const float *b, float eps, int32_t gelu, uint16_t *out);
int pce_selftest_w2v_posconv(pce_ctx *ctx, const float *x, int32_t n_win, int32_t T, int32_t d, int32_t groups, const uint16_t *w, const float *bias,
                             float *out);
/* ... and the two stages that take per-item frame counts, through pce_w2v_run_segments' launches.  _wave_segments: item i is samples
 * [seg[2 i], seg[2 i + 1]) of ONE clip, run on max(its samples, min_samples); out [n_seg][slot][C], slot = the longest item's frames, rows behind
 * an item's own frames zero.  _posconv_segments: window i holds len[i] <= T frames in a slot of T rows of x / out [n_win][T][d]; rows behind
 * its frames come back as x.  Since minor 21. */
int pce_selftest_w2v_wave_segments(pce_ctx *ctx, const int16_t *pcm, int64_t n_samples, const int64_t *seg, int32_t n_seg, int32_t min_samples,
                                   int32_t feat_norm, int32_t C, int32_t stride, const float *w, const float *bias, const float *gamma, const float *beta,
                                   uint16_t *out);
int pce_selftest_w2v_posconv_segments(pce_ctx *ctx, const float *x, int32_t n_win, const int32_t *len, int32_t T, int32_t d, int32_t groups,
                                      const uint16_t *w, const float *bias, float *out);

/* ---- asynchronous statistics fetch ---------------------------------------
 * The per-slice numbers of the last pce_energy_run / pce_lufs_run / pce_pitch_run are what the reference's
 * driver consumes per utterance (Code/audioPipeline.py:380-400) and what the sharded driver all-gathers
 * (SURVEY.md 8e).  pce_stats_enqueue queues their device-to-host copies behind those runs into pinned
 * staging memory and returns at once; pce_stats_wait blocks only on those copies and unpacks them, so the
 * next batch's kernels can already be running.  slot is 0 or 1 (two batches in flight).  Any output pointer
 * may be NULL; a non-NULL pointer whose run did not precede the enqueue is an error (PCE_E_STATE). */
int pce_stats_enqueue(pce_ctx *ctx, int32_t slot);
int pce_stats_wait(pce_ctx *ctx, int32_t slot, pce_energy *energy, double *lufs, int32_t *lufs_status, pce_pitch_summary *pitch);

/* ---- measurement -------------------------------------------------------
 * With profiling on, every kernel launch is bracketed by HIP events on the
 * context's stream; pce_profile_get returns the accumulated device time. */
enum pce_kernel_id {
    PCE_K_ENERGY = 0,
    PCE_K_LUFS_PASS1, PCE_K_LUFS_SCAN, PCE_K_LUFS_PASS2, PCE_K_LUFS_GATE,
    PCE_K_PITCH_REFINE, PCE_K_PITCH_FRAMES, PCE_K_PITCH_PATH, PCE_K_PITCH_MEDIAN, PCE_K_PITCH_DELTA,
    PCE_K_STFT_MAX, PCE_K_STFT_DB, PCE_K_LOGMEL, PCE_K_WHISPER_ENC, PCE_K_RESAMPLE, PCE_K_DTW, PCE_K_WHISPER_ALIGN, PCE_K_NW, PCE_K_STFT_NORM,
    PCE_K_FRAME_ENERGY, PCE_K_BERT, PCE_K_PYIN_FRAMES, PCE_K_PYIN_VITERBI, PCE_K_WHISPER_DECODE,
    /* the launches inside the composite entries above (whisper_encoder, whisper_align, bert_forward, whisper_decode_step),
     * each bracketed on its own so that a roofline figure divides one kernel's work by that kernel's own duration */
    PCE_K_GEMM128, PCE_K_GEMM_WIDE, PCE_K_ATTENTION, PCE_K_LAYERNORM, PCE_K_GEMM_FLAT,
    /* round 3: one id per device kernel name (what rocprofv3 --kernel-trace prints), and the persistent GEMM per encoder shape
     * ("k_gemm_flat:<shape>"; PCE_K_GEMM_FLAT keeps the launches no shape is named for) */
    PCE_K_ADD_LAYERNORM, PCE_K_STFT_RAW, PCE_K_LOGMEL_NORM, PCE_K_ATTENTION_LEAN,
    PCE_K_GEMM_FLAT_QKV, PCE_K_GEMM_FLAT_OUT, PCE_K_GEMM_FLAT_FC1, PCE_K_GEMM_FLAT_FC2, PCE_K_GEMM_FLAT_XKV,
    PCE_K_DECODE_LOOP, PCE_K_CROSS_ATTN1, PCE_K_GEMM_SKINNY, PCE_K_LEVENSHTEIN,
    /* minor 6: the tile sweeps and the walk back of pce_dtw_series; their work count (pce_profile_get_work) is in-window CELLS, not flops */
    PCE_K_DTW_SERIES, PCE_K_DTW_SERIES_TRACE,
    /* minor 7 */
    PCE_K_INTENSITY, PCE_K_INTENSITY_SUMMARY,
    /* minor 9: PCE_K_SILENCE_RANGES brackets three launches (tiles, carry, tiles with the carry) */
    PCE_K_MS_ENERGY, PCE_K_SILENCE_SCAN, PCE_K_SILENCE_RANGES,
    /* minor 13: CREPE (PCE_K_CREPE_CONV2: block 2 alone, the launch that carries most of the work; PCE_K_CREPE_CONV: blocks 3-6; PCE_K_CREPE_DECODE:
     * the log-softmax / arg-max pass and the gather) */
    PCE_K_CREPE_FRAMES, PCE_K_CREPE_CONV1, PCE_K_CREPE_CONV2, PCE_K_CREPE_CONV, PCE_K_CREPE_CLASSIFIER, PCE_K_CREPE_DECODE, PCE_K_CREPE_VITERBI,
    /* minor 24: pce_ivl_match's class tables and claims; work count = text PAIRS tested, gold STEPS */
    PCE_K_IVL_CLASSES, PCE_K_IVL_CLAIM,
    /* minor 16: pce_w2v_run as a whole; the waveform layer (statistics, finish and recompute passes together), the positional convolution, the log-softmax tail */
    PCE_K_W2V, PCE_K_W2V_WAVE, PCE_K_W2V_POSCONV, PCE_K_W2V_TAIL,
    /* minor 20: pce_wx_align's row maxima for the wildcard (launched only when a clip holds one), the sweep (both launch shapes) and the beam back-track;
     * work count = emission values read, trellis CELLS, frames */
    PCE_K_WX_ROWMAX, PCE_K_WX_TRELLIS, PCE_K_WX_BACKTRACK,
    /* minor 15: the register form (both launch shapes), the general form and the walk back of pce_ctc_align; work count = trellis CELLS (frames for the walk) */
    PCE_K_CTC, PCE_K_CTC_GENERAL, PCE_K_CTC_TRACE,
    /* minor 10: their work count is swept CELLS (k_seqmatch: every range of every pair, recursion included; k_seqmatch_align: n_a * n_b) */
    PCE_K_SEQMATCH, PCE_K_SEQMATCH_ALIGN, PCE_K_COUNT
};
int pce_profile_enable(pce_ctx *ctx, int on);
int pce_profile_reset(pce_ctx *ctx);
int pce_profile_get(pce_ctx *ctx, int kernel_id, double *total_ms, int64_t *launches);
/* algorithmic work of the bracketed launches of a kernel id since the last reset: floating-point operations
 * (2 M N K of a GEMM launch, 4 T^2 d of an attention launch; 0 for ids that do not count) */
int pce_profile_get_work(pce_ctx *ctx, int kernel_id, double *flops);
const char *pce_kernel_name(int kernel_id);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* PCE_H */
