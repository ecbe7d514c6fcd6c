/*
 * audiotoken_hip.h — C ABI of libaudiotoken_hip.so: the MI355X (gfx950) hot path of cmeraki/audiotoken.
 *
 * The reference has no FFI: its seam is the Python callable protocol
 *     self.encoder(input_batch: float32[B,N] on device, attention_mask: float32[B,N]) -> int16[B,K,T]
 * (reference audiotoken/core.py:194 and :276; encoder classes audiotoken/encoder.py:29-186) and
 *     self.decoder(tokens: int64[B,K,T]) -> float32[1, B*320*T]
 * (reference audiotoken/core.py:355-359; audiotoken/decoder.py:66-76).
 * Each entry point below names the reference interface it replaces. All pointers marked "device" are HIP
 * device pointers on the handle's device; everything is row-major and contiguous. Calls are stream-ordered and
 * never synchronise or allocate; scratch comes from a caller-provided workspace so the caller's allocator
 * (PyTorch's caching allocator in the Python binding) stays the only allocator. Functions return 0 on success,
 * a negative code on failure; at_last_error() returns the thread-local message. Nothing aborts.
 *
 * Threading: a handle is bound to one device; calls on one handle must be serialised by the caller; different
 * handles are independent (one process per GPU in the multi-GPU harness).
 */
#ifndef AUDIOTOKEN_HIP_H
#define AUDIOTOKEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* at_stream_t; /* hipStream_t */

/* ---- library ------------------------------------------------------------------------------------------ */
int at_version(void);
const char* at_last_error(void);

/* ---- acoustic tokenizer: EnCodec 24 kHz SEANet encoder + residual VQ, and the decoder ------------------
 * Replaces reference AcousticEncoder (audiotoken/encoder.py:29-57: ctor builds
 * EncodecModel.encodec_model_24khz(), forward = model.encoder -> model.quantizer.encode -> transpose ->
 * int16) and AcousticDecoder (audiotoken/decoder.py:50-76). */
typedef struct at_encodec at_encodec_t;

/* Create an empty model bound to `device_id` (replaces encoder.py:38-39 `EncodecModel...to(device)`). */
at_encodec_t* at_encodec_create(int device_id);

/* Hand one named host tensor (float32) to the model. Names are the `encodec` checkpoint keys with the
 * weight-norm pair already folded to a plain `.weight` (W = g*v/||v||, the tensor the reference convolves
 * with): "encoder.model.0.conv.conv.weight" [32,1,7] / ".bias", "encoder.model.{1,4,7,10}.block.{1,3}.conv.conv.*",
 * "encoder.model.{1,4,7,10}.shortcut.conv.conv.*", "encoder.model.{3,6,9,12}.conv.conv.*",
 * "encoder.model.13.lstm.{weight_ih,weight_hh,bias_ih,bias_hh}_l{0,1}", "encoder.model.15.conv.conv.*",
 * "quantizer.vq.layers.{k}._codebook.embed" [1024,128] (optional ".e2" [1024] = row-wise sum of squares),
 * and for decode "decoder.model.*" ("…convtr.convtr.weight" is [in,out,k]). */
int at_encodec_set_tensor(at_encodec_t* h, const char* name, const float* host_data, const int64_t* shape, int ndim);

/* Repack to kernel layouts, upload, free host staging. with_decoder != 0 also requires the decoder tensors. */
int at_encodec_finalize(at_encodec_t* h, int with_decoder);
void at_encodec_destroy(at_encodec_t* h);
int at_encodec_num_codebooks(const at_encodec_t* h);

/* Workspace size for at_encodec_encode on B clips of N samples. */
size_t at_encodec_workspace_bytes(const at_encodec_t* h, int B, int N);

/* Replaces AcousticEncoder.forward (audiotoken/encoder.py:44-57).
 *   wav   device float32 [B][N]           (24 kHz mono, any N >= 321: the stage-3 strided conv reflects 8 of its ceil(N/40) input rows, and a
 *                                          shorter clip is refused with "clip too short for the strided convs". Clips of 321..1920 samples, T = 2..6
 *                                          frames, follow the reference's short-input rule in the final conv: rows zero-extended to 7, then reflected)
 *   mask  device float32 [B][N] or NULL   — ignored, exactly as the reference ignores attention_mask
 *   n_q   number of codebooks in {1..loaded}; the reference derives it from the bandwidth (encoder.py:50-52)
 *   codes device int16   [B][n_q][T], T = ceil(N/320) returned through *T_out (may be NULL)
 *   emb_out optional device float32 [B][T][128]: the pre-quantiser embedding (parity taps; NULL in production) */
int at_encodec_encode(at_encodec_t* h, const float* wav, const float* mask, int B, int N, int n_q, int16_t* codes,
                      int* T_out, float* emb_out, void* workspace, size_t workspace_bytes, at_stream_t stream);

/* Same as at_encodec_encode, plus a device uint32 status word (stream-ordered): 0 on success; bit 0 (1) = a bounded wait inside the
 * persistent LSTM kernel gave up (the call still terminates); bit 1 (2) = an activation did not fit the fp16 range of an f16x2 kernel ("chain_f16x2",
 * "ih_f16x2", "res_f16x2", "rvq_f16x2", "fin_f16x2"). In both cases the codes are invalid and the caller repeats the batch on the safe path (options
 * persistent_lstm = 0 / chain_f16x2 = ih_f16x2 = res_f16x2 = rvq_f16x2 = fin_f16x2 = 0). Bit 2 (4) = a NaN or an infinity reached the RVQ search (a
 * non-finite sample in `wav`, as a rule): repeating does not help; the reference emits arbitrary codes for such input without a diagnostic.
 * THREADING: a handle carries per-call bookkeeping (the range table the status word is combined from, zeroed at the start of every call), so the
 * *_checked / range_report calls of ONE handle must be issued on one stream at a time — two concurrent calls on the same handle (an encode and a
 * decode included) can clear each other's flags. Use one handle per stream. The same holds for at_w2vbert_* and at_hubert_* handles and for the
 * handle-less at_op_*_split entry points (one range pair per device). */
int at_encodec_encode_checked(at_encodec_t* h, const float* wav, const float* mask, int B, int N, int n_q, int16_t* codes,
                              int* T_out, float* emb_out, void* workspace, size_t workspace_bytes, at_stream_t stream,
                              uint32_t* status_dev);

/* ---- streaming acoustic encode: the same tokens as one at_encodec_encode of the concatenated audio, in bounded memory ----------------------
 * Every conv of the encoder is causal and the only unbounded memory is the LSTM, so a stream carries a small fixed-size state per clip:
 * the last 640 consumed samples (two frames: a frame depends on samples back to 320 t - 478), h and c of both LSTM layers, the last 6 input
 * rows of the final k = 7 conv. A push encodes [640 context samples | n_new new samples] with the one-shot kernels, drops the two context
 * frames, runs the LSTM over the new frames from the carried (h, c) and the final conv over [6 carried rows | new rows]. The first push of a
 * stream has no context: its left reflect padding is the true one.
 *   state   device memory, at_encodec_stream_state_bytes(h, B) bytes, 16-byte aligned; B streams advance in lockstep (same n_new). The
 *           handle keeps a host-side note per state ADDRESS (B, started, finished) — made by at_encodec_stream_reset and by every push for
 *           its state_out — so argument errors are found without synchronising the device. A state therefore cannot be moved or copied
 *           behind the library's back, and it belongs to the handle that reset it.
 *   TRANSACTION RULE: a push reads state_in and writes state_out, which must be two buffers. If the status word of a push is non-zero its
 *           codes AND state_out are invalid; state_in is untouched, so the caller changes the options (as for at_encodec_encode_checked) and
 *           repeats the same push from the same state_in. On success the caller swaps the two buffers.
 *   n_new   a positive multiple of 320 unless `final`; the first push of a stream needs >= 2240 samples (7 frames) unless `final`. The caller
 *           buffers what does not fill a frame yet (AcousticStream in audiotoken_amd/streaming.py does).
 *   final   != 0: the last samples of the stream, any n_new >= 0; the one-shot path's right-edge padding applies inside the window and
 *           T = ceil(n_new / 320). The stream is finished: a further push from state_out is an error until at_encodec_stream_reset.
 *           A stream whose FIRST push is the final one is a one-shot encode: it needs n_new >= 321 like at_encodec_encode.
 *   codes   device int16 [B][n_q][T], T returned through *T_out (n_new / 320, or ceil for the final push); emb_out optional [B][T][128].
 * BIT-IDENTITY: where the one-shot call and the pushes select the same kernels (an even total length with the stage-1 / stage-2 / stage-3
 * lengths divisible by 4 / 5 / 8, i.e. any multiple of 320, pushed in multiples of 320) codes and embeddings are bit-identical to
 * at_encodec_encode's under the same options (profiles/stream_encode.txt; with "lstm_f16x2" = 0 a push runs the fp32 persistent recurrence).
 * Otherwise (an odd or ragged total: the one-shot call then selects other kernels than the frame-aligned windows do) the tokens agree and the
 * embeddings differ in the last bits, as between the kernel options of at_encodec_set_option.
 * Argument errors (null state, state_in == state_out, a state this handle does not know, another B, n_new not a multiple of 320 without
 * final, a first push below 2240 samples without final, a workspace below at_encodec_stream_workspace_bytes, a push after final) return
 * non-zero with at_last_error set; nothing is launched and the device stays usable. */
size_t at_encodec_stream_state_bytes(const at_encodec_t* h, int B);
int at_encodec_stream_reset(at_encodec_t* h, void* state_dev, int B, at_stream_t stream);
/* Workspace of one push of n_new samples: that of a one-shot encode of the window (B, 640 + n_new), whatever was pushed before. */
size_t at_encodec_stream_workspace_bytes(const at_encodec_t* h, int B, int n_new);
int at_encodec_encode_stream_checked(at_encodec_t* h, const void* state_in, void* state_out, const float* wav_new, int B, int n_new, int final,
                                     int n_q, int16_t* codes, int* T_out, float* emb_out, void* workspace, size_t workspace_bytes,
                                     at_stream_t stream, uint32_t* status_dev);

/* Options (they select kernels or bound memory; all but the "*_x3" / "*_f16x2" ones leave the results bit-identical). The product runs the
 * defaults; the others exist as the per-batch range fallback of AcousticEncoder.verified ("*_f16x2" = 0: three bf16 pieces, fp32 exponent range), as
 * the machine fallback ("persistent_lstm" = 0) and as the A/B twins the parity tests compare against (fp32 kernels, unfused GEMM paths). Environment
 * switches are limited to $AUDIOTOKEN_BF16X3_ACOUSTIC, $AUDIOTOKEN_X3_KERNELS (A/B masks of tools/ab_x3.sh), $AUDIOTOKEN_LSTM_STEPWISE and
 * $AUDIOTOKEN_SUBBATCH: round 2's per-option variables were removed.
 *   "persistent_lstm" 1/0 — whole-sequence persistent LSTM kernel (default on) or one launch per time step;
 *   "fused_stage0", "fused_res64", "fused_res128", "fused_down64", "fused_dectail" 1/0 — fused SEANet kernels (default on)
 *   or the GEMM path; "fused_stage1" 1/0 — the 64-channel block and the stage-1 strided conv in ONE kernel (seanet_res64down.hip, default on;
 *   needs "fused_res64", "fused_down64", "res64_x3", "down64_x3", "res_f16x2"; bit-identical to the two kernels it replaces);
 *   "stage0_x3", "res64_x3", "res128_x3", "down64_x3", "down128_x3", "down256_x3", "res256_x3", "lstm_x3", "rvq_x3" 1/0 — the fused kernels, the
 *   stage-2 / stage-3 convs + 256-channel block (as chained GEMMs) the LSTM recurrence and the RVQ search on the bf16 matrix cores with exact 3-way bf16 splits of every
 *   operand (default on; $AUDIOTOKEN_X3_KERNELS bit mask, bits 3, 2, 1, 0, 4, 5, 6, 7, 8 in that order; 0 = the fp32-MFMA kernels:
 *   same tokens, embeddings differ in the last bits);
 *   "ih_f16x2", "chain_f16x2" 1/0 — the two LSTM input projections (encoder and decoder) / the encoder's stage-2 strided conv, 256-channel block
 *   and stage-3 strided conv (the GEMM chain) as two-piece fp16 operand splits, three MFMA products (default on)
 *   or as the three-piece bf16 splits, six products; see csrc/gemm_bf16x3.h;
 *   "res_f16x2", "rvq_f16x2" 1/0 — the fused SEANet kernels of the encoder (stage 0, the 64- and 128-channel residual blocks, the stage-1 strided conv) /
 *   the RVQ search on the same two-piece fp16 scheme (default on) or on three bf16 pieces;
 *   "res128_rs" 1/0 — the 128-channel block on the fp16 scheme as the role-split kernel (csrc/seanet_res128rs.hip, default) or as
 *   csrc/seanet_res128x3.hip; bit-identical results;
 *   "up_f16x2" 1/0 — the decoder's first three transposed convs as two-tap windowed split GEMMs on the fp16 scheme (default on) or as fp32-MFMA GEMMs;
 *   "fin_f16x2" 1/0 — the encoder's final k = 7 conv as a windowed split GEMM on the two-piece fp16 scheme (default on) or on
 *   the fp32 MFMA;
 *   "lstm_f16x2" 1/0 — the persistent LSTM's recurrent product on the two-piece fp16 scheme (h in (-1, 1) always fits: no range check) or on
 *   three bf16 pieces (default on; needs "lstm_x3" = 1);
 *   "dec_skip_twin" 1/0 — TEST-ONLY twin (default 0): one-shot decode and a decode stream's first push store through the tail kernels' skip / stride
 *   variant with skip = 0 and a dense stride; bit-identical results;
 *   "lstm_spin_limit" n >= 0 — polls of a hand-off flag before a workgroup of the persistent LSTM gives up and the status word of the
 *   *_checked entry points becomes 1 (default 2^18, i.e. 0.1-0.3 s; 0 makes the first unready poll give up — used by the tests);
 *   "subbatch" n >= 1 — clips per pass through the conv stack (default 256 or $AUDIOTOKEN_SUBBATCH): bounds
 *   at_encodec_workspace_bytes / at_encodec_decode_workspace_bytes, which must be re-queried after changing it. */
int at_encodec_set_option(at_encodec_t* h, const char* name, int value);
/* Current value of an option of at_encodec_set_option, or -1 for an unknown name. */
int at_encodec_get_option(const at_encodec_t* h, const char* name);

/* Optional timing taps for the benchmark: when enabled, encode brackets each kernel group (conv0, res0..3,
 * down0..3, lstm_ih, lstm_rec, final_conv, rvq) with HIP events recorded on the launch stream.
 * at_encodec_profile(h, enable) resets the accumulated spans. at_encodec_profile_read synchronises on the
 * recorded events and returns the number of groups (names '\n'-separated), or a negative error code. */
int at_encodec_profile(at_encodec_t* h, int enable);
int at_encodec_profile_read(at_encodec_t* h, char* names, size_t names_cap, float* total_ms, int* launches, int max_groups);

size_t at_encodec_decode_workspace_bytes(const at_encodec_t* h, int B, int T);

/* Replaces AcousticDecoder.forward (audiotoken/decoder.py:66-76): codes device int64 [B][K][T] ->
 * wav device float32 [B*320*T] (the reference's [1, B*320*T] row). A NEGATIVE code means "no code": it adds no code-book row, so a frame whose K codes
 * are all negative enters the decoder as a zero embedding row. That is how a clip shorter than the 7 frames a decode needs is extended
 * (decode_batch_files): the reference zero-extends a short input in front of its first reflect padding, and frames behind a clip's end never reach earlier
 * samples (the decoder is causal). Codes above 1023 are clamped to 1023. */
int at_encodec_decode(at_encodec_t* h, const int64_t* codes, int B, int K, int T, float* wav, void* workspace,
                      size_t workspace_bytes, at_stream_t stream);
/* Same, plus the device status word of at_encodec_encode_checked (the decoder runs the same persistent LSTM). */
int at_encodec_decode_checked(at_encodec_t* h, const int64_t* codes, int B, int K, int T, float* wav, void* workspace,
                              size_t workspace_bytes, at_stream_t stream, uint32_t* status_dev);

/* ---- streaming acoustic decode: the waveform of one at_encodec_decode of the concatenated tokens, frame by frame, in bounded memory -------------
 * Every conv of the decoder is causal, so a stream carries per clip: the last 6 rows of the quantised embedding z (128 wide, the history of the
 * k = 7 first conv), h and c of both LSTM layers, and the last 2 rows of ELU(lstm + skip) (512 wide). A push of t_new frames gathers the code-book
 * rows of the new codes behind the carried z rows, runs the first conv over that window without padding, continues the LSTM from the carried
 * (h, c) over the new rows and runs the upsampling stack on [2 carried rows | new rows] with the one-shot kernels; the first 640 samples of the
 * window (an output sample n reaches back to row floor(n / 320) - 2) are never stored. The first push of a stream carries nothing and drops
 * nothing: it IS a one-shot decode of its frames (same kernels, same bits) that also writes the state, and like one it needs t_new >= 7.
 *   state   device memory, at_encodec_decode_stream_state_bytes(h, B) bytes (B * 3840 floats: z rows, h0, c0, h1, c1, y rows), 16-byte aligned.
 *           The handle keeps the same host-side note per state ADDRESS as for the encode stream, with the direction: a decode state is refused by
 *           at_encodec_encode_stream_checked and an encode state by at_encodec_decode_stream_checked.
 *   TRANSACTION RULE: as for the encode stream — state_in != state_out; a push whose status word is non-zero left wav_out and state_out
 *           invalid and state_in untouched, and is repeated from the same state_in after changing the options; on success the caller swaps.
 *   codes_new device int64 [B][K][t_new]; wav_out device float [B][320 * t_new].
 * ROUTES: a push takes every route of at_encodec_decode under the handle's options ("persistent_lstm", "lstm_pipe", "lstm_x3", "lstm_f16x2",
 * "fused_dectail", "dec_chain", "up_f16x2", "res_f16x2", "tail_f16x2"), on windows as short as 3 rows. As for the encode stream, the three-piece
 * bf16 recurrence has no state variant: with "lstm_f16x2" = 0 a push runs the fp32 persistent recurrence. A mid-stream push stores through the
 * skip / stride variant of the tail kernels (compile-time; "dec_skip_twin" = 1 sends one-shot decode and first pushes through the same variant with
 * skip = 0 and a dense stride — bit-identical, the option exists for the tests).
 * BIT-IDENTITY to at_encodec_decode of the same handle and options holds for a stream's first push (any B, K, t_new >= 7). Later pushes run the
 * same arithmetic on other tiles (window-relative tile boundaries select the GEMM's interior or boundary body, the LSTM's projection GEMM sees
 * another M): they agree with one-shot decode to rounding and are held to the oracle's bar only (profiles/stream_decode.txt).
 * Argument errors (null state, state_in == state_out, a state this handle does not know, an encode state, another B, t_new < 1, a first push
 * with t_new < 7, a workspace below at_encodec_decode_stream_workspace_bytes, a handle finalized without a decoder) return non-zero with
 * at_last_error set; nothing is launched and the device stays usable. */
size_t at_encodec_decode_stream_state_bytes(const at_encodec_t* h, int B);
int at_encodec_decode_stream_reset(at_encodec_t* h, void* state_dev, int B, at_stream_t stream);
/* Workspace of one push of t_new frames: a one-shot decode's of (B, t_new + 2) plus the two windows, whatever was pushed before. */
size_t at_encodec_decode_stream_workspace_bytes(const at_encodec_t* h, int B, int t_new);
int at_encodec_decode_stream_checked(at_encodec_t* h, const void* state_in, void* state_out, const int64_t* codes_new, int B, int K, int t_new,
                                     float* wav_out, void* workspace, size_t workspace_bytes, at_stream_t stream, uint32_t* status_dev);

/* ---- stream pools: rows of a stream state that start and finish on their own ---------------------------------------------
 * The B rows of one push advance in lockstep, but WHICH streams form those rows may change from push to push. A pool is an ordinary stream state for S
 * streams (at_encodec_stream_state_bytes(h, S) / at_encodec_decode_stream_state_bytes(h, S) bytes, zeroed and made known to the handle by the matching
 * *_stream_reset with B = S); stream i lives in row ("slot") i of every plane of the state. The pushes themselves are unchanged: they run on staging states
 * of B rows, and two copies move rows between the pool and the staging states.
 *   gather    row b of every plane of state_out (a B-stream state, *_stream_state_bytes(h, B) bytes) = row slots[b] of the pool's plane. The handle notes
 *             state_out as (B, started, not finished), so the next push accepts it as a mid-stream state.
 *   scatter   the inverse, from a state this handle knows (reset, gathered or written by a push) that is not finished: row slots[b] of the pool's planes =
 *             row b of state_in's. The pool's other rows are not touched.
 *   slots     B distinct slots in [0, S), given twice: slots_host (host memory) is what the call validates, slots_dev (device int32 [B], uploaded by the
 *             caller as the feeder uploads its descriptors) is what the kernel reads. The two must hold the same numbers; the kernel skips a row whose
 *             device slot lies outside [0, S).
 * TRANSACTION RULE for the pool: gather(pool -> staging_in); push staging_in -> staging_out with the unchanged *_stream_checked; read the status word and,
 * when it is non-zero, repeat the push from staging_in as for any stream; only after a push that succeeded scatter(staging_out -> pool). A failed push
 * therefore never reaches the pool. Rows that start a stream need no gather (reset the staging state instead), rows on their final encode push no scatter
 * (the slot is free afterwards). Streams that are pushed together through a pool give bit for bit what the same rows give as one lockstep stream of B: the
 * copies are exact and the push is the same call.
 * Each call is stream-ordered, one launch of a pure copy kernel (23 040 bytes per encode stream, 15 360 per decode stream), and neither synchronises nor
 * allocates device memory. Argument errors (a null pointer, B < 1, B > S, a slot outside [0, S), a duplicate slot, a pool this handle did not reset for S
 * streams of that direction, a state_in it does not know or of another B or direction or finished, state == pool) return non-zero with at_last_error set;
 * nothing is launched and the device stays usable. */
int at_encodec_stream_gather(at_encodec_t* h, const void* pool, int S, const int32_t* slots_dev, const int32_t* slots_host, int B, void* state_out,
                             at_stream_t stream);
int at_encodec_stream_scatter(at_encodec_t* h, const void* state_in, int B, const int32_t* slots_dev, const int32_t* slots_host, void* pool, int S,
                              at_stream_t stream);
int at_encodec_decode_stream_gather(at_encodec_t* h, const void* pool, int S, const int32_t* slots_dev, const int32_t* slots_host, int B, void* state_out,
                                    at_stream_t stream);
int at_encodec_decode_stream_scatter(at_encodec_t* h, const void* state_in, int B, const int32_t* slots_dev, const int32_t* slots_host, void* pool, int S,
                                     at_stream_t stream);

/* ---- semantic_m tokenizer: log-mel front-end + Wav2Vec2-BERT conformer + LayerNorm + VQ ------------------
 * Replaces reference Wav2VecBertEncoder (audiotoken/encoder.py:111-186): ctor = Wav2VecBertProcessor +
 * Wav2Vec2BertModel.from_pretrained + VectorQuantize(dim=1024, codebook_size=2048) (:112-161); forward =
 * processor -> model(..., output_hidden_states=True).hidden_states[output_layer] -> LayerNorm(no affine) ->
 * vq -> int16 [B,1,T'] (:163-184), with the attention of audiotoken/modeling_wav2vec2_bert.py:20-80. */
typedef struct at_w2vbert at_w2vbert_t;

at_w2vbert_t* at_w2vbert_create(int device_id);

/* Named host tensors (float32): the HF Wav2Vec2BertModel state-dict keys ("feature_projection.*",
 * "encoder.layers.{i}.*" for consecutive i from 0), "vq._codebook.embed" [1,2048,1024] (the VectorQuantize
 * state-dict key, reference audiotoken/utils.py:331-339; optional "vq._codebook.e2" [2048]), and the two front-end
 * tables of reference processors.py:66-78: "frontend.window" [400], "frontend.mel_filters" [257,80]. */
int at_w2vbert_set_tensor(at_w2vbert_t* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int at_w2vbert_finalize(at_w2vbert_t* h);
/* The finalized model as ONE device blob, for start-up at N > 1 (weights cross xGMI once): one rank reads, folds, uploads and splits
 * the checkpoint and exports; the others import what one RCCL broadcast delivered — no D2H copy, no second host pass over 1.8 GB, no split kernels.
 * (The reference has no counterpart: audiotoken/core.py:66 is single-device; every process would call from_pretrained itself.)
 *   packed_bytes(h)                       size of the blob of a finalized handle (-1: not finalized)
 *   packed_meta(h, host_dst, cap)         the host-side record (block sizes, max |w| per tensor, layer count, arithmetic): returns its size, writes it
 *                                         when cap is large enough (call with NULL / 0 first)
 *   export_packed(h, device_dst, bytes, stream)   concatenate the handle's device allocations into device_dst (stream-ordered D2D copies)
 *   import_packed(h, meta, meta_bytes, device_src, bytes, stream)   on a FRESH handle (create only): copy the blob into one allocation owned by the handle
 *                                         and rebuild the model over it; the handle is finalized afterwards, device_src may be freed. Fails (-1,
 *                                         at_last_error) when the record does not match this build's allocation order / sizes.
 * Both sides must be the same build of this library on the same architecture; the blob is not a file format. */
int64_t at_w2vbert_packed_bytes(at_w2vbert_t* h);
int64_t at_w2vbert_packed_meta(at_w2vbert_t* h, void* host_dst, int64_t cap);
int at_w2vbert_export_packed(at_w2vbert_t* h, void* device_dst, int64_t bytes, void* stream);
int at_w2vbert_import_packed(at_w2vbert_t* h, const void* host_meta, int64_t meta_bytes, const void* device_src, int64_t bytes, void* stream);
void at_w2vbert_destroy(at_w2vbert_t* h);
int at_w2vbert_num_layers(const at_w2vbert_t* h);

/* T' = pad_to_multiple(floor((1 + floor((N-400)/160)) / 2)) (reference processors.py:158,246-259). */
int at_w2vbert_num_tokens(int N, int pad_to_multiple_of);
size_t at_w2vbert_workspace_bytes(const at_w2vbert_t* h, int B, int N, int pad_to_multiple_of);

/* Replaces Wav2VecBertEncoder.forward (audiotoken/encoder.py:163-184).
 *   wav device float32 [B][N] (16 kHz); mask device float32 [B][N] (1 = real sample) or NULL (= all ones)
 *   pad_to_multiple_of: the reference's third argument (default 2)
 *   n_layers: conformer layers to run = the reference's output_layer (19; hidden_states[n] is the output of layer n-1)
 *   tokens device int16 [B][1][T'] or NULL (then no VQ); *T_out = T'
 *   parity taps, all optional (NULL in production): features_out [B][T'][160], attn_mask_out [B][T'],
 *   hidden_out [B][T'][1024] = hidden_states[n_layers]. */
int at_w2vbert_encode(at_w2vbert_t* h, const float* wav, const float* mask, int B, int N, int pad_to_multiple_of, int n_layers,
                      int16_t* tokens, int* T_out, float* features_out, float* attn_mask_out, float* hidden_out, void* workspace,
                      size_t workspace_bytes, at_stream_t stream);
/* Same as at_w2vbert_encode, plus a device int32 status word (stream-ordered: zeroed at the start of the call, final when the call's work
 * has completed): bit 1 (value 2) = an activation did not fit the fp16 range of the "f16x2" arithmetic (|x| > 65504 / 16) — the
 * tokens are then invalid and the caller should repeat the batch after at_w2vbert_set_option(h, "arith", 1); bit 2 (value 4) = a NaN or an
 * infinity reached the quantiser (a non-finite sample in `wav`): repeating does not help. One stream per handle (see at_encodec_encode_checked). */
int at_w2vbert_encode_checked(at_w2vbert_t* h, const float* wav, const float* mask, int B, int N, int pad_to_multiple_of, int n_layers,
                              int16_t* tokens, int* T_out, float* features_out, float* attn_mask_out, float* hidden_out, void* workspace,
                              size_t workspace_bytes, at_stream_t stream, int32_t* status_dev);
/* Options. "arith": arithmetic of the eight linear layers per conformer layer — 0 = f32-input MFMA; 1 = "bf16x3": exact 3-way bf16
 * operand splits, six products on the bf16 matrix cores; 2 = "f16x2" (default, also $AUDIOTOKEN_SEMANTIC_ARITH=f32|bf16x3|f16x2): two fp16
 * pieces per operand, three products, operands pre-scaled by powers of two (fp32-class accuracy: csrc/gemm_bf16x3.h). Weights are split
 * for a scheme the first time it is selected. "dwconv_stream" 1/0 (default 1): the conv module's depthwise conv + LayerNorm + swish as the streaming
 * kernel (csrc/dwconv_stream.hip: one channel per thread walking along time) or the register-stationary one — bit-identical results, the option is
 * the A/B twin the tests compare. "vq_split" 1/0 (default 1): the VQ score GEMM (LayerNorm output x code book) on the split kernel with the handle's
 * arithmetic, or on the fp32 MFMA (always with "arith" = 0). at_w2vbert_get_option returns the current value (or -1). */
int at_w2vbert_set_option(at_w2vbert_t* h, const char* name, int value);
int at_w2vbert_get_option(const at_w2vbert_t* h, const char* name);
int at_w2vbert_profile(at_w2vbert_t* h, int enable);
int at_w2vbert_profile_read(at_w2vbert_t* h, char* names, size_t names_cap, float* total_ms, int* launches, int max_groups);

/* ---- semantic_s tokenizer: mHuBERT-base + k-means ---------------------------------------------------------
 * Replaces reference HubertEncoder (audiotoken/encoder.py:60-108): ctor = HubertModel.from_pretrained + joblib k-means
 * centres (:61-85); __call__ = model(..., output_hidden_states=True).hidden_states[output_layer] -> LayerNorm(no
 * affine) -> torch.cdist -> argmin -> int16 [B,1,T] (:87-108). Input is the waveform AFTER hubert_processor
 * (zero-mean / unit-variance, encoder.py:20-26), which the reference applies on the host before batching. */
typedef struct at_hubert at_hubert_t;
at_hubert_t* at_hubert_create(int device_id);
/* HF HubertModel state-dict keys; the positional conv's weight-norm pair folded by the caller (dim = 2) into
 * "encoder.pos_conv_embed.conv.weight" [768,48,128]; "kmeans.cluster_centers_" [1000,768] (optional "kmeans.c2" [1000]). */
int at_hubert_set_tensor(at_hubert_t* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int at_hubert_finalize(at_hubert_t* h);
/* the finalized model as one device blob: as at_w2vbert_packed_bytes / _packed_meta / _export_packed / _import_packed above */
int64_t at_hubert_packed_bytes(at_hubert_t* h);
int64_t at_hubert_packed_meta(at_hubert_t* h, void* host_dst, int64_t cap);
int at_hubert_export_packed(at_hubert_t* h, void* device_dst, int64_t bytes, void* stream);
int at_hubert_import_packed(at_hubert_t* h, const void* host_meta, int64_t meta_bytes, const void* device_src, int64_t bytes, void* stream);
void at_hubert_destroy(at_hubert_t* h);
int at_hubert_num_layers(const at_hubert_t* h);
/* T = chained floor((L - k)/s) + 1 over the 7 feature-extractor convs (HF modeling_hubert.py:664-677). */
int at_hubert_num_tokens(int N);
size_t at_hubert_workspace_bytes(const at_hubert_t* h, int B, int N);
/* wav device float32 [B][N] (normalised, 16 kHz); mask device float32 [B][N] or NULL; n_layers = output_layer (11);
 * tokens device int16 [B][1][T] or NULL; hidden_out optional device float32 [B][T][768] = hidden_states[n_layers]. */
int at_hubert_encode(at_hubert_t* h, const float* wav, const float* mask, int B, int N, int n_layers, int16_t* tokens, int* T_out,
                     float* hidden_out, void* workspace, size_t workspace_bytes, at_stream_t stream);
/* As at_w2vbert_encode_checked / at_w2vbert_set_option / at_w2vbert_get_option: device status word (bit 1 = fp16 range overflow of the
 * "f16x2" arithmetic) and the "arith" option (0 f32 MFMA, 1 bf16x3, 2 f16x2 = default; also covers the six 512->512 feature-extractor convs). */
int at_hubert_encode_checked(at_hubert_t* h, const float* wav, const float* mask, int B, int N, int n_layers, int16_t* tokens, int* T_out,
                             float* hidden_out, void* workspace, size_t workspace_bytes, at_stream_t stream, int32_t* status_dev);
/* Test tap: the conv feature encoder alone — the stage at_hubert_encode_checked runs first, on the handle's current "arith", over the same workspace
 * layout (at_hubert_workspace_bytes(h, B, N)). feats_out device float32 [B][T][512] = the seventh conv's GELU output, T = at_hubert_num_tokens(N).
 * status_dev: nullable device word, the OR of the front end's range sites (bit 1 = fp16 range overflow). */
int at_hubert_features(at_hubert_t* h, const float* wav, int B, int N, float* feats_out, void* workspace, size_t workspace_bytes, at_stream_t stream,
                       int32_t* status_dev);
int at_hubert_set_option(at_hubert_t* h, const char* name, int value);
int at_hubert_get_option(const at_hubert_t* h, const char* name);
int at_hubert_profile(at_hubert_t* h, int enable);
int at_hubert_profile_read(at_hubert_t* h, char* names, size_t names_cap, float* total_ms, int* launches, int max_groups);

/* ---- input side of encode_batch_files: what the reference does through torchaudio / ffmpeg ------------------------------- */
/* FLAC (RFC 9639), host code: replaces the StreamReader decode of reference audiotoken/utils.py:71-101 for '.flac' members of AUDIO_EXTS. `data` = the whole
 * file in host memory. at_flac_info: STREAMINFO fields (md5_16 nullable: the MD5 of the decoded little-endian PCM, for the caller to verify).
 * at_flac_decode: planar int32 samples out[c * cap_samples_per_channel + i], every frame's CRC-8 / CRC-16 verified; returns samples per channel or a
 * negative code. Thread-safe (no handle, no device). */
int at_flac_info(const uint8_t* data, size_t n, int* sample_rate, int* channels, int* bits_per_sample, int64_t* total_samples, uint8_t* md5_16);
int64_t at_flac_decode(const uint8_t* data, size_t n, int32_t* out, int64_t cap_samples_per_channel);

/* Raw PCM on the device -> the batch the encoders take, in one launch: sample format conversion, the per-chunk resampling of reference
 * audiotoken/utils.py:82-98 (torchaudio Resample defaults), the segmentation / zero padding / mask of reference audiotoken/datasets.py:75-105.
 * One descriptor per output row (built on the host from headers and lengths only; the array lives in device memory):
 *   pcm        device pointer to the decoded file's mono samples in format `fmt`
 *   table      device pointer to the resampling table of (orig, new): float32 [n][2 width + o] (audiotoken_amd/audio_io.py: resample_table) followed by
 *              int32 [n][2] = the non-zero tap range [lo, hi) of every phase; NULL = the file is at the model's rate
 *   chunk_off / chunk_len   the streamed chunk (chunk_size seconds at the SOURCE rate) this row is cut from: every chunk is resampled on its own
 *   out_start / valid_len   the row = samples [out_start, out_start + valid_len) of the resampled chunk, then padding up to seg_len
 *   scale      multiplies integer samples (1 / 32768 for 16-bit WAV, 1 / 2^31 for 24 / 32-bit WAV, 1 / 2^(bits - 1) for FLAC); u8: (x - 128) * scale
 *   o, n, width   orig / g, new / g, half kernel width (o == n when table is NULL)
 * segments [nseg][seg_len] float32, masks [nseg][seg_len] float32 (1 = sample exists; nullable). Stream-ordered, no allocation. */
enum { AT_PCM_S16 = 0, AT_PCM_S32 = 1, AT_PCM_F32 = 2, AT_PCM_U8 = 3 };
typedef struct at_segment_desc {
    const void* pcm;
    const float* table;
    int64_t chunk_off;
    int32_t chunk_len, out_start, valid_len, fmt;
    float scale;
    int32_t o, n, width;
    int32_t chunk_out_len;   /* samples of the whole resampled chunk (ceil(n * chunk_len / o); chunk_len at the model's rate): the span of the per-chunk moments below */
} at_segment_desc;
int at_segments_from_pcm(const at_segment_desc* descs_dev, int nseg, int seg_len, float pad_value, float* segments, float* masks, at_stream_t stream);
/* The same with the reference's per-chunk transform of Tokenizers.semantic_s folded in (round 5): `hubert_processor` = HF Wav2Vec2FeatureExtractor with
 * do_normalize (reference audiotoken/encoder.py:20-26), applied by the reference to every streamed chunk BEFORE it is cut and padded
 * (audiotoken/datasets.py:78-79): valid samples become (x - mean) / sqrt(var + eps) with mean / population variance over the row's whole resampled chunk
 * (float64 sums in a fixed order: deterministic), eps = 1e-7; padding stays pad_value. workspace: at_segments_zmuv_workspace_bytes(nseg, max over rows of
 * chunk_out_len) bytes of device memory. Three launches, stream-ordered, no allocation. */
size_t at_segments_zmuv_workspace_bytes(int nseg, int max_chunk_out_len);
int at_segments_from_pcm_zmuv(const at_segment_desc* descs_dev, int nseg, int seg_len, int max_chunk_out_len, float pad_value, float eps, float* segments,
                              float* masks, void* workspace, size_t workspace_bytes, at_stream_t stream);

/* ---- stateful resampling of streamed audio: the rule of at_segments_from_pcm at GLOBAL sample positions -------------------------------
 * A signal of L source samples has outputs j in [0, ceil(n L / o)): with f = j / n, p = j % n, base = f o - width,
 *   y[j] = sum over k in [lo_p, hi_p), ascending, of one fmaf(K[p][k], x[base + k], acc),   x[s] = 0 for s < 0 or s >= L
 * (table, phases and tap ranges as in at_segment_desc; the sample conversion too). A row evaluates `out_len` consecutive outputs from a WINDOW of the signal,
 * so a signal pushed in pieces, each with the tail of the one before in front, gets the samples of resampling it once. One descriptor per row:
 *   pcm        device pointer to the window's samples in format `fmt`; table: as in at_segment_desc, NULL = native rate (o = n = 1, width = 0: conversion only)
 *   src_base   global index of pcm[0] (negative for a window that opens with stored zeros before the signal); src_len: samples of the window
 *   src_total  L, read when `final` is non-zero: taps at s >= L are zeros. A row that is not final may only have taps inside its window
 *   out_start  global j of the row's first output; out_len outputs are written to out + dst_off (floats), nothing else is touched
 * at_resample_rows: ONE launch for all rows (they may differ in rate, format and length); stream-ordered, no allocation; it trusts the descriptors.
 * at_resample_rows_check: host code over a HOST copy of the descriptors, to be called before every launch: 0, or a negative code with at_last_error set for
 * a null pointer, nrows < 1, a negative length or offset, an unknown fmt, o / n / width that do not belong together (o and n coprime, width =
 * ceil(6 o / (0.99 min(o, n))), a table exactly when o != n), a row that is not final with a tap (k in [0, 2 width + o)) outside its window, a final row
 * with a tap inside [0, src_total) but outside its window, or outputs past ceil(n src_total / o). */
typedef struct at_resample_row {
    const void* pcm;
    const float* table;
    int64_t src_base, src_len, src_total, out_start;
    int32_t out_len, fmt;
    float scale;
    int32_t o, n, width, final;
    int32_t reserved;
    int64_t dst_off;
} at_resample_row;
int at_resample_rows(const at_resample_row* rows_dev, int nrows, float* out, at_stream_t stream);
int at_resample_rows_check(const at_resample_row* rows_host, int nrows);

/* ---- output side of decode_batch_files: the decoder's float32 batch -> compacted 16-bit PCM ------------------------------------------
 * One descriptor per row (built on the host; the array lives in device memory):
 *   src_off   first sample of the row, in floats from `src` (the padded decoder output [B][320 T_max]: src_off = b * 320 * T_max)
 *   dst_off   first sample of the row in the packed output, in int16 elements from `dst` (rows follow each other without gaps)
 *   n         samples of the row (320 * valid frames)
 *   scale     multiplies every finite sample before the clamp (1, or the file's min(0.99 / peak, 1) computed in fp32 on the host)
 * The entry points trust the descriptors: every [src_off, src_off + n) must lie inside `src` and every [dst_off, dst_off + n) inside `dst`.
 * at_pcm_peaks: peaks[r] = max |x| over the FINITE samples of row r (0 for a row without one); an integer atomic max on the bit pattern, so the result does
 * not depend on scheduling. at_pcm_pack, per sample: NaN -> 0 and +-infinity -> +-limit (both counted as non-finite); otherwise y = x * scale in fp32,
 * c = min(max(y, -limit), limit), counted as clipped when c != y; q = rint(c * 32768) (round half to even) stored as int16. counts: uint32 [nrows][2] =
 * {clipped, non-finite} per row, zeroed by the call. limit in (0, 32767 / 32768]; max_n >= every row's n (it sizes the grid). Rows whose source and destination
 * are 16-byte aligned (offsets that are multiples of 8 samples from aligned bases) take 16-byte loads and stores; any other row is still converted correctly.
 * Both are stream-ordered and do not allocate; arguments are validated before the device is touched. The reference has no counterpart (it converts on the
 * host: audiotoken/utils.py save_audio). */
typedef struct at_pcm_row_desc {
    int64_t src_off, dst_off, n;
    float scale;
    int32_t reserved;
} at_pcm_row_desc;
int at_pcm_peaks(const float* src, const at_pcm_row_desc* rows_dev, int nrows, int64_t max_n, float* peaks, at_stream_t stream);
int at_pcm_pack(const float* src, const at_pcm_row_desc* rows_dev, int nrows, int64_t max_n, float limit, int16_t* dst, uint32_t* counts, at_stream_t stream);

/* ---- FLAC output (RFC 9639): the decoder's float32 batch -> FLAC subframes on the device, framed on the host --------------------------
 * The stream is mono, 16 bit, variable block size; every row is cut into blocks of AT_FLAC_BLOCK samples plus one shorter last block, one subframe per block.
 * The sample value is the one of at_pcm_pack (same scale, limit, NaN / infinity handling and counts). The subframe rule is stated in DESIGN.md section 14 and
 * at the top of csrc/flac_encode.hip; it is integer arithmetic throughout, so the device encoder and the host twin write IDENTICAL bytes.
 * Row descriptor (built on the host; the array lives in device memory):
 *   src_off      first sample of the row, in floats from `src`
 *   n            samples of the row; the row has ceil(n / 4096) blocks
 *   first_block  index of the row's first block among the launch's blocks: the exclusive prefix sum of the rows' block counts
 *   scale        multiplies every finite sample before the clamp
 * Block record, one per block in row order:
 *   first        first sample of the block inside its row;  n  its samples (1 .. 4096)
 *   kind         AT_FLAC_CONSTANT / AT_FLAC_VERBATIM / AT_FLAC_FIXED;  order  the FIXED predictor order (else 0);  porder  the Rice partition order (else 0)
 *   nbytes       bytes of the subframe (zero-padded to a byte);  byte_off  its place in `bytes`: the exclusive prefix sum of nbytes in record order
 *
 * at_flac_encode_rows: blocks[nblocks], the subframes compacted back to back into `bytes`, counts uint32 [nrows][2] = {clipped, non-finite} per row (zeroed by the
 * call). nblocks must be the sum of the rows' block counts. The worst case is 1 + 2 n bytes per block: size `bytes` (bytes_cap) by nblocks + 2 * sum(n); a
 * subframe that would pass bytes_cap is not written. workspace: at_flac_encode_workspace_bytes(nblocks) bytes of device memory, 16-byte aligned. Stream-ordered,
 * does not allocate; arguments are validated before the device is touched; the descriptors are trusted as those of at_pcm_pack are.
 *
 * at_flac_encode_pcm16: the HOST twin for one row of int16 samples (plain C++): records blocks[0 .. ceil(n / 4096)) with `row` and byte offsets counted from
 * `byte_off`, subframes written to bytes + byte_off onwards (bytes_cap >= byte_off + blocks + 2 n). Returns the number of blocks, or -1.
 *
 * at_flac_write_frames: host. Frames the records in order: frame header (variable block size: the coded number is first_sample_of_row[row] + first; block-size
 * code 12 for 4096, else 6 / 7 with the 8- / 16-bit n - 1 field; sample-rate code of the RFC's table, 0 for a rate outside it; mono; 16 bit) with its CRC-8,
 * the subframe, the table-driven CRC-16. `out` needs 18 + nbytes bytes per frame. Returns the bytes written or -1; stats[7] = {min frame bytes, max frame
 * bytes, min block size over all blocks BUT the call's last (0 when there is one block), max block size, the last block's size, frames, samples}.
 *
 * at_flac_streaminfo: host. The 42-byte stream head: "fLaC", a last-metadata-block STREAMINFO header and its 34 bytes (mono, 16 bit, MD5 all zero = not computed). */
enum { AT_FLAC_BLOCK = 4096 };
enum { AT_FLAC_CONSTANT = 0, AT_FLAC_VERBATIM = 1, AT_FLAC_FIXED = 2 };
typedef struct at_flac_row_desc {
    int64_t src_off, n;
    int32_t first_block;
    float scale;
} at_flac_row_desc;
typedef struct at_flac_block {
    int64_t first, byte_off;
    int32_t row, n, kind, order, porder, nbytes;
} at_flac_block;
size_t at_flac_encode_workspace_bytes(int nblocks);
int at_flac_encode_rows(const float* src, const at_flac_row_desc* rows_dev, int nrows, int nblocks, float limit, at_flac_block* blocks, uint8_t* bytes,
                        int64_t bytes_cap, uint32_t* counts, void* workspace, size_t workspace_bytes, at_stream_t stream);
int64_t at_flac_encode_pcm16(const int16_t* samples, int64_t n, int row, at_flac_block* blocks, int64_t blocks_cap, uint8_t* bytes, int64_t bytes_cap,
                             int64_t byte_off);
int64_t at_flac_write_frames(const at_flac_block* blocks, int nblocks, const uint8_t* bytes, int64_t bytes_len, int sample_rate, const int64_t* first_sample_of_row,
                             int nrows, uint8_t* out, int64_t cap, int64_t* stats);
int at_flac_streaminfo(int sample_rate, int min_block, int max_block, int min_frame, int max_frame, int64_t total_samples, uint8_t* out42);

/* ---- measurement aid (bench.py): the clock the chip held over a stretch of the stream ----------------------------------------------------------------
 * slots_dev: device uint64 [16][2], zeroed by the caller. One tiny launch writes {s_memtime (shader cycles), s_memrealtime (100 MHz)} into slot [xcc] for every
 * XCD a wave of it ran on. Between two stamps A, B on one stream: held clock = (B.memtime - A.memtime) / (B.memrealtime - A.memrealtime) x 100 MHz per XCD
 * (XCDs' counters are not mutually synchronised). No product kernel carries a stamp; the reference has no counterpart. */
int at_clock_stamp(uint64_t* slots_dev, at_stream_t stream);

/* ---- operator-level entry points (the kernels behind the models; used by the parity tests) ------------- */

/* Measured fp16 headroom of the LAST encode / decode of a handle (round 3). Every place where activations are split into fp16 pieces (a "site":
 * a fused SEANet kernel's staging, a GEMM epilogue that writes the next layer's operand, LayerNorm -> pieces, the attention kernel ...) records the
 * largest |x * scale| it saw; the two-piece fp16 arithmetic overflows at 65504 (status bit 1). at_*_range_sites: newline-separated site names
 * (returns the count, or -(bytes needed)); at_*_range_report: max_scaled[k] per site (0 = the site did not run on the fp16 scheme), returns the
 * count. Synchronises the device. */
int at_encodec_range_sites(char* names, size_t cap);
int at_encodec_range_report(at_encodec_t* h, float* max_scaled, int cap);
int at_w2vbert_range_sites(char* names, size_t cap);
int at_w2vbert_range_report(at_w2vbert_t* h, float* max_scaled, int cap);
int at_hubert_range_sites(char* names, size_t cap);
int at_hubert_range_report(at_hubert_t* h, float* max_scaled, int cap);
/* The power of two each split site multiplies its activations by before the fp16 split (round 5). 16 everywhere, except that a site fed by an affine
 * LayerNorm gets, at finalize, the largest power of two s <= 16 with s (sqrt(D) max|gamma| + max|beta|) <= 65 000: |LN(x)_k| <= sqrt(D) |gamma_k| + |beta_k|
 * for any input, so those sites provably cannot overflow whatever the data. at_w2vbert_site_scales: scales[l * n_sites + k] (n_sites and the order of
 * at_w2vbert_range_sites); at_hubert_site_scales: scales[2 l] = input of layer l's q/k/v projection, scales[2 l + 1] = input of its first FFN GEMM. Return
 * the number of floats written. (The reference has no such notion: fp32 throughout, audiotoken/encoder.py:87-108,163-186.) */
int at_w2vbert_site_scales(const at_w2vbert_t* h, float* scales, int cap);
int at_hubert_site_scales(const at_hubert_t* h, float* scales, int cap);
/* Per conformer layer, the OR of its split sites' status flags in the LAST encode (bit 1 = an activation of that layer left the fp16 range). An overflow
 * becomes infinities that every later layer flags as well: the FIRST flagged layer is the cause. Returns the number of layers written (<= cap).
 * Synchronises the device. With option "layer_arith:<i>" (at_w2vbert_set_option; -1 = the handle's "arith", 1 = bf16x3, 2 = f16x2) ONE layer can be moved
 * to the wide-range arithmetic while the others stay on f16x2 — what the product's range fallback does (round 4; the reference has no such notion:
 * its fp32 arithmetic cannot overflow, audiotoken/encoder.py:163-186). */
int at_w2vbert_layer_status(at_w2vbert_t* h, int32_t* flags, int cap);
/* The same for at_hubert_t: flags[0] = conv feature encoder + positional conv, flags[1 + l] = transformer layer l; option "layer_arith:<l>" of
 * at_hubert_set_option moves one transformer layer to bf16x3 / f16x2. */
int at_hubert_layer_status(at_hubert_t* h, int32_t* flags, int cap);

/* Windowed fp32 GEMM: out[b][m][n] = alpha*act(sum_kk A(b,m,kk)*W[n][kk] + bias[n]) (+ R[b][m][n]) with
 * A(b,m,kk) = pro(X[b][m*stride + kk/Cin - pad_left][kk%Cin]); rows outside [0,Tin) reflect (pad_mode=1) or are
 * zero (pad_mode=0). Covers conv1d (ref: encodec SConv1d), Linear and ConvTranspose1d-as-phases. */
typedef struct at_gemm_desc {
    const float* X; int64_t x_bstride; int32_t Tin, Cin, ldx;
    int32_t ktaps, stride, pad_left, pad_mode;
    const float* W; const float* bias;
    float* C; int64_t c_bstride; int32_t ldc;
    const float* R; int64_t r_bstride; int32_t ldr;
    int32_t M, N, K, batch;
    int32_t pro; /* 0 none, 1 ELU, 2 power: A = X[kk]^2 + X[kk+aux_off]^2 */
    int32_t epi; /* 0 none, 1 swish, 2 ELU, 3 GELU(erf), 4 log(max(v, mel_floor)), 5 GLU over interleaved rows */
    float alpha;
    int32_t aux_off;
    const float* row_mask; /* optional [batch*M]: rows with mask 0 are written as zeros */
} at_gemm_desc;
int at_op_gemm(const at_gemm_desc* d, at_stream_t stream);
/* The same call with the second A source filled in (ktaps == 1, K1 == Cin): A(b,m,kk) = pro(X[b][m][kk]) for kk < K1 and X2[b][m][kk - K1] (row stride
 * ld2, clip stride x2_bstride, no prologue) for K1 <= kk < K — the SEANet residual block's fused shortcut. K1 and K - K1 must be multiples of 4. */
int at_op_gemm_dual(const at_gemm_desc* d, const float* X2, int64_t x2_bstride, int ld2, int K1, at_stream_t stream);
/* The route at_op_gemm / at_op_gemm_dual (X2 NULL = single source) would take, without launching anything (pure host code, no device needed):
 * out[0] = tile configuration (0 128x16, 1 128x32, 2 128x64, 3 128x64 with K tile 16, 4 64x64, 5 128x128 with K tile 16, 6 128x128; -1 = nothing to
 * launch), out[1..3] = workgroups over the whole grid (batch included) that take the general, the FAST and the TAP body (csrc/gemm_core.h: gemm_body).
 * Returns the argument check's error code when the call would be refused. */
int at_op_gemm_route(const at_gemm_desc* d, const float* X2, int64_t x2_bstride, int ld2, int K1, int32_t* out);

/* Residual VQ search (ref: encodec ResidualVectorQuantizer.encode; formula SURVEY.md Appendix A.1):
 * x device float32 [rows][128]; codebooks device [n_q][1024][128]; e2 device [n_q][1024];
 * codes int16 written at codes[(row / T)*n_q*T + q*T + row % T]. */
/* The named host tensors (float32, weight-norm already folded) a model's finalize() needs, one per line as "name d0 d1 ...":
 * model "encodec" (n = number of codebooks, with_extras = decoder too), "w2vbert" (n = conformer layers, with_extras = VQ codebook),
 * "hubert" (n = transformer layers, with_extras = k-means centres), "gpt" (n = layers; the embedding shapes listed are the reference's V = 53376 and
 * block = 1024, finalize takes both from the tensors; with_extras is ignored). Returns the number of entries, or -(bytes needed) when buf is NULL or
 * too small. A checkpoint loader can validate its output against this list without a device. */
int at_required_tensors(const char* model, int n, int with_extras, char* buf, size_t cap);

/* The split-operand GEMM of the semantic tokenizers (csrc/gemm_bf16x3.h), for the parity tests: C[M][N] = X[M][K] . W[N][K]^T + bias with both
 * fp32 operands written as 16-bit pieces — scheme 0 = three bf16 pieces / six products, 1 = two fp16 pieces / three products (w_max_abs = max |W|
 * sets the weight scale). kernel: 0 = as the product dispatches, 1 = the two-group kernel (gemm_f16x2_tg.hip), 2 = the register-staged kernel.
 * workspace >= (round_up(M, 256) + N) * K * pieces * 2 bytes. status_dev: nullable device word (bit 1 = fp16 range overflow). */
int at_op_gemm_split(const float* X, const float* W, const float* bias, float* C, int M, int N, int K, int scheme, float w_max_abs,
                     int kernel, void* workspace, size_t workspace_bytes, int32_t* status_dev, at_stream_t stream);
/* A causal conv1d (reflect front padding k - stride; ref: encodec SConv1d) on the WINDOWED two-piece fp16 split GEMM
 * (csrc/gemm_f16x2_tg.hip), for the parity / soak tests: X [B][L][Cin] float32 channels-last, W [Cout][k * Cin] (tap-major), C [B][L / stride][Cout].
 * Cin % 16, Cout % 128, L % stride == 0. workspace >= 2 * (B * Cin * stride * (round_up(L / stride, 256) + (k - 1) / stride + 1) + Cout * k * Cin) * 2 bytes. */
int at_op_conv_split(const float* X, const float* W, const float* bias, float* C, int B, int L, int Cin, int Cout, int ktaps, int stride,
                     float w_max_abs, void* workspace, size_t workspace_bytes, int32_t* status_dev, at_stream_t stream);
int at_op_rvq_encode(const float* x, int64_t rows, int T, const float* codebooks, const float* e2, int n_q,
                     int16_t* codes, at_stream_t stream);
/* The same search on the SPLIT kernel the product runs (csrc/rvq_encode_x3.hip): scheme 1 = two fp16 pieces / three products (default), 0 = three
 * bf16 pieces / six products; cb_max_abs = max |codebook| (the fp16 scheme's power-of-two codebook scale); workspace >= pieces * n_q * 1024 * 128 * 2 + 8
 * bytes; status_dev nullable (bit 1 = fp16 range overflow of the residual). */
int at_op_rvq_encode_split(const float* x, int64_t rows, int T, const float* codebooks, const float* e2, int n_q, int16_t* codes, int scheme,
                           float cb_max_abs, void* workspace, size_t workspace_bytes, int32_t* status_dev, at_stream_t stream);

/* The first HuBERT feature-extractor layer in its fp32-output form (csrc/hubert_kernels.hip; HF modeling_hubert.py:154-176), for the parity tests:
 * conv1d(1 -> 512, k 10, stride 5, valid, no bias) -> GroupNorm(512 groups, eps 1e-5, affine) over the T0 = (N - 10) / 5 + 1 frames -> GELU(erf).
 * wav [B][N], w [512][10], gamma / beta [512], out [B][T0][512], any N >= 10. workspace (16-byte aligned) >= round_up(B * ceil(T0 / 4096) * 520, 256)
 * + B * 4096 bytes: the float64 waveform-moment partials and the per-channel scale / shift. */
int at_op_hub_conv0(const float* wav, const float* w, const float* gamma, const float* beta, float* out, int B, int N, void* workspace,
                    size_t workspace_bytes, at_stream_t stream);
/* HuBERT's frame-level mask (HF modeling_hubert.py:664-693): fmask [B][T] = 1 for t < out_len(sum of the clip's sample mask), else 0, out_len = the
 * chained floor((L - k) / s) + 1 of the seven convs. smask [B][N] of 0 / 1 values, or NULL = every sample valid (out_len(N)). */
int at_op_hub_frame_mask(const float* smask, float* fmask, int B, int N, int T, at_stream_t stream);

/* LayerNorm over the last dim (eps 1e-5); gamma/beta NULL = non-affine; rows with row_mask 0 are zeroed. */
int at_op_layernorm(const float* x, const float* gamma, const float* beta, const float* row_mask, float* y, int64_t rows, int D,
                    at_stream_t stream);

/* Rel-pos attention (ref audiotoken/modeling_wav2vec2_bert.py:46-73): qkv [B*T][3072] = [q|k|v] (16 heads x 64),
 * attn_mask [B*T] (1 = valid key), dist_emb80 [80][64] (73 rows used, rest zero) -> ctx [B*T][1024]. */
int at_op_relpos_attention(const float* qkv, const float* attn_mask, const float* dist_emb80, float* ctx, int B, int T,
                           at_stream_t stream);

/* The same attention on the fp32 matrix-core kernel (csrc/w2vbert_kernels.hip: relpos_attention_kernel), whatever the default arithmetic: what the fine
 * stage launches at every layer. heads 1..64: qkv [B*T][3 * heads * 64], ctx [B*T][heads * 64]; dist_emb80 NULL = no rel-pos bias. */
int at_op_attention_f32(const float* qkv, const float* attn_mask, const float* dist_emb80, float* ctx, int B, int T, int heads, at_stream_t stream);

/* The same attention on the path the product runs (ref audiotoken/modeling_wav2vec2_bert.py:46-73; HF HubertAttention with dist_emb80 = NULL): k / v are
 * first written as the row-major fp16 pieces the fused q / k / v projection's epilogue produces and the distance embeddings as the fp16 pieces finalize()
 * prepares per layer (dist_max_abs = max |dist_emb80|: their power-of-two scale), both into kv_workspace (4 * ceil256(B * T) * heads * 64 * 2 + 24576
 * bytes), then w8 = 1 runs csrc/attention_f16x2_w8.hip (8-wave workgroups, 64-key tiles, LDS-DMA staging), w8 = 0 its round-3 twin
 * (csrc/attention_bf16x3.hip <SchemeF16x2, KVP>), w8 = -1 the default. status_dev nullable (bit 1 = fp16 range overflow; {flag, census} pair). */
int at_op_relpos_attention_kvp(const float* qkv, const float* attn_mask, const float* dist_emb80, float dist_max_abs, float* ctx, int B, int T, int heads, int w8,
                               void* kv_workspace, size_t kv_workspace_bytes, int32_t* status_dev, at_stream_t stream);

/* Conformer conv middle (HF modeling_wav2vec2_bert.py:212-222): causal depthwise k31 -> LayerNorm -> swish;
 * g [B*T][1024], w [31][1024]. */
int at_op_dwconv_ln_swish(const float* g, const float* w31x1024, const float* gamma, const float* beta, float* out, int B, int T,
                          at_stream_t stream);
/* the same op on the streaming kernel (csrc/dwconv_stream.hip); bit-identical to at_op_dwconv_ln_swish */
int at_op_dwconv_stream(const float* g, const float* w31x1024, const float* gamma, const float* beta, float* out, int B, int T,
                        at_stream_t stream);

/* VQ assign from precomputed dots [rows][C]: argmax_n -sqrt(max(|x|^2 + e2[n] - 2 dots, 0)), first index. */
int at_op_vq_argmax(const float* x, const float* dots, const float* e2, int16_t* out, int64_t rows, int D, int C, at_stream_t stream);
/* The same with the code rows given (codebook [C][D] fp32, round 5): codes whose approximate squared distance lies within (|x|^2 + e2[best]) 2^-17 of the
 * best are re-evaluated exactly — sum_k (x_k - e_k)^2 in float64 — and the smallest exact distance wins, ties to the lower index. What the two semantic
 * tokenizers run (option "vq_refine"); replaces the nearest-code step of vector_quantize_pytorch / torch.cdist + argmin (reference audiotoken/encoder.py:
 * 100-101,180-181), whose expanded fp32 form cancels when the centres sit in the data. */
int at_op_vq_argmax_refined(const float* x, const float* dots, const float* e2, const float* codebook, int16_t* out, int64_t rows, int D, int C, at_stream_t stream);

/* ---- k-means: fitting the semantic tokenizers' code books (csrc/kmeans.hip) ------------------------------------------------------------------------
 * Replaces the reference's code-book fitting (scripts/clustering/cluster_tokens.py, KMeansClusterConfig audiotoken/configs.py:221-226) with full-batch
 * Lloyd iterations on a device-resident sample X [N][D] fp32 (row-major, kept by pointer) and centres C [K][D] fp32. D % 64 == 0, 64 <= D <= 1024;
 * 4 <= K <= 32767, K % 4 == 0 (int16 labels); K <= N < 2^31. Calls are stream-ordered and never synchronise; all scratch is allocated by create(). */
typedef struct at_kmeans at_kmeans_t;

/* Device bytes at_kmeans_create allocates for this shape (0 when the shape is invalid): size a sample against free memory with it. */
size_t at_kmeans_device_bytes(int64_t N, int D, int K);
/* Create a handle on `device` for N rows of D floats and K centres; NULL on failure (at_last_error). */
at_kmeans_t* at_kmeans_create(int device, int64_t N, int D, int K);
void at_kmeans_destroy(at_kmeans_t* h);
/* "scheme": the E-step's score GEMM operands, 1 = two fp16 pieces (default: the rows are split once per at_kmeans_set_data), 0 = three bf16 pieces (any
 * magnitude; the rows are split chunk by chunk in every E-step) — the fall-back after a range overflow; call at_kmeans_set_data again after changing it. */
int at_kmeans_set_option(at_kmeans_t* h, const char* name, int value);
/* "scheme", "chunk_rows" (rows per E-step chunk), "trials" (k-means++ local trials, 2 + int(ln K)); -1 = unknown name. */
int at_kmeans_get_option(const at_kmeans_t* h, const char* name);
/* Hand the rows to the handle: X device [N][D], 16-byte aligned, must stay valid and unchanged while the handle uses it. x_max_abs = max |X| sets the
 * activation scale of the fp16 scheme (<= 32, LayerNorm-ed rows: the tokenizers' scale 16; else the power of two that puts max |X| into [2^14, 2^15)). */
int at_kmeans_set_data(at_kmeans_t* h, const float* X, float x_max_abs, at_stream_t stream);
/* Greedy k-means++ seeding (sklearn's _kmeans_plusplus, n_local_trials = trials = 2 + int(ln K)): uniforms device float64 [K][trials] in [0, 1);
 * the first centre is row floor(uniforms[0][0] N); every later centre c draws candidate rows by searching uniforms[c][t] * total in the float64 inclusive
 * scan of the current closest squared distances and keeps the candidate of the smallest potential sum_i min(d2_i, |x_i - x_cand|^2) (ties to the first
 * trial, as sklearn). Writes C_out device [K][D] and picked_rows device int64 [K]. */
int at_kmeans_plusplus(at_kmeans_t* h, const double* uniforms, int trials, float* C_out, int64_t* picked_rows, at_stream_t stream);
/* E-step: labels device int16 [N] = the nearest centre of every row (the tokenizers' score GEMM + at_op_vq_argmax_refined: exact float64 re-evaluation of
 * near-ties, ties to the lower index). c_max_abs = max |C| sets the centre scale (<= 0: max |X|, a bound for any mean of rows). status_dev (nullable
 * device word, overwritten): bit 1 = the fp16 range was exceeded (repeat with option "scheme" 0), bit 2 = a row or centre holds a NaN / infinity. */
int at_kmeans_assign(at_kmeans_t* h, const float* C, float c_max_abs, int16_t* labels, int32_t* status_dev, at_stream_t stream);
/* M-step, bitwise reproducible (no float atomics): per-cluster float64 sums of the rows in a stable inverted-index order, the empty clusters relocated
 * (sklearn's rule: the rows farthest from their centre, ties to the lower row, in decreasing distance to the empty clusters in increasing index order),
 * C_new = sum / count rounded to fp32 once. counts device int32 [K] (after relocation); prev_labels nullable (then n_changed = 0); C_new must not alias
 * C_old. stats_dev device float64 [6]: inertia = sum of |x - C_old[label]|^2, shift2 = sum |C_new - C_old|^2, n_changed, n_empty, max |C_new|, and the
 * number of labels outside [0, K) (ignored rows). */
int at_kmeans_update(at_kmeans_t* h, const int16_t* labels, const int16_t* prev_labels, const float* C_old, float* C_new, int32_t* counts,
                     double* stats_dev, at_stream_t stream);
/* The non-affine LayerNorm (eps 1e-5) of a tokenizer's quantiser step on rows x [rows][D] -> y, bit for bit the kernel that step runs: split_kernel 1 =
 * semantic_m's (fp32 rows written with the operand pieces; D 1024; workspace >= round_up(rows, 8) * D * 4 bytes), 0 = semantic_s's plain kernel. */
int at_kmeans_layernorm(const float* x, float* y, int64_t rows, int D, int split_kernel, void* workspace, size_t workspace_bytes, at_stream_t stream);
/* The last update's per-row squared distances to the old centres (device float64 [N]) and its relocations (device int32 [K][3] = row, old cluster,
 * new cluster; the first n_empty entries are valid): for tests. */
int at_kmeans_row_d2(const at_kmeans_t* h, double* out, at_stream_t stream);
int at_kmeans_relocations(const at_kmeans_t* h, int32_t* out, at_stream_t stream);

/* ---- semantic-to-acoustic generation: a KV-cached GPT decoder (csrc/gpt.hip) -------------------------------------------------
 * The model of the reference's semantic decoders' first stage: token embedding wte [V][768] tied to the head, learned positions wpe [block][768],
 * n_layer pre-LN blocks (LayerNorm with a gain only, eps 1e-5; every linear without bias; 12 heads of 64; causal attention scaled by 1/8; MLP
 * 768 -> 3072 -> 768 with the erf GELU), a final LayerNorm, logits = ln_f(x) . wte^T. Tensors carry the checkpoint's names ("transformer.wte.weight",
 * "transformer.h.<i>.attn.c_attn.weight", ...; at_required_tensors("gpt", n_layer, ...)). finalize takes n_layer (1 to 48), V (a multiple of 64, at
 * most 65536) and block (a multiple of 64, at most 1024) from the shapes and refuses anything else, a ".bias" tensor included. */
typedef struct at_gpt at_gpt_t;
at_gpt_t* at_gpt_create(int device_id);
int at_gpt_set_tensor(at_gpt_t* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int at_gpt_finalize(at_gpt_t* h);
void at_gpt_destroy(at_gpt_t* h);
int at_gpt_num_layers(const at_gpt_t* h);
int at_gpt_vocab(const at_gpt_t* h);
int at_gpt_block_size(const at_gpt_t* h);
/* Bytes of the caller-owned device state of one at_gpt_generate call with B rows (1 to 64) whose sequences reach at most max_len tokens
 * (prompt + new, at most the block size): the K / V cache, the activations of the prefill and the rows' bookkeeping. 0 = error. */
size_t at_gpt_state_bytes(const at_gpt_t* h, int B, int max_len);
#define AT_GPT_FINISH_STOP 1
#define AT_GPT_FINISH_MAX_NEW 2
#define AT_GPT_FINISH_BLOCK 3
/* Generate up to max_new tokens for B rows in one stream-ordered call that allocates nothing. prompts_dev: device int32 [B][prompt_stride], row b
 * holding prompt_len[b] ids (prompt_len is a HOST array; 1 <= prompt_len[b] <= prompt_stride). uniforms_dev: device float32 [B][max_new], the draw of
 * row b at step s. Per step and row: logits of the last token, then the sampling rule of at_op_topk_sample (below) with `allow` = NULL or a HOST array
 * int32 [2][4]: step s may only produce ids in [a[s%2][0], a[s%2][1]) or [a[s%2][2], a[s%2][3]). A row finishes when it samples stop_token (not
 * written; negative = none): finish AT_GPT_FINISH_STOP; after max_new tokens: _MAX_NEW; when prompt + new reaches the model's block size: _BLOCK
 * (the reference crops the context instead). A finished row writes nothing more. out_ids_dev device int32 [B][max_new] (entries past
 * out_len_dev[b] are left as they were), out_len_dev / finish_dev device int32 [B]; logits_out_dev NULL or device float32 [B][max_new][V]: the logits each
 * written token was sampled from (and those of a sampled stop token). state_dev: at_gpt_state_bytes(h, B, max_len) bytes with
 * max_len >= min(block, longest prompt + max_new). The steps are enqueued without waiting for the device; every 16 steps the host reads the rows' finish
 * flags and stops when all rows are done, so the call returns with work still in flight on `stream`. status_dev NULL or a device word: bit 0 = a prompt
 * id outside [0, V) was clamped. Every argument is checked before the device is touched. Not re-entrant per handle. */
int at_gpt_generate(at_gpt_t* h, const int32_t* prompts_dev, int prompt_stride, const int32_t* prompt_len, int B, int max_new, float temperature, int top_k,
                    int stop_token, const float* uniforms_dev, const int32_t* allow, int32_t* out_ids_dev, int32_t* out_len_dev, int32_t* finish_dev,
                    float* logits_out_dev, void* state_dev, size_t state_bytes, int max_len, at_stream_t stream, int32_t* status_dev);
/* The long form: sources longer than one prompt, generated window by window with the row's own output carried over, every window of
 * every row enqueued by one call and nothing copied to the host in between. Windows of a source of N ids (1 to 65536) at window S and hop H (both even,
 * 2 <= H <= S, S + 1 + r S <= block): n = 1 if N <= S, else ceil((N - S) / H) + 1 (at_gpt_long_num_windows; 0 = error). Window k reads source ids
 * [k H, k H + min(S, N - k H)); its prompt is those ids + semantic_offset, infer_token, then the row's stream positions [r k H, r k H + carry) with carry = 0
 * for k = 0 and r (S - H) after. A non-final window produces exactly r S - carry ids, step s from [acoustic_offset + (s % 2) codebook_size, ... +
 * codebook_size), and cannot stop. The final window also allows stop_token (negative = none) on even steps, has min(max_new, block - prompt) steps and
 * sets finish_dev[b] as at_gpt_generate does. Pass k of the call runs window k of every row that has one as one batch: one launch that writes the prompts,
 * the prefill, then the steps. The id, the draw and the logits of a step live at the row's STREAM position: out_ids_dev int32 [B][out_stride],
 * uniforms_dev float32 [B][u_stride], logits_out_dev NULL or float32 [B][out_stride][V]; both strides >= the final window's first position + its
 * steps, for every row. src_dev: device int32 [B][src_stride] raw semantic ids, src_len a HOST array. out_len_dev[b] = ids of the row's stream.
 * state_dev: at_gpt_long_state_bytes(h, B, max_len) bytes, max_len >= the longest window's prompt + steps (S + 1 + r S covers every non-final one) and
 * <= block. status_dev bit 0 = a source id outside [0, semantic_vocab) was clamped. For N <= S the result is at_gpt_generate's on the same prompt with
 * the same rules. Every argument and the whole schedule are checked before the device is touched. Not re-entrant per handle. */
int at_gpt_long_num_windows(int N, int S, int H);
size_t at_gpt_long_state_bytes(const at_gpt_t* h, int B, int max_len);
int at_gpt_generate_long(at_gpt_t* h, const int32_t* src_dev, int src_stride, const int32_t* src_len, int B, int S, int H, int r, int semantic_offset,
                         int semantic_vocab, int infer_token, int acoustic_offset, int codebook_size, int stop_token, int max_new, float temperature, int top_k,
                         const float* uniforms_dev, int u_stride, int32_t* out_ids_dev, int out_stride, int32_t* out_len_dev, int32_t* finish_dev,
                         float* logits_out_dev, void* state_dev, size_t state_bytes, int max_len, at_stream_t stream, int32_t* status_dev);
/* The generation queue: n_src sources (1 to 4096) through `slots` cache rows (1 to 64). Every source follows at_gpt_generate_long's
 * schedule unchanged (the same windows, carry, allow sets and finish rules, one draw per stream position); only when a window runs changes, and a slot
 * that finishes a source takes the next waiting one, in the caller's order. All arrays are indexed by SOURCE: src_dev [n_src][src_stride], src_len HOST
 * [n_src], uniforms_dev [n_src][u_stride], out_ids_dev [n_src][out_stride], out_len_dev / finish_dev [n_src], logits_out_dev NULL or
 * [n_src][out_stride][V]; the draw of stream position p of source i is uniforms[i][p] whatever slot and tick it ran in. A tick is one model pass over one
 * token list and one sampler launch: one step token of every slot that is mid-window, then the whole prompt of every window admitted this tick, in slot
 * order while the list stays within tick_tokens (slots + max_len <= tick_tokens <= 65600, so one window always fits; a window that does not fit waits).
 * A list of more than 64 tokens takes the GEMM route, a shorter one the streaming linear kernel, as a pass of at_gpt_generate does. The host reads the
 * slots' flags every 16 ticks while some slot is in a final window, and nothing else. state_dev: at_gpt_queue_state_bytes(h, slots, max_len, tick_tokens)
 * bytes (K / V for slots rows of max_len positions, activations for tick_tokens tokens, nothing per source); max_len as for at_gpt_generate_long.
 * trace NULL or HOST int32 [trace_cap][4], one row per tick: step tokens, windows started, prefill tokens, route (1 = GEMM); n_ticks NULL or HOST: the
 * ticks run (a trace too small loses its tail, the run goes on). placement NULL or HOST int32 [n_src][3]: slot, first tick, last tick of each source.
 * With slots = 1 every tick is a lone prefill or a lone step, and the result is, id for id and logit for logit, the chain of one-row
 * at_gpt_generate_long calls. Every argument and the schedule's extent are checked before the device is touched. Not re-entrant per handle. */
size_t at_gpt_queue_state_bytes(const at_gpt_t* h, int slots, int max_len, int tick_tokens);
int at_gpt_generate_queue(at_gpt_t* h, const int32_t* src_dev, int src_stride, const int32_t* src_len, int n_src, int S, int H, int r, int semantic_offset,
                          int semantic_vocab, int infer_token, int acoustic_offset, int codebook_size, int stop_token, int max_new, float temperature, int top_k,
                          const float* uniforms_dev, int u_stride, int32_t* out_ids_dev, int out_stride, int32_t* out_len_dev, int32_t* finish_dev,
                          float* logits_out_dev, void* state_dev, size_t state_bytes, int max_len, int slots, int tick_tokens, int32_t* trace, int trace_cap,
                          int32_t* n_ticks, int32_t* placement, at_stream_t stream, int32_t* status_dev);
/* Voice prompts: the prompted forms of the two calls above. A source with a prompt of P semantic ids and their r P coarse ids follows the
 * same schedule on the concatenated source, prompt ids then source ids. Stream positions [0, r P) are given: position p is
 * codes[p & 1][p >> 1] + acoustic_offset + (p & 1) codebook_size. Window 0 carries those r P ids instead of none and, unless final, produces r S - r P ids.
 * The carry of a later window comes from the prompt below stream position r P and from the row's output above it. The result excludes the prompt:
 * out_ids_dev, out_len_dev, uniforms_dev and logits_out_dev are indexed by result position q = stream position - r P, and the strides count result ids.
 * The table: prompt_sem_dev device int32 [n_prompts][p_stride], prompt_codes_dev device int32 [n_prompts][2][f_stride], prompt_len HOST int32 [n_prompts]
 * (even, 2 <= P <= S - H, P <= p_stride, r P / 2 <= f_stride), prompt_of_src HOST int32 per source: its entry or -1 for none; n_prompts 0 to 4096. A source's
 * P + N must not exceed 65536. One entry serves any number of sources. A prompt id outside [0, semantic_vocab) is clamped like a source id (status bit 0);
 * a code outside [0, codebook_size) is clamped and sets status bit 1. The state sizes do not depend on the prompt: at_gpt_long_state_bytes and
 * at_gpt_queue_state_bytes serve, with max_len for the windows of the concatenated sources. A call whose sources all have -1 is the prompt-free call, bit
 * for bit. at_gpt_long_num_windows_prompted: the windows of a source of N ids after a prompt of P (0 = error). */
int at_gpt_long_num_windows_prompted(int P, int N, int S, int H);
int at_gpt_generate_long_prompted(at_gpt_t* h, const int32_t* src_dev, int src_stride, const int32_t* src_len, int B, const int32_t* prompt_sem_dev, int p_stride,
                                  const int32_t* prompt_codes_dev, int f_stride, const int32_t* prompt_len, int n_prompts, const int32_t* prompt_of_src, int S, int H,
                                  int r, int semantic_offset, int semantic_vocab, int infer_token, int acoustic_offset, int codebook_size, int stop_token, int max_new,
                                  float temperature, int top_k, const float* uniforms_dev, int u_stride, int32_t* out_ids_dev, int out_stride, int32_t* out_len_dev,
                                  int32_t* finish_dev, float* logits_out_dev, void* state_dev, size_t state_bytes, int max_len, at_stream_t stream, int32_t* status_dev);
int at_gpt_generate_queue_prompted(at_gpt_t* h, const int32_t* src_dev, int src_stride, const int32_t* src_len, int n_src, const int32_t* prompt_sem_dev, int p_stride,
                                   const int32_t* prompt_codes_dev, int f_stride, const int32_t* prompt_len, int n_prompts, const int32_t* prompt_of_src, int S, int H,
                                   int r, int semantic_offset, int semantic_vocab, int infer_token, int acoustic_offset, int codebook_size, int stop_token, int max_new,
                                   float temperature, int top_k, const float* uniforms_dev, int u_stride, int32_t* out_ids_dev, int out_stride, int32_t* out_len_dev,
                                   int32_t* finish_dev, float* logits_out_dev, void* state_dev, size_t state_bytes, int max_len, int slots, int tick_tokens,
                                   int32_t* trace, int trace_cap, int32_t* n_ticks, int32_t* placement, at_stream_t stream, int32_t* status_dev);
/* The sampling step alone, one workgroup per row, no float atomics (the same call twice gives the same ids). logits_dev device float32 [B][V], V <= 65536;
 * uniforms_dev device float32 [B]; allow NULL or a HOST array int32 [4] = two half-open id ranges; out_dev device int32 [B]. The rule:
 * 1. zt_i = z_i / temperature (one IEEE fp32 division). 2. ids outside the allow ranges become -inf. 3. v = the min(top_k, V)-th largest zt; every id
 * with zt_i >= v is kept (ties at the threshold stay). 4. m = max kept zt, p_i = exp(zt_i - m), S = sum p_i. 5. the token is the lowest kept id whose
 * running sum in ascending id order exceeds u * S; if rounding leaves none, the highest kept id whose zt is not -inf. */
int at_op_topk_sample(const float* logits_dev, int B, int V, float temperature, int top_k, const float* uniforms_dev, const int32_t* allow, int32_t* out_dev,
                      at_stream_t stream);
/* Truncation after the top-k. K = the ids step 3 keeps, p and m as in step 4, S_K = the sum of p over K.
 * 3a. min_p in (0, 1): lmin = float32(log(min_p)), the logarithm in double, rounded once; an id stays iff (zt_i - m) >= lmin, one fp32 subtraction. Exact.
 * 3b. top_p in (0, 1): G(x) = the sum of p over the ids of K with zt > x; an id stays iff G(zt_i) < top_p * S_K: the mass strictly above it is below
 *     top_p (Hugging Face's TopPLogitsWarper, applied to the top-k set). Equal values stay or go together, the maximum always stays. The device adds
 *     floor(p_i * 2^40) as 64-bit integers (the order of additions does not matter) and compares with ceil(top_p * that total): the kept set is the rule's
 *     wherever no |G(x) / S_K - top_p| is below 2^-21 + 2^-22.
 * Both are evaluated on K and intersected; with v_min and v_p the lowest values that stay, steps 4 and 5 run on zt_i >= max(v, v_min, v_p).
 * top_p = 1 and min_p = 0 are off; NaN, top_p outside (0, 1] and min_p outside [0, 1) are refused before any device work.
 * at_gpt_set_truncation sets both on the handle (off at creation): at_gpt_generate, at_gpt_generate_long, at_gpt_generate_queue and their prompted forms
 * read them; a refused call leaves the handle unchanged. With both off those calls launch what they launched before and give the same ids, bit for bit.
 * at_op_nucleus_sample is the op alone: at_op_topk_sample's arguments and rule with the two cuts, and kept_out_dev / thresh_out_dev, each NULL or device
 * int32 / float32 [B]: the size of row b's final set and its lowest value. */
int at_gpt_set_truncation(at_gpt_t* h, float top_p, float min_p);
int at_op_nucleus_sample(const float* logits_dev, int B, int V, float temperature, int top_k, float top_p, float min_p, const float* uniforms_dev,
                         const int32_t* allow, int32_t* out_dev, int32_t* kept_out_dev, float* thresh_out_dev, at_stream_t stream);
/* Teacher-forced scoring (csrc/gpt_score.hip): the log-probability and the rank of GIVEN ids under the model, where the calls above draw ids.
 * Row b of seq_dev (device int32 [n_rows][seq_stride], n_rows 1 to 65536) holds seq_len[b] ids of the model's own vocabulary, 2 <= seq_len[b] <= max_len <=
 * block; seq_len and score_from are HOST arrays, 1 <= score_from[b] < seq_len[b]. For every p in [score_from[b], seq_len[b]) the logits at position p - 1
 * (causal, positions from 0) are scored against the target seq[b][p] by the rule of at_op_score_rows (below) with `allow` = NULL or a HOST array int32
 * [2][4], the set of a position being allow[(p - score_from[b]) % 2], and the result goes to logprob_out_dev / rank_out_dev [b][p - score_from[b]] (device
 * float32 / int32 [n_rows][out_stride], out_stride >= every row's seq_len - score_from, n_rows * out_stride < 2^31; entries past a row's count are left as
 * they were). logits_out_dev NULL or device float32 [n_rows][out_stride][V]: the logits each target was scored on. The rows are taken in the caller's order
 * into passes of at most `rows` cache rows (1 to 64) and at most pass_tokens tokens (max_len to 65600, so one row always fits). A row puts its first
 * seq_len - 1 ids into the list: nothing is scored on the logits of its last id, which is a target only. A pass is one prefill of its token list through
 * the model at_gpt_generate runs (a list of more than 64 tokens on the GEMM route, a shorter one on the streaming linear kernel), then the
 * head for the pass's scored positions, head_rows (a multiple of 16, 16 to 4096) at a time: the final LayerNorm, the logits on the fp32 GEMM, the row rule.
 * The logits exist one chunk at a time. state_dev: at_gpt_score_state_bytes(h, rows, max_len, pass_tokens, head_rows) bytes (K / V for rows x max_len
 * positions, activations for pass_tokens tokens, one chunk of logits; nothing per row of the call or per scored position; 0 = error). Everything is
 * enqueued on `stream`; the host waits for nothing and nothing is allocated. status_dev NULL or a device word: bit 0 = an id outside [0, V) was clamped.
 * Every argument is checked before the device is touched. Not re-entrant per handle. */
size_t at_gpt_score_state_bytes(const at_gpt_t* h, int rows, int max_len, int pass_tokens, int head_rows);
int at_gpt_score(at_gpt_t* h, const int32_t* seq_dev, int seq_stride, const int32_t* seq_len, const int32_t* score_from, int n_rows, float temperature,
                 const int32_t* allow, float* logprob_out_dev, int32_t* rank_out_dev, int out_stride, float* logits_out_dev, void* state_dev, size_t state_bytes,
                 int rows, int max_len, int pass_tokens, int head_rows, at_stream_t stream, int32_t* status_dev);
/* The scoring rule alone, one workgroup per row, no float atomics (the same call twice gives the same bits). logits_dev device float32 [R][V], R 1 to 65536,
 * 1 <= V <= 65536; targets_dev device int32 [R]; allow NULL or a HOST array int32 [4] = two half-open id ranges; logprob_out_dev device float32 [R],
 * rank_out_dev device int32 [R]. The rule, for a row z with target t: 1. zt_i = z_i / temperature (one IEEE fp32 division; exact at 1). 2. ids outside the
 * allow ranges become -inf. 3. m = max zt, S = sum exp(zt_i - m) in one fixed order of additions, logprob = (zt_t - m) - log(S).
 * 4. rank = the number of ids with zt_i > zt_t (ties not counted): at_op_topk_sample's top_k = k keeps the target exactly when rank < k. A target that is
 * not allowed, or outside [0, V), gets logprob = -inf and rank = V. */
int at_op_score_rows(const float* logits_dev, int R, int V, const int32_t* targets_dev, float temperature, const int32_t* allow, float* logprob_out_dev,
                     int32_t* rank_out_dev, at_stream_t stream);

/* ---- the fine stage: coarse code books -> all eight (csrc/fine.hip) -----------------------------------------------------------
 * bark's non-causal fine transformer: 8 embedding tables wtes[i] [1056][E] and learned positions wpe [W][E]; n_layer pre-LN blocks (LayerNorm with gain
 * and bias, eps 1e-5; E / 64 heads of 64; attention over the whole window without a mask, scaled by 1/8; MLP E -> 4E -> E with the erf GELU; the four
 * linears of every block with a bias or all without); a final LayerNorm; 7 heads lm_heads[j] [1056][E], lm_heads[j] predicting code book j + 1. Tensors
 * carry bark's names ("transformer.wtes.<i>.weight", "transformer.h.<l>.attn.c_attn.weight", "lm_heads.<j>.weight", ...; at_required_tensors("fine",
 * n_layer, with_bias, ...) lists them at E = 1024, W = 1024). finalize takes E (768 or 1024), W (a multiple of 128, 128 to 1024) and n_layer (1 to 48)
 * from the shapes and refuses anything else. */
typedef struct at_fine at_fine_t;
at_fine_t* at_fine_create(int device_id);
int at_fine_set_tensor(at_fine_t* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int at_fine_finalize(at_fine_t* h);
void at_fine_destroy(at_fine_t* h);
int at_fine_num_layers(const at_fine_t* h);
int at_fine_hidden(const at_fine_t* h);
int at_fine_block_size(const at_fine_t* h);
int at_fine_has_bias(const at_fine_t* h);
/* Windows of a row of T frames (1 to 262144): max(0, ceil((T - W) / (W / 2))) + 1. 0 = error. */
int at_fine_num_windows(const at_fine_t* h, int T);
/* Bytes of the caller-owned device state of one at_fine_generate call with B rows (1 to 64) of at most max_T frames: the rows' work arrays
 * [max(max_T, W)][8] and the activations of B windows. 0 = error. */
size_t at_fine_state_bytes(const at_fine_t* h, int B, int max_T);
/* Fill code books 2 to 7 of B rows in one stream-ordered call that allocates nothing and never waits for the device. coarse_dev: device int32
 * [B][2][t_stride], row b holding lens[b] frames (lens is a HOST array; 1 <= lens[b] <= min(t_stride, max_T)). A row's work array is [L][8] with
 * L = max(T, W), every cell 1024 but the coarse codes; window k of its n windows covers positions [start, start + W) with start = min(k W/2, L - W) and
 * predicts buffer positions >= rel = min(k W/2, L - W/2) - start: for c = 2..7 the model runs on the window's current contents and one id per predicted
 * position is written into channel c, padding positions included. Pass k of the call runs window k of every row that has one as one batch.
 * greedy = 1: the id is the argmax of the logits [0, 1024), the lowest id among equals (temperature and uniforms_dev are not read). greedy = 0: with
 * u = uniforms_dev[b][k][c - 2][t] (device float32 [B][n_max][6][W], n_max >= the windows of the longest row): zt_i = z_i / temperature (one IEEE fp32
 * division), m = max zt, p_i = expf(zt_i - m), S = sum p_i; the id is the lowest whose running sum in ascending id order exceeds u * S; if rounding
 * leaves none, the highest id with p_i > 0. out_dev: device int32 [B][8][t_stride]; entries at t >= lens[b] are left as they were. logits_out_dev NULL
 * or device float32 [B][n_max][6][W][1024], window_ids_dev NULL or device int32 [B][n_max][6][W]: the logits every written id was drawn from and the id;
 * entries of positions < rel and of windows a row does not have are left as they were. status_dev NULL or a device word: bit 0 = a coarse code outside
 * [0, 1024) was clamped. Every argument is checked before the device is touched. Not re-entrant per handle. */
int at_fine_generate(at_fine_t* h, const int32_t* coarse_dev, int t_stride, const int32_t* lens, int B, float temperature, int greedy,
                     const float* uniforms_dev, int n_max, int32_t* out_dev, float* logits_out_dev, int32_t* window_ids_dev, void* state_dev, size_t state_bytes,
                     int max_T, at_stream_t stream, int32_t* status_dev);
/* Bytes of the caller-owned device state of one at_fine_generate_queue call: `slots` (1 to 64) work arrays [max(max_T, W)][8] and the activations of
 * `slots` windows, nothing per row: what at_fine_state_bytes(h, slots, max_T) gives. 0 = error. */
size_t at_fine_queue_state_bytes(const at_fine_t* h, int slots, int max_T);
/* The fine stage's window queue: n_rows rows (1 to 4096) through `slots` work arrays (1 to 64). Every row follows at_fine_generate's
 * schedule unchanged (the same windows, start, rel, code-book order and write-back); only when a window runs changes. Rows take empty slots in the
 * caller's order; a slot runs its row's windows 0 .. n - 1 in consecutive passes, and a slot whose row has run its last window takes the next waiting
 * row in the next pass. Pass p is the current window of every occupied slot, in slot order, as one batch: windows of different k sit side by side. The
 * schedule follows from the lengths alone; the call is enqueued on `stream`, allocates no device memory and never waits for the device.
 * All arrays are ragged and indexed by ROW, never by slot: lens HOST int32 [n_rows] (1 <= lens[b] <= max_T); with off = the exclusive prefix sum of lens
 * and woff = that of the rows' window counts, row b's coarse codes are device int32 [2][T_b] at coarse_dev + 2 off[b], its result [8][T_b] at
 * out_dev + 8 off[b], and the draw of its window k, code book 2 + j, buffer position t is uniforms_dev[((woff[b] + k) * 6 + j) * W + t] whatever slot
 * and pass it ran in. logits_out_dev NULL or float32 [sum n_b][6][W][1024], window_ids_dev NULL or int32 [sum n_b][6][W], by the same window cell;
 * entries of positions < rel are left as they were. A row's work array is written when it enters its slot (all max(T_b, W) cells, so nothing of the
 * slot's previous row can be read) and copied out when it leaves. trace NULL or HOST int32 [trace_cap][3], one row per pass: windows, rows admitted,
 * rows retired; n_passes NULL or HOST: the passes run (a trace too small loses its tail, the run goes on). placement NULL or HOST int32 [n_rows][3]:
 * slot, first pass, last pass of each row. greedy, temperature, the sampling rule and status_dev as at_fine_generate. state_dev:
 * at_fine_queue_state_bytes(h, slots, max_T) bytes. With slots = 1 every pass is one window and a row's launches are those of at_fine_generate on the
 * row alone. Every argument and the state's size are checked before the device is touched. Not re-entrant per handle. */
int at_fine_generate_queue(at_fine_t* h, const int32_t* coarse_dev, const int32_t* lens, int n_rows, float temperature, int greedy, const float* uniforms_dev,
                           int32_t* out_dev, float* logits_out_dev, int32_t* window_ids_dev, void* state_dev, size_t state_bytes, int max_T, int slots,
                           int32_t* trace, int trace_cap, int32_t* n_passes, int32_t* placement, at_stream_t stream, int32_t* status_dev);
/* ---- the fine stage with a history prompt: BarkFineModel.generate with history_prompt["fine_prompt"] ---------------------------
 * A row of T frames may continue a history of Th frames of all 8 code books. With H = W / 2 and h = min(H, Th), the row's work array is [L][8] with
 * L = max(h + T, W): cells [0, h) hold the LAST h history frames in every channel, cells [h, h + T) the coarse codes, 1024 everywhere else. The row has
 * n = max(0, ceil((T - (W - h)) / H)) + 1 windows; window k has start = min(k H, L - W), fill = min(h + k H, L - H) and rel = fill - start, which is
 * positive in every window of a row with a history. History cells are never written; the result is cells [h, h + T). h = 0 is the rule above, unchanged,
 * and the entry points above are these with an empty table, bit for bit.
 * The history table: hist_dev device int32 [n_hist][8][h_stride]; hist_lens HOST int32 [n_hist], 1 <= hist_lens[i] <= min(h_stride, max_hist);
 * hist_of_row HOST int32 [B or n_rows], the entry each row continues or -1 for none, so one entry serves any number of rows. n_hist = 0 (0 to 4096): no
 * table; the three pointers are not read, except that a non-null hist_of_row must then hold -1 everywhere. max_hist (0 to 262144) sizes the state:
 * work arrays of max(min(H, max_hist) + max_T, W) cells. A history id outside [0, 1024) is clamped and sets bit 1 of *status_dev.
 * uniforms, logits_out and window_ids keep their layouts: per window cell and buffer position, positions below rel left as they were; n_max and the
 * queue's window offsets count a row's windows by at_fine_num_windows_hist(h, T, Th). */
int at_fine_num_windows_hist(const at_fine_t* h, int T, int Th);
size_t at_fine_state_bytes_hist(const at_fine_t* h, int B, int max_T, int max_hist);
size_t at_fine_queue_state_bytes_hist(const at_fine_t* h, int slots, int max_T, int max_hist);
int at_fine_generate_hist(at_fine_t* h, const int32_t* coarse_dev, int t_stride, const int32_t* lens, int B, const int32_t* hist_dev, int h_stride,
                          const int32_t* hist_lens, int n_hist, const int32_t* hist_of_row, int max_hist, float temperature, int greedy,
                          const float* uniforms_dev, int n_max, int32_t* out_dev, float* logits_out_dev, int32_t* window_ids_dev, void* state_dev,
                          size_t state_bytes, int max_T, at_stream_t stream, int32_t* status_dev);
int at_fine_generate_queue_hist(at_fine_t* h, const int32_t* coarse_dev, const int32_t* lens, int n_rows, const int32_t* hist_dev, int h_stride,
                                const int32_t* hist_lens, int n_hist, const int32_t* hist_of_row, int max_hist, float temperature, int greedy,
                                const float* uniforms_dev, int32_t* out_dev, float* logits_out_dev, int32_t* window_ids_dev, void* state_dev, size_t state_bytes,
                                int max_T, int slots, int32_t* trace, int trace_cap, int32_t* n_passes, int32_t* placement, at_stream_t stream,
                                int32_t* status_dev);

/* ---- the semantic-to-audio stream: one source, pushed as its ids arrive -------------------------------------------------------
 * Both stages run the windows of the calls above as soon as their inputs exist; ids, logits and codes are those of at_gpt_generate_long and
 * at_fine_generate on the whole source at one row. The device state of each stage is caller-owned and its size does not depend on the stream's
 * length. `pos` is the stream's HOST record, int64 [2] = {items pushed so far, 1 after the final call}, zeroed by the caller to start a stream and
 * updated by a call that succeeds. Every argument, the geometry, the state's size, a push after the final call and a final call with nothing pushed
 * are refused before the device is touched. All launches go on `stream`; neither call is re-entrant per handle.
 *
 * at_gpt_stream_push: n_new (>= 0) source ids, device int32. Window k of at_gpt_generate_long's schedule runs as a NON-final window as soon as
 * more than k H + S ids exist; final = 1 runs the one remaining window as the final one (STOP on even steps, budget min(max_new, block - prompt)).
 * The state (at_gpt_stream_state_bytes: the K / V cache and activations of one row, 2 S source ids, the last r (S - H) stream ids) keeps the ids no
 * window has left behind yet; a long push is absorbed 2 S ids at a time. out_ids_dev: device int32 [out_cap], this call's piece of the stream: with k0
 * windows run before the call it starts at stream position r k0 H, so for k0 > 0 its first r (S - H) entries are the carry and the ids this call
 * produced follow; for k0 = 0 they start at entry 0. out_cap must hold them (the final window: its budget). The draw of stream position p is
 * uniforms_dev[p - u_pos0]; the call refuses when a window it will run needs a position outside [u_pos0, u_pos0 + u_len). out_len_dev / finish_dev: one
 * device word each, as row 0 of at_gpt_generate_long has them (the length counts the whole stream). windows_run: NULL or HOST, the windows this call
 * ran. The host looks at the device only while the final window runs (its flag, every 16 steps). at_gpt_set_truncation applies. */
size_t at_gpt_stream_state_bytes(const at_gpt_t* h, int S, int H, int r);
int at_gpt_stream_push(at_gpt_t* h, void* state_dev, size_t state_bytes, int64_t* pos, const int32_t* ids_dev, int n_new, int final, int S, int H, int r,
                       int semantic_offset, int semantic_vocab, int infer_token, int acoustic_offset, int codebook_size, int stop_token, int max_new,
                       float temperature, int top_k, const float* uniforms_dev, int64_t u_pos0, int64_t u_len, int32_t* out_ids_dev, int out_cap,
                       int32_t* out_len_dev, int32_t* finish_dev, int32_t* windows_run, at_stream_t stream, int32_t* status_dev);
/* at_fine_stream_push: n_frames (>= 0) new coarse frames as the GPT wrote them: ids_dev device int32 [2 n_frames], interleaved, code book 0 carrying
 * acoustic_offset and code book 1 acoustic_offset + codebook_size (8-byte aligned). The state (at_fine_stream_state_bytes) holds a window onto the
 * row's work array: 2 W cells, from the start of the last window run on; a long push is absorbed as far as that leaves room. Window j of
 * at_fine_generate's schedule runs at start = j W/2 as soon as j W/2 + W frames exist; final = 1 (T = the frames pushed in all) runs the padded single
 * window when T < W, or the last window at start = T - W with rel > 0 when the windows run do not cover T. After non-last window j frames
 * [j W/2, (j + 1) W/2) are final, after the last window everything up to T: they are written to emit_dev, device int64 [8][emit_stride], in order from
 * column 0 (what AcousticDecodeStream.push takes); n_emitted (HOST, not NULL) is their count, and emit_stride must hold it. The draw of window j, code
 * book 2 + c, buffer position t is uniforms_dev[((j - u_win0) * 6 + c) * W + t]; a window outside [u_win0, u_win0 + u_windows) is refused. An id
 * outside its code book sets bit 2 of *status_dev and its frame is left as it was. greedy / temperature as at_fine_generate. */
size_t at_fine_stream_state_bytes(const at_fine_t* h);
int at_fine_stream_push(at_fine_t* h, void* state_dev, size_t state_bytes, int64_t* pos, const int32_t* ids_dev, int n_frames, int final, int acoustic_offset,
                        int codebook_size, float temperature, int greedy, const float* uniforms_dev, int u_win0, int u_windows, int64_t* emit_dev,
                        int emit_stride, int32_t* n_emitted, int32_t* windows_run, at_stream_t stream, int32_t* status_dev);
/* The hand-over kernel alone: frames 0 .. n_frames - 1 of ids_dev (as above) into channels 0 and 1 of work_dev (device int32 [n_frames + n_pad][8]),
 * 1024 into channels 2 to 7; cells [n_frames, n_frames + n_pad) get 1024 in all 8. Status bit 2 as above. */
int at_op_fine_handover(const int32_t* ids_dev, int n_frames, int n_pad, int acoustic_offset, int codebook_size, int32_t* work_dev, at_stream_t stream,
                        int32_t* status_dev);

/* ---- semantic-to-audio stream pools: live streams share the GPT's ticks and the fine stage's passes ------------------------------
 * A pool's device state is caller-owned: the shared part of at_gpt_generate_queue / at_fine_generate_queue (`slots` cache rows and `tick_tokens` token
 * rows; the activations of `fine_slots` windows) and per stream only what outlives a call. `pos` is the pool's HOST record, int64 [streams][2], row
 * `place` = {items pushed so far, 1 after the final call} of the stream in that place; the caller zeroes a row to start a stream there and a call that
 * succeeds updates the rows it names. One call serves n of the streams, named by place[n] (HOST, distinct) and listed in ascending stream id, which is
 * the order in which they take free rows; every other call array is indexed by the call's streams, 0 .. n - 1. A call is checked whole before the
 * device or the record is touched: a refused call leaves every stream as it was. All launches go on `stream`; not re-entrant per handle.
 *
 * at_gpt_pool_push: stream i of the call pushes n_new[i] (HOST, >= 0) ids, ids_dev holding all of them back to back in the call's order, and
 * final[i] = 1 (HOST) runs its remaining window as the final one. Per stream the windows, their rules and the meaning of its piece are
 * at_gpt_stream_push's: out_ids_dev [n][out_stride], row i starting at stream position r k0 H of stream i (its carry first when k0 > 0);
 * uniforms_dev [n][u_stride], the draw of stream position p of stream i being uniforms_dev[i][p - u_pos0[i]] (u_pos0 HOST int64 [n]);
 * out_len_dev / finish_dev device int32 [n] (finish must be zeroed by the caller; out_len counts the whole stream and is written when an id is);
 * logits_out_dev NULL or [n][out_stride][V], indexed as out_ids_dev. The streams' windows share `slots` cache rows by at_gpt_generate_queue's tick
 * (GptPoolSchedule in csrc/gpt.h). The rings hold 2 S ids per stream, so a long push is absorbed in rounds that are global to the call: one copy-in,
 * the round's ticks, one shift. HOST outputs, each nullable: windows_run [n]; trace [trace_cap][5] = a tick's step tokens, windows started, prefill
 * tokens, route (1: the GEMM) and round; n_ticks; n_rounds; placement [n][3] = the cache row of the stream's last chain, its first and last tick (-1:
 * it ran no window). n * out_stride and every u_pos0 must fit 31 bits. max_len must hold max(S + 1 + r S, min(block, S + 1 + r (S - H) + max_new)) positions, tick_tokens at least slots + max_len.
 * The host looks at the device only while some row is in a final window (the rows' flags, every 16 ticks). at_gpt_set_truncation applies. */
size_t at_gpt_pool_state_bytes(const at_gpt_t* h, int streams, int slots, int max_len, int tick_tokens, int S, int H, int r);
int at_gpt_pool_push(at_gpt_t* h, void* state_dev, size_t state_bytes, int streams, int slots, int max_len, int tick_tokens, int64_t* pos, int n,
                     const int32_t* place, const int32_t* ids_dev, const int32_t* n_new, const int32_t* final, int S, int H, int r, int semantic_offset,
                     int semantic_vocab, int infer_token, int acoustic_offset, int codebook_size, int stop_token, int max_new, float temperature, int top_k,
                     const float* uniforms_dev, int u_stride, const int64_t* u_pos0, int32_t* out_ids_dev, int out_stride, int32_t* out_len_dev,
                     int32_t* finish_dev, float* logits_out_dev, int32_t* windows_run, int32_t* trace, int trace_cap, int32_t* n_ticks, int32_t* n_rounds,
                     int32_t* placement, at_stream_t stream, int32_t* status_dev);
/* at_fine_pool_push: stream i of the call hands over n_frames[i] (HOST, >= 0) new coarse frames, the 2 n_frames[i] interleaved ids from
 * ids_dev[id_off[i]] on (id_off HOST int64 [n], even; ids_dev 8-byte aligned; at_gpt_pool_push's out_ids_dev with id_off[i] = i out_stride + the carry is
 * such an array), and final[i] = 1 (HOST) ends it. Per stream the windows, their draws and what turns final are at_fine_stream_push's. The state
 * (at_fine_pool_state_bytes) holds 2 W cells [8] per stream and the activations of fine_slots windows. Per round, for all streams of the call: one
 * hand-over launch (status bit 2 as at_fine_stream_push), the runnable windows in waves (wave w: the w-th runnable window of every stream that has one, in
 * passes of up to fine_slots windows; two windows of one stream never share a pass), one emit launch, one shift launch; a launch takes up to 128 streams.
 * The draw of window j of stream i, code book 2 + c, buffer position t is uniforms_dev[((u_cell0[i] + j - u_win0[i]) * 6 + c) * W + t] (all three HOST
 * int32 [n]); a window outside [u_win0[i], u_win0[i] + u_windows[i]) is refused. emit_dev: device int64 [n][8][emit_stride], stream i's final frames in
 * order from column 0 (n * 8 * emit_stride must fit 31 bits); n_emitted (HOST int32 [n], not NULL) their counts. HOST outputs, nullable: windows_run [n]; trace [trace_cap][3] = a pass's round,
 * wave and windows; n_passes. Nothing is polled: the schedule is known from the counts. */
size_t at_fine_pool_state_bytes(const at_fine_t* h, int streams, int fine_slots);
int at_fine_pool_push(at_fine_t* h, void* state_dev, size_t state_bytes, int streams, int fine_slots, int64_t* pos, int n, const int32_t* place,
                      const int32_t* ids_dev, const int64_t* id_off, const int32_t* n_frames, const int32_t* final, int acoustic_offset, int codebook_size,
                      float temperature, int greedy, const float* uniforms_dev, const int32_t* u_cell0, const int32_t* u_win0, const int32_t* u_windows,
                      int64_t* emit_dev, int emit_stride, int32_t* n_emitted, int32_t* windows_run, int32_t* trace, int trace_cap, int32_t* n_passes,
                      at_stream_t stream, int32_t* status_dev);

#ifdef __cplusplus
}
#endif
#endif /* AUDIOTOKEN_HIP_H */
