/*
 * llmie.h -- C ABI of the MI355X-native Llama-2 decoder hot path.
 *
 * Drop-in boundary for chongchen1999/llm-inference-engine (reference @ 2024_10_08).
 * The reference has no FFI of its own: its boundary is the set of C++ `launch*`
 * templates in src/kernels/includes/ *.cuh plus the layer classes in
 * src/layers/includes/ *.h.  Every entry point below replaces exactly one of those
 * (cited per function, paths relative to the reference root); the C++ templates
 * of the same names shipped in llm-inference-engine_amd/src/ are thin adaptors that
 * unpack TensorWrapper<T> into these calls, so user_entry.cpp / examples/cpp build
 * unchanged on top (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - plain pointers + sizes, no C++/torch types.  All data pointers are DEVICE
 *     pointers (HBM) unless the name ends in _host.
 *   - `dtype` selects the element type of every `void *` tensor of the call:
 *     LLMIE_F32 (float) or LLMIE_F16 (IEEE half); accumulation is always fp32.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  No
 *     entry point allocates, frees or synchronises: all of them are legal inside
 *     hipStreamBeginCapture/EndCapture (hipGraph).
 *   - return value: 0 on success, a negative llmie_status otherwise;
 *     llmie_last_error() returns a thread-local message.  The C++ adaptors turn a
 *     non-zero status into the reference's LLM_CHECK behaviour (std::runtime_error,
 *     src/utils/macro.h:74-94).
 *   - tensors are dense row-major; offsets are computed in 64-bit (the
 *     reference's int32 offsets overflow for the 7B KV cache at batch >= 8).
 */
#ifndef LLMIE_H
#define LLMIE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history (llmie_abi_version() returns the library's; a consumer compares it with the header it was built against):
 *   1  round 1.
 *   2  llmie_linear, llmie_linear_swiglu, llmie_linear_w8a16, llmie_linear_w4a16 gained (workspace, workspace_bytes) in front
 *      of the stream argument and llmie_linear_fp8_workspace_bytes gained N; w8a16 with M > 64 / w4a16 with M > 8 need a
 *      workspace (NULL -> LLMIE_ERR_UNSUPPORTED).  A version-1 consumer would pass its stream where the slab pointer goes.
 *   3  round 3: additions only are listed at the entries they concern (int8 / int4 weight-only prefill, decoder config flags,
 *      per-request sampling: llmie_sampling_params, llmie_sample_logits(_workspace_bytes), llmie_lm_head_sample_params; token scoring:
 *      llmie_score_tokens(_workspace_bytes); the decode attention's launch plan: llmie_decoder_mha_plan; masks, logit bias,
 *      stop sets and top-N log-probabilities in the sampler: llmie_sampling_ext, llmie_sample_logits_ext,
 *      llmie_lm_head_sample_ext; several hypotheses per request: llmie_beam_step(_workspace_bytes),
 *      llmie_kv_pages_fork(_workspace_bytes); speculative decoding: llmie_spec_verify(_workspace_bytes), llmie_ngram_draft,
 *      llmie_spec_verify_sampled(_workspace_bytes); draft trees: llmie_spec_tree_prepare, llmie_spec_verify_tree(_workspace_bytes),
 *      llmie_kv_tree_commit, llmie_ngram_draft_tree, llmie_decoder_set_tree). */
#define LLMIE_ABI_VERSION 3

typedef enum { LLMIE_F32 = 0, LLMIE_F16 = 1 } llmie_dtype;

typedef enum {
    LLMIE_OK = 0,
    LLMIE_ERR_INVALID_ARG = -1,   /* NULL pointer, non-positive size, shape mismatch */
    LLMIE_ERR_UNSUPPORTED = -2,   /* shape/dtype outside what the kernels implement   */
    LLMIE_ERR_LAUNCH = -3,        /* hipGetLastError() != hipSuccess after the launch */
    LLMIE_ERR_WORKSPACE = -4      /* caller-provided workspace too small              */
} llmie_status;

typedef void *llmie_stream; /* hipStream_t */

typedef enum {
    LLMIE_W_F16 = 0,     /* fp16 weights [N,K]                                   */
    LLMIE_W_INT8 = 1,    /* int8 [N,K] + fp16 per-row scale                      */
    LLMIE_W_INT4 = 2,    /* packed int4 [N,K/2] + fp16 scale per (row, group)    */
    LLMIE_W_FP8 = 3,     /* e4m3 [N,K] + fp32 per-row scale                      */
    LLMIE_W_F32 = 4,     /* fp32 weights (dtype LLMIE_F32 engines only)          */
    LLMIE_W_MXFP4 = 5    /* OCP MXFP4: packed e2m1 [N,K/2] + e8m0 scale byte per (row, 32 k) */
} llmie_weight_format;

int llmie_abi_version(void);
const char *llmie_last_error(void);
/* "gfx950" -- the only architecture this library carries code objects for */
const char *llmie_target_arch(void);

/* ------------------------------------------------------------------------- */
/* 1. per-kernel entry points (one per reference launcher)                   */
/* ------------------------------------------------------------------------- */

/* replaces launchInputEmbedding        src/kernels/input_embedding.cu:24-51
 * out[t,:] = table[ids[t],:]; ids outside [0,vocab) -> row of zeros is NOT written
 * (status LLMIE_OK; the row is left untouched, as the reference would fault). */
int llmie_input_embedding(const int32_t *ids, const void *table, void *out,
                          int num_tokens, int hidden, int vocab,
                          llmie_dtype dtype, llmie_stream stream);

/* replaces launchCalPaddingOffset      src/kernels/cal_padding_offset.cu:45-70
 * padding_offset is packed (first sum(lens) ints written), cum_seqlens has batch+1 ints */
int llmie_cal_padding_offset(int32_t *padding_offset, int32_t *cum_seqlens,
                             const int32_t *input_lengths, int batch, int max_q_len,
                             llmie_stream stream);

/* replaces launchBuildCausalMasks      src/kernels/build_causal_mask.cu:25-42 */
int llmie_build_causal_mask(void *mask, const int32_t *q_lens, const int32_t *k_lens,
                            int batch, int max_q_len, int max_k_len,
                            llmie_dtype dtype, llmie_stream stream);

/* replaces launchRMSNorm               src/kernels/rmsnorm.cu:130-159
 * resid (nullable) = x;  x = x * gamma * rsqrt(mean(x^2)+eps)  in place */
int llmie_rmsnorm(void *x, void *resid, const void *gamma, float eps,
                  int num_tokens, int hidden, llmie_dtype dtype, llmie_stream stream);

/* replaces launchFusedAddBiasResidualAndRMSNorm  src/kernels/add_residual_and_rmsnorm.cu:170-201
 * out += resid; resid = out; out += bias (nullable); out = gamma*out*rsqrt(mean(out^2)+eps) */
int llmie_fused_add_bias_residual_rmsnorm(void *resid, void *out, const void *bias,
                                          const void *gamma, float eps,
                                          int num_tokens, int hidden,
                                          llmie_dtype dtype, llmie_stream stream);

/* replaces launchAddResidual           src/kernels/add_residual.cu:51-76     out += resid */
int llmie_add_residual(const void *resid, void *out, int num_tokens, int hidden,
                       llmie_dtype dtype, llmie_stream stream);

/* replaces launchLinearGemm            src/kernels/linear.cu:10-87 (+ cublas_utils.cpp:29-93)
 * trans_b != 0: y[M,N] = x[M,K] . W[N,K]^T ; trans_b == 0: y = x . W[K,N].
 * bias (nullable, [N]) and residual (nullable, [M,N], may alias y) are fused epilogues the
 * reference does in separate kernels; pass NULL for the plain reference semantics.
 * workspace: the counterpart of the scratch the reference's cublasWrapper argument owns (cublas_utils.cpp:29-93) -- caller-owned
 * fp32 slabs of the split-K forms (decode / short-prefill batches of up to 192 rows), llmie_linear_workspace_bytes() bytes,
 * 16-byte aligned.  NOTHING on the compute path allocates: a first call may already run under hipGraph capture.  NULL: fp16
 * runs its non-split kernels (slower at 8 < M <= 192); a non-NULL workspace that is too small is LLMIE_ERR_WORKSPACE. */
size_t llmie_linear_workspace_bytes(llmie_weight_format fmt, int M, int K, int N);
int llmie_linear(const void *x, const void *w, void *y, int M, int K, int N, int trans_b,
                 const void *bias, const void *residual,
                 llmie_dtype dtype, void *workspace, size_t workspace_bytes, llmie_stream stream);

/* replaces launchLinearGemm(gate_and_up) + launchSiluAndMul   src/layers/ffn.cpp:105-122,
 * src/kernels/silu_and_mul.cu:61-82 in one kernel: w is the fused gate_up matrix [2I,K]
 * (rows [0,I) gate, [I,2I) up); y[M,I] = silu(x.Wg^T) * (x.Wu^T).  fp16 only (decode path).
 * workspace: llmie_linear_workspace_bytes(LLMIE_W_F16, M, K, two_inter), see llmie_linear; without it 64 < M needs
 * prefill-sized shapes. */
int llmie_linear_swiglu(const void *x, const void *w, void *y, int M, int K, int two_inter,
                        llmie_dtype dtype, void *workspace, size_t workspace_bytes, llmie_stream stream);

/* Which kernel route llmie_linear (fmt LLMIE_W_F16, fp16, trans_b) / llmie_linear_swiglu (swiglu != 0) / llmie_linear_w8a16 /
 * llmie_linear_w4a16 would run this call on: the planned route's name ("splitk", "tiles256", "g8p", ...; the fp16 image routes
 * of int8 / int4 weights as "image_prefill+<route of the fp16 GEMM>"), from the same planner the entry points launch from.
 * Pure host function: the pointers are never dereferenced (only their alignment counts), the workspace is split exactly as the
 * entry points split it.  scale / group as in _w8a16 / _w4a16 (ignored for fp16).  A call the entry point would refuse returns
 * NULL and leaves the reason in llmie_last_error().  The string is valid until the thread's next call.
 * LLMIE_W_FP8: the route of llmie_linear_fp8 -- "fp8_gemv" (M <= 8, K within the GEMV's register budget), "fp8_gemm256" (the
 * 256-row tiled GEMM on the quantised activations) or "fp8_splitk" (passes of 128 rows over the slabs); scale = the fp32 row
 * scales, workspace as llmie_linear_fp8_workspace_bytes(M, K, N) sizes it (the activation part first, which has to be there, the
 * slabs behind it).  LLMIE_W_MXFP4: section "MXFP4 weights" below. */
const char *llmie_linear_route(llmie_weight_format fmt, const void *x, const void *w, const void *scale, const void *y, int M,
                               int K, int N, int swiglu, int group, const void *bias, const void *residual,
                               const void *workspace, size_t workspace_bytes);

/* How the 256-row tiled GEMM family cuts a prefill-sized projection into column tiles, and which kernels run the cuts: the plan the
 * "tiles256" / "swiglu256" / "g8p" routes, llmie_linear_fp8 / _fp8_swiglu and the prefill's QKV projection launch from.
 *   form:     0 plain (y[M,N], bias / residual), 1 SwiGLU (N = two_inter, the columns are those of the [M, N/2] output, N % 8 == 0),
 *             2 QKV projection with RoPE + KV-cache append as its epilogue (N % 128 == 0)
 *   operands: 0 fp16, 1 e4m3 weights and activations, 2 int8 weights under fp16 activations
 * Answer: the kernel family ("8p" eight-phase, "2s" two-stage where the eight-phase kernels' 32-bit offsets do not fit; named again
 * in front of a range that changes it), then one WIDTHxTILES@FIRSTCOL per launch: "8p 256x32@0 128x2@8192".  Any positive shape is
 * answered, also those whose grid does not fill the chip.  Pure host function; NULL + llmie_last_error() for other arguments.  The
 * string is valid until the thread's next call. */
const char *llmie_gemm256_tiles(int form, int operands, int M, int N, int K);

/* replaces launchLinearStridedBatchGemm src/kernels/linear.cu:89-158 (+ cublas_utils.cpp:95-154)
 * per batch i: C_i[m,n] = A_i[m,k] . B_i  (B_i is [n,k] if trans_b else [k,n]); dense strides */
int llmie_batched_gemm(const void *a, const void *b, void *c, int batch, int m, int n, int k,
                       int trans_b, llmie_dtype dtype, llmie_stream stream);

/* replaces launchFusedQKVAddBiasAndTransposeAndRope  src/kernels/qkv_bias_and_rope.cu:86-138
 * QKV[T, nh+2kvh, hs] -> q[bs,nh,S,hs], k/v[bs,kvh,S,hs]; RoPE at history_len[b]+local_token */
int llmie_qkv_bias_transpose_rope(void *q, void *k, void *v, const void *qkv, const void *bias,
                                  const int32_t *padding_offset, const int32_t *history_len,
                                  int batch, int seq_len, int num_tokens,
                                  int head_num, int kv_head_num, int head_size,
                                  int rotary_dim, float rotary_base,
                                  llmie_dtype dtype, llmie_stream stream);

/* replaces launchRope                  src/kernels/rope.cu:60-98
 * in place on qkv[bs, nh+2kvh, hs]; position = step-1.  If step_dev != NULL the position is
 * read from that device int (graph replay with a moving step) and `step` is ignored. */
int llmie_rope_decode(void *qkv, int batch, int head_num, int kv_head_num, int head_size,
                      int step, const int32_t *step_dev, int rotary_dim, float rotary_base,
                      llmie_dtype dtype, llmie_stream stream);

/* replaces launchDecoderMaskedMultiHeadAttention   src/kernels/decoder_self_attention.cu:211-270
 * qkv[bs, nh+2kvh, hs] (+bias) ; caches [L,bs,kvh,max_seq,hs]; out [bs, nh*hs].
 * Appends k,v at slot step-1 of `layer`, then attends over t < step.
 * workspace: llmie_decoder_mha_workspace_bytes() bytes (split-KV partials). */
size_t llmie_decoder_mha_workspace_bytes(int batch, int head_num, int head_size, int max_seq_len);
int llmie_decoder_mha(const void *qkv, const void *qkv_bias, void *k_cache, void *v_cache,
                      void *out, int layer, int batch, int head_num, int kv_head_num,
                      int head_size, int max_seq_len, int step, const int32_t *step_dev,
                      void *workspace, size_t workspace_bytes,
                      llmie_dtype dtype, llmie_stream stream);

/* Fused form used by the decoder engine: launchRope + launchDecoderMaskedMultiHeadAttention in one launch
 * (src/layers/self_attention.cpp:100-118).  rope_table: [max_pos][head_size/2] pairs (cos, sin) of
 * pos / base^(2j/rot_dim) (NULL = q,k already rotated); q and the new k are rotated in-kernel before the
 * bias add, exactly the reference's order.  tickets: [batch, kv_head_num] int32 arrival counters that must be
 * ZERO before the first call (the kernel re-arms them): the last workgroup of each (batch, kv head) merges the
 * split partials in the same launch (no merge kernel).  NULL tickets = separate merge kernel.
 * Supported: head_size in {32,64,128,256}, head_num/kv_head_num in {1,2,4,8}; else LLMIE_ERR_UNSUPPORTED. */
int llmie_decoder_mha_rope(const void *qkv, const void *qkv_bias, void *k_cache, void *v_cache,
                           void *out, int layer, int batch, int head_num, int kv_head_num,
                           int head_size, int max_seq_len, int step, const int32_t *step_dev,
                           void *workspace, size_t workspace_bytes, const void *rope_table,
                           int rotary_dim, int32_t *tickets, llmie_dtype dtype, llmie_stream stream);

/* Ragged batch (continuous batching; no reference counterpart: the reference's decode step shares ONE `step` across the batch,
 * decoder_self_attention.cu:211-270 / self_decoder.cpp:69): ctx_len_dev[b] = tokens of sequence b INCLUDING this step's; the RoPE
 * position, the append slot and the attention span are per sequence.  A value outside [1, max_seq_len] leaves that sequence's
 * cache and output untouched.  block_table (nullable) = paged cache, see llmie_decoder_forward_paged.  Row b equals the row a
 * batch-1 call at step ctx_len[b] produces, bit for bit (same kernels, same chunking). */
int llmie_decoder_mha_ragged(const void *qkv, const void *qkv_bias, void *k_cache, void *v_cache, void *out, int layer,
                             int batch, int head_num, int kv_head_num, int head_size, int max_seq_len,
                             const int32_t *ctx_len_dev, void *workspace, size_t workspace_bytes, const void *rope_table,
                             int rotary_dim, const int32_t *block_table, int max_pages, int num_pages,
                             llmie_dtype dtype, llmie_stream stream);

/* ABI 3 (an addition; host only, no device access).  The launch the three entries above -- and the engine's calls, which add the
 * e4m3 cache, the split-K slabs and the x32 output -- plan for a call, as one line of text:
 *   "split f16 hs128 rep4 kv=e4m3 cpw2 chunk512 grid 4x8x16 merge 32x16/128"   the split kernel's instantiation, chunks per workgroup,
 *        tokens per workgroup, grid (splits x kv heads x batch) and the merge launch (grid / block; "in-launch": by tickets; "none":
 *        one split)
 *   "generic f32 grid 32x2 lds 1028"   the kernel for any head size / ratio: grid (heads x batch), dynamic LDS bytes
 * NULL for a call they refuse: llmie_last_error() says why and *status (nullable) receives the code they return.
 * step: the host position (ignored with LLMIE_ATTN_STEP_DEV).  residues: address % 16 of each operand after the layer offset, 4 bits
 * each from bit 0: qkv, qkv_bias, k_cache, v_cache, slabs, the slab scales' wf and wh vectors, and (slab rows x columns) % 4.
 * workspace_bytes < 0: no workspace. */
#define LLMIE_ATTN_STEP_DEV 1u    /* the position is device resident (*step_dev, or ctx_len_dev) */
#define LLMIE_ATTN_RAGGED 2u      /* one context length per sequence */
#define LLMIE_ATTN_BIAS 4u
#define LLMIE_ATTN_ROPE 8u        /* rope_table given */
#define LLMIE_ATTN_TICKETS 16u
#define LLMIE_ATTN_SLABS 32u      /* q/k/v from the QKV projection's split-K slabs (engine) */
#define LLMIE_ATTN_PAGED 64u      /* block_table given, with max_pages / num_pages */
#define LLMIE_ATTN_X32 128u       /* the output is the x32 activation image (engine) */
#define LLMIE_ATTN_BAD_SCALES 256u /* e4m3 cache: a scale that is not positive */
const char *llmie_decoder_mha_plan(llmie_dtype dtype, int kv_e4m3, int batch, int head_num, int kv_head_num, int head_size,
                                   int max_seq_len, int step, unsigned forms, int max_pages, int num_pages,
                                   unsigned long long residues, long long workspace_bytes, int *status);

/* ABI 3 (an addition; no reference counterpart).  Sliding-window attention with sink tokens.
 * Positions are absolute and 0-based.  With window W >= 1 and S >= 0 sink tokens the query at position i sees key j iff
 *        j <= i  and  ( i - j < W  or  j < S )
 * W = 0 is full attention and S is then ignored.  RoPE is unchanged: keys are cached rotated at their absolute position, queries are
 * rotated at theirs, nothing is re-based.  The appended token always sees itself.  The softmax keeps the (sum + 1e-6) denominator.
 * In a decode step at context length `step` (the new token included) the live keys are [0, min(S, step)) and [max(0, step - W),
 * step); the ranges may overlap or touch, a key of both counts once.
 *
 * llmie_decoder_mha_window: llmie_decoder_mha_ragged's operands and behaviour (ctx_len_dev[b] = context length of sequence b with
 * this step's token; block_table nullable) under that mask, plus `tickets` (nullable; llmie_decoder_mha_rope) and, with kv_e4m3 != 0,
 * caches of e4m3 bytes, stored = e4m3(x / scale) (fp16 activations; separate merge only).  The split kernel walks only the chunks
 * that hold a live key -- the grid's x extent is at most ceil(S / chunk) + ceil(W / chunk) + 1 whatever max_seq_len is -- and never
 * follows the block-table entry of a page without a live key, so such entries may be unmapped (-1).  Supported with a window: fp16
 * activations, head_size 64 / 128, head_num / kv_head_num in {1,2,4,8} (e4m3 cache: {1,2,4}); everything else with window > 0 is
 * LLMIE_ERR_UNSUPPORTED.  window = 0 makes the call llmie_decoder_mha_ragged makes; a window >= the context gives its output bit
 * for bit.  llmie_decoder_mha_window_plan: llmie_decoder_mha_plan for such a call; with a window the line gains
 * " window W sinks S live N" (N live chunks of the host step) or "... live <=N" (device position: the grid's bound). */
int llmie_decoder_mha_window(const void *qkv, const void *qkv_bias, void *k_cache, void *v_cache, void *out, int layer,
                             int batch, int head_num, int kv_head_num, int head_size, int max_seq_len,
                             const int32_t *ctx_len_dev, void *workspace, size_t workspace_bytes, const void *rope_table,
                             int rotary_dim, const int32_t *block_table, int max_pages, int num_pages, int window, int sinks,
                             int32_t *tickets, int kv_e4m3, float k_scale, float v_scale, llmie_dtype dtype, llmie_stream stream);
const char *llmie_decoder_mha_window_plan(llmie_dtype dtype, int kv_e4m3, int batch, int head_num, int kv_head_num, int head_size,
                                          int max_seq_len, int step, unsigned forms, int max_pages, int num_pages,
                                          unsigned long long residues, long long workspace_bytes, int window, int sinks,
                                          int *status);

/* ABI 3 (an addition; no reference counterpart).  A learned sink logit per query head ("head sink"; gpt-oss `self_attn.sinks`).
 * "Sinks" keeps meaning sink TOKENS (above); the two features compose.  head_sink: device array of fp32, [head_num] for one layer
 * ([num_layers, head_num] on an engine, llmie_decoder_set_head_sinks); a loader converts stored bf16 values to fp32.  Let l_j be the
 * scaled logits of the keys the mask exposes to the query (causal; with a window, the window and its sink tokens) and s_h the value
 * of query head h.  Its softmax runs over those keys and ONE extra column with logit s_h and no value row:
 *        M   = max(max_j l_j, s_h)
 *        out = sum_j exp(l_j - M) v_j / (sum_j exp(l_j - M) + exp(s_h - M) + 1e-6)
 * The extra term enters exactly once per (query row, head), whatever the number of splits, waves, tiles or lanes that share the row.
 * s_h = -INFINITY is "no sink for this head" and gives the bits of the call without a head sink.  The array is read on the device at
 * every launch, so a captured step replays with new values.  NaN values: results unspecified; the call stays in bounds and ends.
 *
 * llmie_decoder_mha_sink: llmie_decoder_mha_window's operands and behaviour plus head_sink (nullable: NULL is that entry's call, bit
 * for bit).  Supported with a head sink where the windowed form is: fp16 activations, head_size 64 / 128, head_num / kv_head_num in
 * {1,2,4,8} (e4m3 cache: {1,2,4}), dense or paged, tickets or separate merge; anything else with head_sink != NULL is
 * LLMIE_ERR_UNSUPPORTED and writes nothing.  llmie_decoder_mha_sink_plan: llmie_decoder_mha_window_plan plus the form bit
 * LLMIE_ATTN_HEAD_SINK (the two older plan queries ignore the bit); the line gains " head_sink" when it is set -- same grid, slots and
 * merge, the SINK instantiation of the kernels. */
#define LLMIE_ATTN_HEAD_SINK 512u /* head_sink given */
int llmie_decoder_mha_sink(const void *qkv, const void *qkv_bias, void *k_cache, void *v_cache, void *out, int layer,
                           int batch, int head_num, int kv_head_num, int head_size, int max_seq_len,
                           const int32_t *ctx_len_dev, void *workspace, size_t workspace_bytes, const void *rope_table,
                           int rotary_dim, const int32_t *block_table, int max_pages, int num_pages, int window, int sinks,
                           int32_t *tickets, int kv_e4m3, float k_scale, float v_scale, const float *head_sink /* device, [head_num] */,
                           llmie_dtype dtype, llmie_stream stream);
const char *llmie_decoder_mha_sink_plan(llmie_dtype dtype, int kv_e4m3, int batch, int head_num, int kv_head_num, int head_size,
                                        int max_seq_len, int step, unsigned forms, int max_pages, int num_pages,
                                        unsigned long long residues, long long workspace_bytes, int window, int sinks,
                                        int *status);

/* ABI 3 (an addition; no reference counterpart).  QK-norm: a learned RMSNorm over head_size on every q head and every k head,
 * between the QKV projection and RoPE (Qwen3 `self_attn.q_norm` / `self_attn.k_norm`, shape [head_size]).  For a head row
 * x[0..hs) of the projection's output (fp16), a gamma g[0..hs) (fp16) and eps >= 0:
 *        ss  = sum_d float(x_d)^2                         fp32, in ONE fixed order (below)
 *        inv = 1 / sqrt(ss / hs + eps)                    fp32
 *        n_d = fp16( (float(x_d) * inv) * float(g_d) )    one rounding
 * It is applied to every q head with q_gamma and to every k head with k_gamma, never to v, BEFORE RoPE: the rotation reads the fp16
 * value n_d.  A Gemma-style (1 + w) gamma is the loader's business: it passes 1 + w.  QK-norm together with a QKV bias is refused
 * with LLMIE_ERR_UNSUPPORTED (no checkpoint has both, and decode and prefill add the bias on different sides of RoPE).
 * Summation order: within each aligned group of 8 consecutive elements ss_g = fmaf(x, x, ss_g) in ascending d, from 0; the hs / 8
 * group sums are combined by a butterfly over the bits of the group index, lowest bit first, with plain fp32 adds.  The operator,
 * the fused decode kernel (both cache formats) and the prefill kernel follow it, so they agree to the bit.
 * The gammas are DEVICE arrays read at every launch: a captured step replays with new values.  NaN / Inf gammas: results
 * unspecified; the call stays in bounds and ends.
 *
 * llmie_qk_norm: the operator on its own, in place on packed rows [rows, (head_num + 2 kv_head_num) * head_size]; the v columns are
 * not touched.  fp16, head_size 64 / 128.  The per-kernel path runs it between llmie_linear and llmie_qkv_bias_transpose_rope.
 * LLMIE_ERR_INVALID_ARG: NULL pointers; non-positive sizes; head_num % kv_head_num != 0; eps < 0 or NaN; qkv or a gamma not
 * 16-byte aligned.  LLMIE_ERR_UNSUPPORTED: LLMIE_F32; other head sizes.  Nothing is written in either case.
 *
 * llmie_decoder_mha_qknorm: llmie_decoder_mha_sink's operands and behaviour plus the gammas (device, [head_size] each, nullable
 * together: both NULL is that entry's call, bit for bit; exactly one NULL, a gamma not 16-byte aligned or qk_eps < 0 / NaN is
 * LLMIE_ERR_INVALID_ARG).  With gammas the output, the caches and the pools are those of llmie_qk_norm on qkv followed by
 * llmie_decoder_mha_sink(head_sink = NULL), bit for bit.  Supported with gammas: fp16 activations, head_size 64 / 128,
 * head_num / kv_head_num in {1,2,4,8} (e4m3 cache: {1,2,4}), dense or paged, tickets or separate merge.  With gammas each of a QKV
 * bias, window > 0, head_sink != NULL, fp32, head size 32 / 256, ratio 8 over e4m3 and operands that would fall to the generic
 * kernel (unaligned buffers) is LLMIE_ERR_UNSUPPORTED and writes nothing.  llmie_decoder_mha_qknorm_plan:
 * llmie_decoder_mha_sink_plan plus the form bit LLMIE_ATTN_QK_NORM (the three older plan queries ignore the bit); the line gains
 * " qk_norm" when it is set -- same grid, slots and merge, the QKN instantiation of the split kernel. */
#define LLMIE_ATTN_QK_NORM 1024u /* q_gamma / k_gamma given */
int llmie_qk_norm(void *qkv /* [rows, (head_num + 2 kv_head_num) * head_size], in place */, int rows, int head_num, int kv_head_num,
                  int head_size, const void *q_gamma, const void *k_gamma /* device, [head_size] each */, float eps,
                  llmie_dtype dtype, llmie_stream stream);
int llmie_decoder_mha_qknorm(const void *qkv, const void *qkv_bias, void *k_cache, void *v_cache, void *out, int layer,
                             int batch, int head_num, int kv_head_num, int head_size, int max_seq_len,
                             const int32_t *ctx_len_dev, void *workspace, size_t workspace_bytes, const void *rope_table,
                             int rotary_dim, const int32_t *block_table, int max_pages, int num_pages, int window, int sinks,
                             int32_t *tickets, int kv_e4m3, float k_scale, float v_scale, const float *head_sink /* device, [head_num] */,
                             const void *q_gamma, const void *k_gamma /* device [head_size], nullable together */, float qk_eps,
                             llmie_dtype dtype, llmie_stream stream);
const char *llmie_decoder_mha_qknorm_plan(llmie_dtype dtype, int kv_e4m3, int batch, int head_num, int kv_head_num, int head_size,
                                          int max_seq_len, int step, unsigned forms, int max_pages, int num_pages,
                                          unsigned long long residues, long long workspace_bytes, int window, int sinks,
                                          int *status);

/* ABI 3 (an addition; host only, no device access).  RoPE frequency scaling: the one function that computes a (cos, sin) table.
 * cos_sin_out: host, [max_pos][head_size/2] pairs (cos, sin), the layout of llmie_decoder_mha_rope's rope_table.  For pair
 * j < rotary_dim/2 with f_j = rotary_base^(-2j/rotary_dim) the entry at position p is (cos(p f'_j), sin(p f'_j)) a, where
 *   LLMIE_ROPE_LINEAR  f'_j = f_j / factor
 *   LLMIE_ROPE_LLAMA3  wavelength w = 2 pi / f_j;  w > original/low_freq_factor: f_j / factor;  w < original/high_freq_factor: f_j;
 *                      otherwise t = (original/w - low_freq_factor) / (high_freq_factor - low_freq_factor), f'_j = (1-t) f_j/factor + t f_j
 *   LLMIE_ROPE_YARN    c(n) = rotary_dim ln(original / (2 pi n)) / (2 ln base); lo = c(beta_fast), hi = c(beta_slow); with `truncate`
 *                      lo = floor(lo), hi = ceil(hi); then lo = max(lo, 0), hi = min(hi, rotary_dim - 1), hi += 0.001 if equal;
 *                      ramp_j = clamp((j - lo)/(hi - lo), 0, 1); f'_j = f_j/factor ramp_j + f_j (1 - ramp_j); a = the attention factor
 * (a = 1 for the other kinds).  factor >= 1 is used by every kind but NONE; original_max_pos by LLAMA3 and YARN; low_/high_freq_factor
 * by LLAMA3; beta_fast, beta_slow, attn_factor and truncate by YARN: a beta of 0 means 32 / 1, an attn_factor <= 0 means
 * 0.1 ln(factor) + 1.  Entries with j >= rotary_dim/2 stay (1, 0), unscaled.  Scaled kinds are evaluated in double and rounded once
 * to fp32.  LLMIE_ROPE_NONE, or scaling = NULL, runs the fp32 formula llmie_decoder_create has always used (cosf / sinf of
 * p / powf(base, 2j/rotary_dim)) and gives that table bit for bit; llmie_decoder_create calls this function with NULL.
 * LLMIE_ERR_INVALID_ARG: NULL output, max_pos < 1, an odd or non-positive head_size, rotary_dim odd or outside [2, head_size],
 * base <= 0, an unknown kind, factor < 1 (or not finite), original_max_pos < 1 where used, high_freq_factor <= low_freq_factor or
 * low_freq_factor <= 0 (LLAMA3), a negative beta (YARN). */
typedef enum { LLMIE_ROPE_NONE = 0, LLMIE_ROPE_LINEAR, LLMIE_ROPE_LLAMA3, LLMIE_ROPE_YARN } llmie_rope_kind;
typedef struct {
    llmie_rope_kind kind;
    float factor;
    int original_max_pos;
    float low_freq_factor, high_freq_factor;
    float beta_fast, beta_slow;
    float attn_factor;
    int truncate;
} llmie_rope_scaling;
int llmie_rope_table_fill(float *cos_sin_out, int max_pos, int head_size, int rotary_dim, float rotary_base,
                          const llmie_rope_scaling *scaling);

/* ABI 3 (an addition).  The page ring of windowed sequences over a paged cache: one launch, nothing read by the host, so a captured
 * decode loop replays it.  For every sequence b and every logical page that the positions [cached_len[b], cached_len[b] + n) need
 * (n = new_tokens[b], or 1 with new_tokens = NULL) and whose block-table entry is unmapped (-1), it takes the pool page of the
 * lowest mapped logical page that lies wholly at or above the sink pages and wholly below cached_len[b] + 1 - window (dead for this
 * and every later query), maps it at the new index and unmaps the old one; status[b] = 0.  Without enough dead pages status[b] = 1
 * and the row is left as it was: the caller must supply a page.  status[b] = 2: the positions do not fit max_pages.  A sequence
 * then lives in ceil(S / 128) + ceil((W + n) / 128) + 1 pool pages at any context length.  window: the LARGEST window of any layer
 * (>= 1).  Not applicable when some layer attends to everything, or when table rows share pages (llmie_kv_pages_fork). */
int llmie_kv_window_advance(int32_t *block_table /* [batch, max_pages] in/out */, int max_pages, const int32_t *cached_len /* [batch] */,
                            const int32_t *new_tokens /* [batch] or NULL = 1 each */, int batch, int window, int sinks,
                            int32_t *status /* [batch] */, llmie_stream stream);

/* replaces launchConcatKVCache         src/kernels/concat_past_kv.cu:44-89  (one call = K or V) */
int llmie_concat_kv(const void *src, void *cache, const int32_t *cur_len,
                    const int32_t *history_len, int layer, int batch, int kv_head_num,
                    int max_q_len, int max_seq_len, int head_size,
                    llmie_dtype dtype, llmie_stream stream);

/* replaces launchRepeatKVCache         src/kernels/repeat_kv.cu:51-106      (one call = K or V) */
int llmie_repeat_kv(const void *cache, void *dst, const int32_t *ctx_len, int layer, int batch,
                    int head_num, int kv_head_num, int max_k_len, int max_seq_len, int head_size,
                    llmie_dtype dtype, llmie_stream stream);

/* replaces launchFusedScaleMaskAndSoftmax  src/kernels/scale_and_mask_and_softmax.cu:213-341
 * out may alias qk */
int llmie_scale_mask_softmax(const void *qk, const void *mask, void *out, float scale,
                             int batch, int head_num, int q_len, int k_len,
                             llmie_dtype dtype, llmie_stream stream);

/* replaces launchFusedTransposeAndRemovePadding  src/kernels/transpose_and_remove_padding.cu:45-74 */
int llmie_transpose_remove_padding(const void *src, void *dst, const int32_t *padding_offset,
                                   int num_tokens, int batch, int seq_len, int head_num,
                                   int head_size, llmie_dtype dtype, llmie_stream stream);

/* replaces launchSiluAndMul            src/kernels/silu_and_mul.cu:61-82   in[T,2,I] -> out[T,I] */
int llmie_silu_and_mul(const void *in, void *out, int num_tokens, int inter,
                       llmie_dtype dtype, llmie_stream stream);

/* replaces launchTopKForBeamSearch     src/kernels/topk.cu:104-140
 * probs[rows,vocab] -> ids/vals[rows,K] descending (ties: lower id first).
 * tmp_ids/tmp_vals: [rows, blocks_per_row, K] scratch (the reference's round-1 buffers);
 * 1 <= K <= 32, 1 <= blocks_per_row <= 64. */
int llmie_topk(const void *probs, int32_t *tmp_ids, void *tmp_vals, int32_t *ids, void *vals,
               int rows, int vocab, int K, int blocks_per_row,
               llmie_dtype dtype, llmie_stream stream);

/* replaces launchSampling              src/kernels/sampling.cu:73-102
 * topk_val is NOT modified (the reference overwrites it with the exponentials).
 * finished is a byte per sequence (C++ bool).  Uniform draw: Philox4x32-10(seed=step, stream=b).
 * If step_dev != NULL the seed is read from that device int. */
int llmie_sampling(const int32_t *topk_id, const void *topk_val, int32_t *seq_len,
                   uint8_t *finished, int32_t *out_id, int batch, int K, int step,
                   const int32_t *step_dev, int end_id, int vocab,
                   llmie_dtype dtype, llmie_stream stream);

/* ABI 3.  Per-request sampling controls (no reference launcher: the reference samples from the top-K at temperature 1).
 * One entry per row of the batch, read on the device from params_dev[batch] (a captured graph picks up new values on replay).
 * Per row, from logits[b, 0..V) read as fp32:
 *   1 penalties, once per distinct id t of history[b, 0..history_len[b]) (ids outside [0, V) ignored, c_t = its count):
 *     l_t <- (l_t > 0 ? l_t / rep : l_t * rep) - presence - c_t * frequency, in fp32 in that order;
 *   2 temperature == 0: greedy (largest penalised logit, ties -> lower id, no draw); else l <- l / T clamped to +-FLT_MAX;
 *   3 top_k (0 = off) keeps exactly min(top_k, valid) tokens in (value desc, id asc) order -- llmie_topk's order;
 *   4 softmax exp(l - max) over them;  5 top_p (>= 1 = off): the smallest prefix of that order whose mass is >= top_p x the
 *     total, widened to every token whose value equals the prefix's last;  6 min_p (0 = off): probability >= min_p x the max;
 *   7 u = Philox4x32-10(seed = step, stream = params.seed) (llmie_sampling's generator); the pick is the first kept token, in
 *     that order, at which the running mass exceeds u x the kept mass (u == 1: the last kept token).
 * NaN logits are excluded everywhere; a row without a valid token emits end_id.  out_id / seq_len / finished follow
 * llmie_sampling.  out_logprob (may be NULL) = log_softmax(raw logits)[chosen], before penalties, temperature and truncation.
 * history_append != 0: the pick is written at history[b, history_len[b]] and history_len[b] += 1 while history_len[b] <
 * history_stride.  history / history_len may be NULL when history_stride == 0; history_stride <= LLMIE_SAMPLE_MAX_HISTORY.
 * Clamped on the device: temperature < 0 / NaN -> 0; top_k < 0 -> 0, > V -> V; top_p <= 0 keeps one token, > 1 -> 1; min_p to
 * [0, 1]; repetition_penalty <= 0 / NaN -> 1.
 * Determinism: masses are fixed point, floor(exp(l - max) * 2^32) summed as uint64 (exact, in any order), so the same inputs
 * give the same bits and a row's result does not depend on the other rows or the batch size.  The cost: a token whose
 * exp(l - max) is below 2^-32 has mass 0 and is never drawn, and masses carry a 2^-32 absolute rounding (the float sums of
 * llmie_sampling can pick the neighbour when u sits on a boundary).
 * One launch per call (one 1024-thread workgroup per row).  workspace: llmie_sample_logits_workspace_bytes(batch, vocab)
 * bytes, 16-byte aligned (a fp32 / key copy of each row). */
typedef struct {
    float temperature;
    int top_k;
    float top_p;
    float min_p;
    float repetition_penalty;
    float presence_penalty;
    float frequency_penalty;
    uint32_t seed;
} llmie_sampling_params;
#define LLMIE_SAMPLE_MAX_HISTORY 8192
size_t llmie_sample_logits_workspace_bytes(int batch, int vocab);
int llmie_sample_logits(const void *logits, int batch, int vocab, const llmie_sampling_params *params_dev, int32_t *history,
                        int history_stride, int32_t *history_len, int history_append, int32_t *seq_len, uint8_t *finished,
                        int32_t *out_id, float *out_logprob, int step, const int32_t *step_dev, int end_id, void *workspace,
                        size_t workspace_bytes, llmie_dtype dtype, llmie_stream stream);

/* ABI 3 (an addition).  llmie_sample_logits with four more per-request controls, each read from device memory inside the same
 * launch (a captured graph picks up new contents on replay): an allowed-token bit mask (constrained decoding), a logit bias
 * list, a set of stop tokens with a minimum step, and the top-N alternatives of the row.  ext == NULL, or a struct with every
 * pointer NULL and top_n == 0, IS llmie_sample_logits: the same launch and the same bits.  Otherwise the numbered steps of
 * llmie_sample_logits are extended as follows (V = vocab, `step` = the value the Philox seed uses: *step_dev or the argument):
 *   0a bias: for every id of bias_ids[b, 0..bias_len[b]) (bias_len clamped to [0, bias_stride]) l_t <- l_t + bias, one plain
 *      fp32 add, applied ONCE per distinct id, before the penalties of step 1.  Ids outside [0, V) and entries whose value is
 *      NaN or +INFINITY are ignored as if they were absent; of the remaining entries that name one id the LAST of the list
 *      wins (whatever the thread order).  A value of -INFINITY bans the token: it is excluded (0b).
 *   0b mask: a token is EXCLUDED if the row is constrained and the token's bit is clear, if it is banned, or if
 *      step < min_step[b] and it is end_id or one of stop_ids[b, 0..stop_len[b]).  An excluded token is treated everywhere as a
 *      NaN logit is: it cannot be the greedy pick, does not count as valid (top_k clamps to the valid count), has no mass and
 *      cannot be drawn.  A row with no token left emits end_id and sets finished (the rule for a row without a valid token).
 *      Row b is constrained by mask row m = (mask_index ? mask_index[b] : b) if allowed_mask != NULL and 0 <= m < mask_rows;
 *      token v is allowed iff bit (v % 32) of word allowed_mask[m * mask_stride + v / 32] is set; bits at and past V are ignored.
 *   8  stops: finished[b] = (pick == end_id) || pick is one of stop_ids[b, 0..stop_len[b]) (stop_len clamped to
 *      [0, stop_stride]); seq_len and the history append are those of llmie_sample_logits.
 * Reporting is of the model, not of the controls.  out_logprob stays log_softmax(raw logits)[pick].  out_top_ids[b, 0..top_n)
 * are the top_n largest RAW logits of the row in llmie_topk's order (value descending, ties -> lower id, -0 == +0, NaN
 * excluded), whatever the mask, bias, penalties, temperature and truncation are; out_top_logprobs[b, i] is their raw
 * log-softmax (value - log-sum-exp of the raw row).  Entries past the row's count of non-NaN logits hold id -1 and -INFINITY.
 * Comparing out_logprob with out_top_logprobs[b, 0] shows what a constraint cost.
 * Determinism and batch invariance are those of llmie_sample_logits: same inputs, same bits; a row's outputs (top-N
 * included) depend neither on its slot nor on the other rows.
 * Refused on the host before any launch.  LLMIE_ERR_INVALID_ARG: a negative stride or top_n; one of bias_ids / bias_vals /
 * bias_len without the other two; stop_ids without stop_len or the reverse; allowed_mask with mask_stride < ceil(V / 32) or
 * mask_rows < 1, or with mask_index == NULL and mask_rows < batch; mask_index without allowed_mask; top_n > 0 without both
 * outputs.  LLMIE_ERR_UNSUPPORTED: bias_stride, stop_stride or top_n above its LLMIE_SAMPLE_MAX_*.  (min_step alone is
 * legal: it then holds back end_id.)
 * Workspace, launch count (one), no allocation, no synchronisation, capture: as llmie_sample_logits (the same workspace query).
 * A mask row is loaded 16 bytes at a time where allowed_mask and mask_stride keep its rows 16-byte aligned. */
#define LLMIE_SAMPLE_MAX_BIAS   1024
#define LLMIE_SAMPLE_MAX_STOPS  16
#define LLMIE_SAMPLE_MAX_TOP_N  32      /* llmie_topk's bound on K */
typedef struct {                 /* host struct; every pointer is a DEVICE pointer and may be NULL (= that control is off) */
    const uint32_t *allowed_mask;   /* [mask_rows, mask_stride] words; token v is allowed iff bit (v % 32) of word v / 32 is set */
    int mask_stride;                /* words per mask row, >= ceil(vocab / 32); bits at and past `vocab` are ignored */
    int mask_rows;
    const int32_t *mask_index;      /* [batch]: which mask row sequence b uses; < 0 or >= mask_rows: unconstrained.
                                       NULL: row b uses mask row b (mask_rows >= batch) */
    const int32_t *bias_ids;        /* [batch, bias_stride] */
    const float   *bias_vals;       /* [batch, bias_stride] */
    const int32_t *bias_len;        /* [batch], clamped on the device to [0, bias_stride] */
    int bias_stride;                /* <= LLMIE_SAMPLE_MAX_BIAS */
    const int32_t *stop_ids;        /* [batch, stop_stride] */
    const int32_t *stop_len;        /* [batch], clamped to [0, stop_stride] */
    int stop_stride;                /* <= LLMIE_SAMPLE_MAX_STOPS */
    const int32_t *min_step;        /* [batch]: while step < min_step[b], end_id and the row's stop ids cannot be picked */
    int top_n;                      /* 0 .. LLMIE_SAMPLE_MAX_TOP_N */
    int32_t *out_top_ids;           /* [batch, top_n] */
    float   *out_top_logprobs;      /* [batch, top_n] */
} llmie_sampling_ext;
int llmie_sample_logits_ext(const void *logits, int batch, int vocab, const llmie_sampling_params *params_dev, int32_t *history,
                            int history_stride, int32_t *history_len, int history_append, int32_t *seq_len, uint8_t *finished,
                            int32_t *out_id, float *out_logprob, int step, const int32_t *step_dev, int end_id, void *workspace,
                            size_t workspace_bytes, llmie_dtype dtype, llmie_stream stream, const llmie_sampling_ext *ext);

/* ABI 3 (an addition).  Score given tokens: RMSNorm + LM head + log-softmax over `rows` hidden states at once, for prompt
 * log-probabilities ("echo + logprobs"), perplexity and ranking by likelihood.  No reference launcher: the reference computes
 * logits for the last prompt token only.  The [rows, vocab] logits are never written and never rounded to fp16.  Per row t:
 *   1 x[t] = RMSNorm(hidden[t], norm_gamma, rms_eps) rounded to fp16 -- the bits llmie_rmsnorm leaves in place (it runs on a
 *     copy in the workspace; `hidden` is NOT modified).  norm_gamma == NULL: x = hidden.
 *   2 z[t, v] = sum_k x[t, k] * lm_head[v, k] (+ lm_bias[v]), accumulated and kept in fp32.
 *   3 lse[t] = log sum_v exp(z[t, v]) with a running maximum (logits of magnitude 200 do not overflow).
 *   4 out_logprob[t] = z[t, targets[t]] - lse[t].  A target outside [0, vocab) means "no target" (the last token of a sequence):
 *     out_logprob[t] = 0, lse and argmax are still produced.
 *   5 out_argmax[t] = id of the largest z[t, :], ties -> lower id (llmie_topk's rule); out_argmax_logprob[t] = max - lse[t].
 * out_lse / out_argmax / out_argmax_logprob may be NULL.  Rows past `rows` of the outputs are not written.
 * Determinism: the vocabulary is cut into spans of column tiles by `vocab` alone and the spans' partial (max, sum, best) are
 * merged in span order without atomics, so the same inputs give the same bits and a row's result depends neither on `rows`
 * nor on the row's position.
 * LLMIE_F16 only (LLMIE_F32: LLMIE_ERR_UNSUPPORTED); hidden_size % 64 == 0 and 16-byte aligned hidden / lm_head, else
 * LLMIE_ERR_UNSUPPORTED; rows >= 1, any vocab >= 1.  workspace: llmie_score_tokens_workspace_bytes(rows, hidden_size, vocab)
 * bytes, 16-byte aligned: the normalised rows (rows * hidden_size halves) and 32 bytes per (row, span), at most 32 spans --
 * never rows * vocab.  NULL / short: LLMIE_ERR_WORKSPACE.  No allocation, no synchronisation; legal inside a graph capture. */
size_t llmie_score_tokens_workspace_bytes(int rows, int hidden_size, int vocab);
int llmie_score_tokens(const void *hidden, const void *norm_gamma, float rms_eps, const void *lm_head, const void *lm_bias,
                       const int32_t *targets, float *out_logprob, float *out_lse, int32_t *out_argmax,
                       float *out_argmax_logprob, int rows, int hidden_size, int vocab, void *workspace,
                       size_t workspace_bytes, llmie_dtype dtype, llmie_stream stream);

/* ------------------------------------------------------------------------- */
/* 2. weight-only quantised / fp8 linears (reference: planned only,           */
/*    README.md:36-39, linear.cuh:12 TODO)                                    */
/* ------------------------------------------------------------------------- */

/* y[M,N] = x[M,K] . (scale[n]*Wq[n,k])^T ; x,y,scale,bias fp16; Wq int8 row-major [N,K].
 * workspace: llmie_linear_workspace_bytes(LLMIE_W_INT8 / LLMIE_W_INT4, M, K, N) bytes of caller-owned split-K slabs (see
 * llmie_linear); without it int8 serves M <= 64 and int4 the GEMV sizes only.  int8 shapes none of the int8 kernels take
 * (8 < M < 192 with K % 256 != 0 beyond 64 rows, or K % 16 != 0) run on an fp16 image of W that the workspace holds as well. */
int llmie_linear_w8a16(const void *x, const int8_t *wq, const void *scale, void *y,
                       int M, int K, int N, const void *bias, const void *residual,
                       void *workspace, size_t workspace_bytes, llmie_stream stream);
/* int4: two nibbles per byte (low nibble = even k), value = nibble-8, scale[n, k/group] fp16 */
int llmie_linear_w4a16(const void *x, const uint8_t *wq, const void *scale, void *y,
                       int M, int K, int N, int group, const void *bias, const void *residual,
                       void *workspace, size_t workspace_bytes, llmie_stream stream);
/* fp8 e4m3 (OCP) weights [N,K] with per-row fp32 scale; x fp16 is quantised per token to e4m3
 * on the fly (scale = amax/448); y[m,n] = w_scale[n] * x_scale[m] * sum_k wq[n,k] xq[m,k], fp32 accumulate; y fp16.
 * M <= 8: K-split GEMV (same arithmetic on the VALU); 8 < M: split-K fp8 MFMA (K % 256 == 0, K >= 512; 64 < M <= 128 rows per
 * pass take the 128-row LDS-DMA form);
 * prefill-sized M x N (>= 192 tiles of 256 x 256 or 256 x 128): tiled v_mfma_scale_f32_16x16x128_f8f6f4 GEMM
 * (K % 128 == 0).  workspace = quantised activations + per-token scales + the fp32 slabs of the split-K form, all caller-owned:
 * llmie_linear_fp8_workspace_bytes(M, K, N) bytes, 256-byte aligned. */
int llmie_linear_fp8(const void *x, const uint8_t *w_fp8, const float *w_scale, void *y,
                     int M, int K, int N, const void *bias, const void *residual,
                     void *workspace, size_t workspace_bytes, llmie_stream stream);
size_t llmie_linear_fp8_workspace_bytes(int M, int K, int N);   /* N = 0: the activation part only (llmie_linear_fp8_swiglu) */
/* y[M, two_inter/2] = silu(gate) * up of the fused gate_up projection in fp8 (ffn.cpp:105-122 in one launch after the
 * activation quantisation); prefill-sized shapes only (LLMIE_ERR_UNSUPPORTED otherwise: use llmie_linear_fp8 +
 * llmie_silu_and_mul) */
int llmie_linear_fp8_swiglu(const void *x, const uint8_t *w_fp8, const float *w_scale, void *y, int M, int K,
                            int two_inter, void *workspace, size_t workspace_bytes, llmie_stream stream);
/* offline quantisers (device side): w fp16 [N,K] -> int8/int4/fp8 + scales */
int llmie_quantize_w8(const void *w, int8_t *wq, void *scale, int N, int K, llmie_stream stream);
int llmie_quantize_w4(const void *w, uint8_t *wq, void *scale, int N, int K, int group,
                      llmie_stream stream);
int llmie_quantize_fp8(const void *w, uint8_t *wq, float *scale, int N, int K, llmie_stream stream);

/* MXFP4 weights (OCP microscaling, an addition within ABI 3; no reference counterpart).  LLMIE_W_MXFP4 = 5.  A matrix W[N, K] with
 * K % 32 == 0 is stored as two arrays:
 *   wq     uint8 [N, K/2], two e2m1 codes per byte, low nibble = even k (the int4 entries' packing).  Bit 3 of a code is the sign,
 *          bits 2..0 index the magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6}; code 0x8 is -0.
 *   scale  uint8 [N, K/32], row-major, e8m0: block (n, k/32) has exponent e = byte - 127 and w[n, k] = magnitude * 2^e with the
 *          code's sign.  Byte 0xFF is NaN.  (This array is what llmie_matrix.scale would carry.)
 * Pinned range: for e in [-23, 13] every weight is exactly an fp16 number (subnormals included, 6 * 2^13 = 49152), and inside that
 * range every route of llmie_linear_mxfp4 agrees on the weight to the bit.  Outside it, or with a 0xFF block, llmie_linear_mxfp4
 * returns unspecified values for the affected columns; it stays in bounds and terminates.
 *
 * llmie_quantize_mxfp4: w fp16 [N, K] -> codes + scales.  Per block of 32 with amax = max |w|: a non-finite element gives scale
 * byte 0xFF (the block's codes are then unspecified); amax == 0 gives byte 127 and all-zero magnitudes; otherwise
 * e = clamp(floor(log2(amax)) - 2, -23, 13) (the OCP rule with emax(e2m1) = 2; the lower clamp departs from OCP on purpose: fp16
 * inputs reach e = -26, where codes would stop being fp16 numbers, and with the clamp such a block lands losslessly on the fp16
 * subnormal grid).  Each element is w / 2^e rounded to the nearest magnitude, ties to the even code (0.25 -> 0, 0.75 -> 1,
 * 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4), saturating at 6.  The sign bit is the sign bit of w, also for a zero result.
 * K % 32 != 0 or w not 16-byte aligned: LLMIE_ERR_UNSUPPORTED.
 * llmie_dequantize_mxfp4: w16[n, k] = the round-to-nearest-even fp16 of the exact value (exact in the pinned range; outside it
 * overflow to +-inf and underflow through the subnormals; a 0xFF block gives fp16 NaN 0x7E00; -0 stays -0).  K % 32 != 0 or w16 not
 * 16-byte / wq not 4-byte aligned: LLMIE_ERR_UNSUPPORTED.
 * llmie_linear_mxfp4: weight-only, y[m, n] = fp16(sum_k float(x[m, k]) * w[n, k] (+ bias[n]) (+ residual[m, n])); x, y, bias,
 * residual fp16, residual may alias y; fp32 accumulation, a block's 2^e applied to the block's fp32 partial sum; no float atomics:
 * same inputs, same bits.  Routes (llmie_linear_route(LLMIE_W_MXFP4, ...) names them): M <= 8 "mxfp4_gemv" (one pass over the
 * weights for all rows); 8 < M <= 64 "mxfp4_mfma" (codes expanded to unscaled fp16 fragments, one v_mfma_f32_16x16x32_f16 per block
 * into a zeroed tile, the tile scaled per lane and added to the accumulator; K split over the waves of a workgroup and reduced in a
 * fixed order); 64 < M < 192 "mxfp4_chunks" (passes of <= 64 rows through that kernel); M >= 192 "image_prefill+<fp16 route>"
 * (llmie_dequantize_mxfp4 into the workspace, then the fp16 GEMM), or "mxfp4_chunks" without a workspace that holds the image.
 * workspace: llmie_linear_workspace_bytes(LLMIE_W_MXFP4, M, K, N) bytes, 16-byte aligned (the fp16 image from 192 rows; 0 below).
 * No route NEEDS one, so the entry never returns LLMIE_ERR_WORKSPACE: from 192 rows a NULL or short workspace is not an error, the
 * call runs as "mxfp4_chunks" -- the slower route there, without a signal to the caller; llmie_linear_route tells which one runs.
 * K % 32 != 0, or x / wq not 16-byte aligned: LLMIE_ERR_UNSUPPORTED.  Scale rows carry no alignment beyond one byte.
 * Engine format: llmie_decoder_config.wfmt = LLMIE_W_MXFP4 (fp16 activations; int4_group ignored; llmie_matrix.scale = the e8m0
 * array; hidden size and inter_size multiples of 32).  Every decode batch runs the "unfused" sequence on the routes above (SwiGLU as
 * projection + llmie_silu_and_mul), dense, paged, ragged or e4m3 caches where the attention geometry has the fused kernel; a
 * hidden_out that is not 16-byte aligned is LLMIE_ERR_UNSUPPORTED.  Prefill runs the "general" sequence at every row count (in-place
 * norms, the plain QKV projection with the RoPE + append launch, gate/up as two launches).  Refused with LLMIE_ERR_UNSUPPORTED:
 * LLMIE_DEC_PACKED_ONLY (no packed image is built), llmie_decoder_lora_attach, and an MXFP4 LM head (lm_fmt) in the
 * llmie_lm_head_sample* entries. */
int llmie_quantize_mxfp4(const void *w, uint8_t *wq, uint8_t *scale, int N, int K, llmie_stream stream);
int llmie_dequantize_mxfp4(const uint8_t *wq, const uint8_t *scale, void *w16, int N, int K, llmie_stream stream);
int llmie_linear_mxfp4(const void *x, const uint8_t *wq, const uint8_t *scale, void *y, int M, int K, int N, const void *bias,
                       const void *residual, void *workspace, size_t workspace_bytes, llmie_stream stream);

/* Tile-packed weight images for decode batches (no reference counterpart: the reference streams row-major weights through
 * cuBLAS, src/kernels/linear.cu:10-87).  An MFMA operand wants 16 different weight rows across the lanes of one load, a
 * DRAM stream wants one contiguous KiB per wave instruction; the packed image gives both: tile = 16 rows, block = KB
 * consecutive k of the tile = 1 KiB in MFMA fragment order (KB = 32 fp16, 64 int8 / e4m3, 128 int4); K % KB == 0, rows
 * past N are zero.  swiglu_pairs != 0: w is a fused gate_up matrix [2I, K], packed tile 2p = gate rows [16p, 16p+16),
 * tile 2p+1 = the matching up rows.  int4: the group-128 scales are re-laid [tile][block][16] fp16 into packed_scale
 * (llmie_packed_scale_bytes; 0 for the other formats, which keep their per-row scale vector as it is).
 * llmie_linear_packed: y[M, N] (or [M, N/2] for swiglu != 0) = [swiglu]( rmsnorm(x + pre_bias) * gamma . W^T ) (+ residual),
 * 1 <= M <= 32 fp16 rows; gamma == NULL: no norm.  x is read once per workgroup into registers (8 waves split K), the
 * weights stream through a per-wave LDS-DMA ring.  workspace: llmie_linear_packed_workspace_bytes() bytes (non-zero only where K
 * exceeds the register-resident slice, e.g. the 7B down projection: fp32 split-K slabs + one reduce launch).
 */
size_t llmie_packed_weight_bytes(llmie_weight_format fmt, int N, int K, int swiglu_pairs);
size_t llmie_packed_scale_bytes(llmie_weight_format fmt, int N, int K, int swiglu_pairs);
int llmie_pack_weight(llmie_weight_format fmt, const void *w, const void *scale, void *packed, void *packed_scale,
                      int N, int K, int swiglu_pairs, llmie_stream stream);
size_t llmie_linear_packed_workspace_bytes(llmie_weight_format fmt, int M, int K, int N);
/* x32_flags: which operands are in the fragment-ordered activation layout "x32" instead of row-major (LLMIE_X32_X = x,
 * LLMIE_X32_Y = y, LLMIE_X32_RES = residual): a [<= 32 rows, C] fp16 matrix, C % 32 == 0, stored
 * [C / 32][2 row tiles][64 lanes][8 halves], lane = 16 * ((c % 32) / 8) + (m % 16), i.e. element (m, c) at half offset
 * ((c / 32) * 2 + m / 16) * 512 + ((c % 32) / 8) * 128 + (m % 16) * 8 + c % 8; always 32 rows of storage
 * (llmie_x32_bytes(C) = 64 C bytes).  Each (32 columns, 16 rows) piece is the 1 KiB MFMA operand of the consumer, so a
 * kernel chain that keeps its activations in x32 loads them with contiguous KiB reads and no transposition;
 * llmie_x32_convert moves a matrix between the two layouts (to_x32 != 0: rows >= M are zero-filled). */
enum { LLMIE_X32_X = 1, LLMIE_X32_Y = 2, LLMIE_X32_RES = 4 };
size_t llmie_x32_bytes(int C);
int llmie_x32_convert(const void *src, void *dst, int M, int C, int to_x32, llmie_stream stream);
int llmie_linear_packed(llmie_weight_format fmt, const void *x, const void *packed, const void *scale, void *y,
                        int M, int K, int N, int swiglu, int x32_flags, const void *residual, const void *gamma,
                        const void *pre_bias, float eps, void *workspace, size_t workspace_bytes,
                        llmie_stream stream);

/* ------------------------------------------------------------------------- */
/* 3. fused decoder engine (what LlamaSelfDecoder<T>::forward and             */
/*    LlamaModel<T>::generateNextToken run on; src/layers/self_decoder.cpp:24-122, */
/*    src/models/llama/llama.cpp:219-318)                                     */
/* ------------------------------------------------------------------------- */

typedef enum { LLMIE_KV_NATIVE = 0, LLMIE_KV_FP8 = 1 } llmie_kv_format;

typedef struct {
    const void *data;      /* [N,K] in the format's storage */
    const void *scale;     /* NULL for F16/F32 */
    const void *bias;      /* nullable, [N], activation dtype */
} llmie_matrix;

typedef struct {
    const void *attn_norm_gamma;   /* [H] */
    llmie_matrix qkv;              /* N=(nh+2kvh)*hs, K=H   (self_attn.qkv, layer_weights.cpp:28-31) */
    llmie_matrix o;                /* N=H, K=H                                                     */
    const void *ffn_norm_gamma;    /* [H] */
    llmie_matrix gate_up;          /* N=2I, K=H  rows [0,I)=gate, [I,2I)=up (layer_weights.cpp:41-44) */
    llmie_matrix down;             /* N=H, K=I */
} llmie_layer_weights;

typedef struct {
    int head_num, kv_head_num, head_size, inter_size, num_layers, vocab_size;
    int max_seq_len, max_batch;
    int rotary_dim;
    float rotary_base, rms_eps;
    llmie_dtype dtype;             /* activation / KV dtype */
    llmie_weight_format wfmt;      /* storage of the 4 big matrices per layer */
    int int4_group;                /* group size for LLMIE_W_INT4 */
    /* KV-cache storage (the reference stores T): LLMIE_KV_NATIVE = dtype, LLMIE_KV_FP8 = e4m3 bytes with one
     * static scale per cache, stored = e4m3(x / scale), same [L, batch, kvh, max_seq, hs] indexing (fp16 engines,
     * head_size 64/128 decode, 128 prefill, head_num/kv_head_num in {1,2,4}); a scale <= 0 means 1. */
    llmie_kv_format kv_fmt;
    float k_scale, v_scale;
    /* ABI 3: LLMIE_DEC_* bits (0 = the round-2 behaviour) */
    int flags;
} llmie_decoder_config;

/* Weight residency (ABI 3).  An engine whose max_batch lies above the GEMV range (gemv_max_batch in csrc/engine.hip is the one table:
 * fp16 5, int8 / fp8 / int4 2 rows when this was written; ask llmie_decoder_plan_name) builds
 * tile-packed images of its four matrices per layer inside its workspace at create time -- a SNAPSHOT: weights updated in place
 * afterwards are seen by the batch <= GEMV-range and prefill paths, not by the packed one; create synchronises the device before
 * it packs, so uploads on any stream have landed.  By default that image is a second copy next to the caller's row-major matrices.
 *   LLMIE_DEC_NO_PACKED_COPY  no image is built: batches above the GEMV range up to 32 take the split-K batch path on the row-major weights (slower there,
 *                             nothing doubled).
 *   LLMIE_DEC_PACKED_ONLY     the images are the ONLY weights the engine reads after create: the `data` arrays of the four
 *                             matrices of every layer may be freed or reused once llmie_decoder_create has returned (scales,
 *                             biases and norm gammas stay referenced).  Needs max_batch <= 32 (fp8: 16) and shapes the packed
 *                             kernels take; every decode batch runs on the packed kernels, prefill (fp16 / int8 / int4) unpacks
 *                             one matrix at a time into its workspace.  An int8 Llama-2-7B decoder is then resident at ~6.5 GB
 *                             instead of ~13 GB.
 * llmie_decoder_resident_weight_bytes: bytes of layer-matrix storage (row-major matrices that must stay + images) of a config. */
/* llmie_decoder_repack (ABI 3): the weights were updated in place, or -- for a packed-only engine -- are to be replaced: rebuild
 * the images from `layers` (row-major matrices in the engine's format; their scale / bias / gamma pointers replace the ones given
 * at create).  The pack kernels are enqueued on `stream`. */
#define LLMIE_DEC_NO_PACKED_COPY 1
#define LLMIE_DEC_PACKED_ONLY 2
size_t llmie_decoder_resident_weight_bytes(const llmie_decoder_config *cfg);

/* Which launch sequence an engine of this config runs (an addition within ABI 3; host only, no device access): the plan of
 * llmie_decoder_forward at `rows` sequences (prefill = 0: "gemv", "packed", "splitk" or "unfused"; LLMIE_CHAIN upgrades "packed" to
 * the chain launches where its probe of the built engine passes) or of llmie_decoder_prefill at `rows` tokens (prefill = 1:
 * "packed_only", "short_splitk", "lean" or "general").  call_flags describe the call, switch_mask stands in for the LLMIE_*
 * environment switches the entry points read.  NULL, with the reason in llmie_last_error(), where the call -- or creating the engine
 * -- is refused.  tests/golden/decoder_paths.txt pins the answers. */
#define LLMIE_PLAN_PAGED 1u              /* the *_paged entry points */
#define LLMIE_PLAN_RAGGED 2u             /* the *_ragged entry points */
#define LLMIE_PLAN_HIDDEN_MISALIGNED 4u  /* hidden_out not 16-byte aligned */
#define LLMIE_PLAN_WEIGHTS_MISALIGNED 8u /* a layer matrix not 16-byte aligned (decode: layer 0's QKV matrix) */
#define LLMIE_PLAN_GAMMAS_MISALIGNED 16u /* a norm gamma not 16-byte aligned */
#define LLMIE_PLAN_O_BIAS 32u            /* some layer has an output-projection bias */
#define LLMIE_PLAN_SCALES_MISALIGNED 64u /* an int4 group-scale array not 4-byte aligned */
#define LLMIE_SW_NO_FUSED_DECODE 1u
#define LLMIE_SW_NO_FUSED_BATCH 2u
#define LLMIE_SW_NO_PACKED_BATCH 4u
#define LLMIE_SW_CHAIN 8u
#define LLMIE_SW_NO_FUSED_SHORT_PREFILL 16u
#define LLMIE_SW_NO_QKV_ROPE_FUSION 32u
const char *llmie_decoder_plan_name(const llmie_decoder_config *cfg, int prefill, int rows, unsigned call_flags, unsigned switch_mask);

/* What ONE LAYER of llmie_decoder_prefill launches (an addition within ABI 3; host only, no device access), as one line of text:
 *   "lean token_table=1 attn_norm=oop qkv=rope_f16 pre=none rope_done=1 attn=q128w8t1 kv=f16 grid=16x16x1 rope_append=0 ffn_norm=oop
 *    gate_up=fused launches attn_norm=1 qkv_gemm=1 mha=1 o_gemm=1 ffn_norm=1 gate_up_swiglu=1 down_gemm=1"
 * the pass's sequence (llmie_decoder_plan_name) and whether it writes the token table of the fused QKV epilogue; the two norm forms
 * (none / inplace / oop / quant: emits e4m3 rows / rownorm: the split-K row kernel); the QKV form (plain, rope_f16 / rope_w8 /
 * rope_image / rope_unpacked / rope_e4m3: RoPE + the cache append in the projection's epilogue, plain_e4m3, unpack_plain, splitk,
 * splitk_rope) with the launch in front of it (dequant / unpack of the matrix's fp16 image) and the rope_done flag the attention
 * launch receives; the flash kernel's instantiation (query rows per workgroup, waves, row tiles per wave, cache format), its grid and
 * whether the RoPE + append launch runs in front; the gate/up form (fused, e4m3_swiglu, fp8_swiglu, two_launch, unpack_fused,
 * unpack_two_launch, splitk); and the launches per profiled op kind of one pass through the layer.  call_flags describe the pass
 * (LLMIE_PLAN_* above) and this layer's operands (below); switch_mask as above.  NULL where llmie_decoder_prefill -- or creating the
 * engine -- refuses: llmie_last_error() says why and *status (nullable) receives the code.  tests/golden/prefill_layer_plans.txt pins
 * the answers. */
#define LLMIE_PLAN_QKV_BIAS_MISALIGNED 128u       /* the layer's QKV bias not 8-byte aligned */
#define LLMIE_PLAN_GATE_UP_SCALES_MISALIGNED 256u /* the layer's gate/up scales not 16-byte aligned */
#define LLMIE_PLAN_NO_FFN_GAMMA 512u              /* the layer has no FFN norm gamma */
const char *llmie_decoder_prefill_layer_plan(const llmie_decoder_config *cfg, int tokens, int batch, int max_q_len, unsigned call_flags,
                                             unsigned switch_mask, int *status);

typedef struct llmie_decoder llmie_decoder; /* opaque */

/* Workspace is caller-owned device memory (no allocation inside). */
size_t llmie_decoder_workspace_bytes(const llmie_decoder_config *cfg);
/* layers[num_layers] is copied (pointers only). Returns NULL on invalid config. */
llmie_decoder *llmie_decoder_create(const llmie_decoder_config *cfg,
                                    const llmie_layer_weights *layers,
                                    void *workspace, size_t workspace_bytes);
void llmie_decoder_destroy(llmie_decoder *dec);
int llmie_decoder_repack(llmie_decoder *dec, const llmie_layer_weights *layers, llmie_stream stream);   /* see LLMIE_DEC_* above */

/* One decode step through all layers, in place semantics of LlamaSelfDecoder::forward:
 * hidden_in[bs,H] -> hidden_out[bs,H] (may alias).  Caches [L, batch, kvh, max_seq, hs].
 * step = context length INCLUDING the new token (reference `step`); if step_dev != NULL it is
 * read on the device (one int shared by the batch) so a captured graph can be replayed. */
int llmie_decoder_forward(llmie_decoder *dec, const void *hidden_in, void *hidden_out,
                          void *k_cache, void *v_cache, int batch, int step,
                          const int32_t *step_dev, llmie_stream stream);

/* Paged KV cache (the reference only has the dense slab): K and V live in pools of 128-token pages
 * [L, num_pages, kvh, LLMIE_KV_PAGE_TOKENS, hs] (element type = the engine's kv_fmt) and block_table[b * max_pages + p]
 * (device int32) names the pool page holding tokens [128 p, 128 p + 128) of sequence b.  Same arithmetic as
 * llmie_decoder_forward (bit-identical outputs for the same cache contents); fused decode paths only.
 * llmie_decoder_prefill_paged is llmie_decoder_prefill writing / reading the pages directly.
 * llmie_kv_pages_copy moves the first ctx_len[b] tokens of every sequence between a dense cache
 * [L, batch, kvh, max_seq, hs] and the pools (to_pages != 0: dense -> pages, e.g. after llmie_decoder_prefill). */
#define LLMIE_KV_PAGE_TOKENS 128
int llmie_decoder_forward_paged(llmie_decoder *dec, const void *hidden_in, void *hidden_out, void *k_pool, void *v_pool,
                                const int32_t *block_table, int max_pages, int num_pages, int batch, int step,
                                const int32_t *step_dev, llmie_stream stream);
/* Ragged batch (continuous batching; the reference steps a whole batch at ONE position, self_decoder.cpp:69-119): sequence b
 * is at context length ctx_len_dev[b] (device int32 [batch], including this step's token).  Only the attention launch differs
 * (RoPE position, append slot, span per sequence); row b is what llmie_decoder_forward at step ctx_len[b] gives that row. */
int llmie_decoder_forward_ragged(llmie_decoder *dec, const void *hidden_in, void *hidden_out, void *k_cache, void *v_cache,
                                 int batch, const int32_t *ctx_len_dev, llmie_stream stream);
int llmie_decoder_forward_paged_ragged(llmie_decoder *dec, const void *hidden_in, void *hidden_out, void *k_pool, void *v_pool,
                                       const int32_t *block_table, int max_pages, int num_pages, int batch,
                                       const int32_t *ctx_len_dev, llmie_stream stream);
int llmie_decoder_prefill_paged(llmie_decoder *dec, const void *hidden_in, void *hidden_out, void *k_pool, void *v_pool,
                                const int32_t *block_table, int max_pages, int num_pages, const int32_t *input_lengths,
                                const int32_t *history_lengths, int batch, int num_tokens, int max_q_len, void *workspace,
                                size_t workspace_bytes, llmie_stream stream);
int llmie_kv_pages_copy(void *dense, void *pool, const int32_t *block_table, const int32_t *ctx_len, int to_pages,
                        int layers, int batch, int kv_head_num, int max_seq_len, int head_size, int max_pages,
                        int num_pages, int elem_bytes, llmie_stream stream);

/* ABI 3 (an addition).  Several hypotheses per request: beam search, or n samples that share one prefilled prompt.  No reference
 * launcher (the reference carries a beamwidth dimension and `launchTopKForBeamSearch` by name only).
 *
 * llmie_beam_step: from the logits [groups * width, vocab] of a step, the next `width` hypotheses of every request.  Beam w of
 * group g is row r = g * width + w, in one of three states:
 *   dead      cum_logprob is -INFINITY or NaN: contributes nothing;
 *   finished  (and not dead): contributes the one candidate (w, end_id, score = cum[w], len = gen_len[w]) -- it stays frozen
 *             and keeps competing; its logits are not read;
 *   live      lse = log-sum-exp of the row's non-NaN logits (fp32, running maximum); the row contributes its min(width, valid)
 *             best tokens in llmie_topk's order on the raw logits (value descending, ties to the lower id, -0 == +0, NaN
 *             excluded), each as (w, v, score = cum[w] + (logit[v] - lse), len = gen_len[w] + 1): one fp32 subtract, then one
 *             fp32 add.  A score that comes out NaN (a +INFINITY logit, a row of -INFINITY) is no candidate.
 * Candidates of a group are ordered by key descending, ties to the lower w, then to the earlier rank inside the row;
 * key = score when length_penalty == 0 (bit exact, no powf), else score / powf((float)len, length_penalty) (a NaN key, 0 / 0 at
 * len 0, ranks as -INFINITY).  The first `width` candidates fill slots 0..width-1 in that order: out_parent[g, j] = g * width + w
 * (the ABSOLUTE row), out_token = v, cum_logprob = score, gen_len = len, finished = parent was finished || v == end_id.  Slots
 * past the candidate count become dead: out_parent = the slot's own row (llmie_kv_pages_fork leaves it alone), out_token =
 * end_id, cum = -INFINITY, gen_len = 0, finished = 1.  The state is updated in place; all of a group's reads happen before any
 * of its writes.  A request starts with cum = [0, -INFINITY, ...] so that its identical first-step rows yield no duplicates.
 * Same inputs, same bits; a group's outputs depend neither on its slot nor on the other groups; no float atomics.
 * LLMIE_ERR_INVALID_ARG: NULL pointers, non-positive sizes, NaN length_penalty.  LLMIE_ERR_UNSUPPORTED: width >
 * LLMIE_BEAM_MAX_WIDTH.  LLMIE_ERR_WORKSPACE: NULL, short or not 4-byte aligned.  LLMIE_ERR_UNSUPPORTED: an unknown dtype.
 * Two launches, no allocation, no synchronisation, legal inside a graph capture: every operand is read on the device. */
#define LLMIE_BEAM_MAX_WIDTH 16
size_t llmie_beam_step_workspace_bytes(int groups, int width, int vocab);
int llmie_beam_step(const void *logits /* [groups*width, vocab], dtype */, int groups, int width, int vocab,
                    float *cum_logprob /* [groups, width] in/out */, int32_t *gen_len /* [groups, width] in/out */,
                    uint8_t *finished /* [groups, width] in/out */, int32_t *out_parent /* [groups, width] */,
                    int32_t *out_token /* [groups, width] */, int end_id, float length_penalty, void *workspace,
                    size_t workspace_bytes, llmie_dtype dtype, llmie_stream stream);

/* ABI 3 (an addition).  llmie_kv_pages_fork: row j of a paged cache continues the sequence of row parent[j] (copy on fork).
 * Pools [L, num_pages, kvh, 128, hs] and block_table [rows, max_pages] as llmie_decoder_forward_paged takes them; own_table
 * [rows, max_pages] names the pages row j may write; cached_len [rows] is the number of tokens in the cache of each row.  "Old"
 * is a value as it was before the call.  With q = parent[j], n = old cached_len[q], pc = n / 128, r = n % 128, row j is left
 * entirely untouched if q == j, q lies outside [0, rows), n lies outside [0, 128 * max_pages], or -- r > 0 -- the page it would
 * read (old block_table[q][pc]) or write (own_table[j][pc]) lies outside [0, num_pages).  Otherwise cached_len[j] = n;
 * block_table[j][p] = old block_table[q][p] for p < pc (completed pages are shared, nothing is copied) and own_table[j][p] for
 * p >= pc; and if r > 0 the first r token rows of page old block_table[q][pc] are copied bit-exactly into page own_table[j][pc],
 * for every layer and KV head, in both pools -- exactly those rows are written and nothing else in either pool.  Every read is of
 * the old state whatever `parent` is (a swap, a rotation: source tails are destination tails of other rows): one launch gathers
 * tails, table rows and lengths into the workspace, a second scatters them.  16 bytes per lane where the addresses allow it, plain
 * bytes otherwise; any elem_bytes (fp16 and e4m3 caches are both just bytes).
 * Caller contract: own_table names a distinct page per (row, page index); a row's pages at indices >= cached_len / 128 are its
 * own; the context lengths in a family of forks never shrink -- a row's own page at index p is shared only once it is complete,
 * such a page is never handed out again, and a caller that forks to a shorter context supplies fresh pages.
 * LLMIE_ERR_INVALID_ARG: NULL pointers, non-positive sizes.  LLMIE_ERR_UNSUPPORTED: kv_head_num or layers above 65535, rows above
 * 32767.  LLMIE_ERR_WORKSPACE: NULL, short or not 16-byte aligned.  No allocation, no synchronisation, legal inside a capture. */
size_t llmie_kv_pages_fork_workspace_bytes(int rows, int layers, int kv_head_num, int head_size, int elem_bytes, int max_pages);
int llmie_kv_pages_fork(void *k_pool, void *v_pool, int32_t *block_table /* [rows, max_pages] in/out */,
                        const int32_t *own_table /* [rows, max_pages] */, const int32_t *parent /* [rows]: absolute row */,
                        int32_t *cached_len /* [rows] in/out */, int rows, int layers, int kv_head_num, int head_size,
                        int max_pages, int num_pages, int elem_bytes, void *workspace, size_t workspace_bytes,
                        llmie_stream stream);

/* ABI 3 (an addition).  Speculative decoding behind the logits.  No reference launcher.  The forward over a chunk of k + 1
 * inputs per sequence is llmie_decoder_prefill(_paged) on top of the cached history; these two entries are what follows the
 * logits, and a drafter that needs no second model.  (Rejection sampling against a sampled draft model: llmie_spec_verify_sampled,
 * below.)
 *
 * llmie_spec_verify: EXACT-MATCH verification.  logits [batch * (k + 1), vocab]: row r = b * (k + 1) + i holds the logits that
 * follow input i of sequence b; input 0 is the last emitted token, input i >= 1 is draft_ids[b, i - 1].  s_b, the Philox step of
 * sequence b, is step_rows[b] if step_rows != NULL, else *step_dev if step_dev != NULL, else `step`.  For a sequence with
 * finished[b] == 0 on entry, pick_i is the token llmie_sample_logits_ext returns for row (b, i) alone at step s_b + i, with
 * the parameters of b, the ext arrays of b, and the history of b as i preceding calls would have left it: history_append != 0:
 * the old history followed by pick_0 .. pick_{i-1} as far as history_stride lets them be appended; history_append == 0: the
 * history unchanged.  (The sampler is deterministic -- Philox keyed by (step, seed), fixed-point masses -- so pick_i is THE
 * token plain decoding would have emitted.)  Emission walks i = 0, 1, ...: emit pick_i; stop behind it if i == draft_len[b]
 * (draft_len == NULL: k; clamped to [0, k]), if pick_i != draft_ids[b, i], or if pick_i finishes the sequence (end_id or one of
 * the row's stop ids: step 8 of llmie_sample_logits_ext); otherwise go on.  count, in [1, k + 1], is the number of emitted tokens:
 * bit for bit what `count` successive llmie_sample_logits_ext calls emit from these rows, for greedy and for every control.
 *   out_tokens[b, 0..count) the emitted tokens, later slots -1;  out_count[b] = count;
 *   out_logprob[b, i] (may be NULL) the raw log-softmax of emitted token i as the sampler's out_logprob, later slots -INFINITY;
 *   seq_len, finished, history, history_len: exactly as behind those `count` sequential calls;
 *   last_token[b] (may be NULL) = out_tokens[b, count - 1];  cached_len[b] (may be NULL) += count: input 0 and the accepted
 *   drafts are now valid cache rows;  step_rows[b] (may be NULL) += count.
 * A sequence with finished[b] != 0 on entry is left alone -- out_count = 0, out_tokens all -1, out_logprob all -INFINITY, no state
 * changes -- the one deliberate departure from the plain sampler, which samples finished rows again.
 * ext (may be NULL): per-request arrays are indexed by b (bias, stops, min_step -- compared with s_b + i -- and the mask row
 * when mask_index == NULL); mask_index, if given, is [batch * (k + 1)], indexed by r (a grammar has one mask per position);
 * out_top_ids / out_top_logprobs are [batch * (k + 1), top_n], indexed by r, and written for EVERY row, rejected positions and
 * finished sequences included: they are a property of the raw logits.
 * Refused on the host before any launch: first whatever llmie_sample_logits_ext refuses (out_tokens in the place of out_id),
 * then LLMIE_ERR_INVALID_ARG: k < 1, NULL draft_ids / out_tokens / out_count; LLMIE_ERR_UNSUPPORTED: k > LLMIE_SPEC_MAX_DRAFT;
 * LLMIE_ERR_WORKSPACE: NULL, short (llmie_spec_verify_workspace_bytes; 0 for non-positive or unsupported sizes) or not 16-byte
 * aligned.
 * Two launches (one 1024-thread workgroup per row runs the sampler's body on a history view that splices draft_ids[b, 0..i)
 * behind the stored history -- whenever position i matters the earlier picks equal the earlier drafts, so the positions of a
 * sequence run side by side; then one pass per sequence walks the picks).  No allocation, no synchronisation, legal inside a
 * graph capture: every operand is read on the device.  No float atomics; same inputs, same bits; a sequence's outputs depend
 * neither on its slot nor on the other sequences. */
#define LLMIE_SPEC_MAX_DRAFT 15
size_t llmie_spec_verify_workspace_bytes(int batch, int k, int vocab);
int llmie_spec_verify(const void *logits /* [batch*(k+1), vocab], row r = b*(k+1)+i */, int batch, int k, int vocab,
                      const int32_t *draft_ids /* [batch, k] */, const int32_t *draft_len /* [batch], NULL = k; clamped to [0,k] */,
                      const llmie_sampling_params *params_dev /* [batch] */, int32_t *history, int history_stride,
                      int32_t *history_len, int history_append, int32_t *seq_len, uint8_t *finished,
                      int32_t *out_tokens /* [batch, k+1] */, int32_t *out_count /* [batch] */, float *out_logprob /* [batch,k+1], nullable */,
                      int32_t *last_token /* [batch], nullable */, int32_t *cached_len /* [batch], nullable, in/out */,
                      int32_t *step_rows /* [batch], nullable, in/out */, int step, const int32_t *step_dev, int end_id,
                      void *workspace, size_t workspace_bytes, llmie_dtype dtype, llmie_stream stream,
                      const llmie_sampling_ext *ext /* nullable */);

/* ABI 3 (an addition).  llmie_spec_verify_sampled: REJECTION-SAMPLING verification against a drafter that SAMPLED its drafts (a
 * small model at temperature > 0).  Exact match accepts such a draft with probability p(d); the rule below accepts with
 * probability min(1, p(d) / q(d)) and, behind a rejection, draws from the residual max(0, p - q): the emitted tokens are
 * distributed as plain sampling from the target, whatever the drafter's distribution.
 * Operands are those of llmie_spec_verify, plus draft_logits [batch, k, vocab] (same dtype as logits; row (b, i) holds the draft
 * model's logits from which draft i of sequence b was sampled), draft_params_dev [batch] (the controls the drafter sampled with)
 * and out_accepted [batch] (may be NULL: the number of drafts among the emitted tokens).
 * CALLER CONTRACT: the drafter sampled draft_ids[b, i] with llmie_sample_logits from draft_logits[b, i], draft_params_dev[b] and
 * the history view of position i below (no extension).  Its seed should differ from params_dev[b].seed, or the drafter's draw and
 * this entry's draws of lane 0 coincide.
 * Position i of sequence b is row r = b * (k + 1) + i; its Philox step is s_b + i (s_b as in llmie_spec_verify) and its history is
 * the spliced view of llmie_spec_verify: the stored history followed by draft_ids[b, 0..i) as far as i appends reach.
 *   Target masses.  P_v is the sampler's fixed-point mass of token v in row r for params_dev[b] and ext: floor(expf(l_v - max) *
 *   2^32) as a 64-bit integer over the tokens llmie_sample_logits_ext keeps (behind bias, mask, stops and min_step, penalties,
 *   temperature, top-k, top-p, min-p), 0 for every other token; S_P = sum_v P_v.  A greedy row, or one with at most one valid token,
 *   is the point mass P = S_P = 1 on the sampler's pick; a row without a valid token has P = 0 everywhere and S_P = 0.
 *   Draft masses.  Q_v, S_Q: the same construction on draft_logits[b, i] with draft_params_dev[b], the same history view and no
 *   extension -- the distribution llmie_sample_logits draws from.  A greedy draft is a point mass.
 *   Draws.  U(lane) = (c0 >> 8) + 1 in [1, 2^24], c0 the first word of Philox4x32-10 with key (s_b + i, 0x4c4c4d49) on the counter
 *   (params_dev[b].seed, lane, 0, 0).  Lane 0 is the sampler's own draw (u = U / 2^24), lane 1 the accept draw, lane 2 the residual
 *   draw.
 *   Accept.  With d = draft_ids[b, i], draft i is accepted iff 0 <= d < vocab and (U(1) - 1) * Q_d * S_P < 2^24 * P_d * S_Q, an
 *   exact comparison of 128-bit integers (no division, no rounding): P_d / S_P >= Q_d / S_Q always accepts, P_d == 0 never does,
 *   Q_d == 0 < P_d does.
 *   Residual.  R_v = max(0, P_v * S_Q - Q_v * S_P), SR = sum_v R_v, thr = ((U(2) - 1) * SR) >> 24, all in 128-bit integers; the
 *   residual token is the first id, ascending, at which the running sum of R exceeds thr.  If SR == 0 -- a point-mass or degenerate
 *   input only, S_Q == 0 included; SR > 0 wherever a non-degenerate rejection is possible -- it is the sampler's own pick of the row.
 * Emission walks i = 0, 1, ... with m = draft_len[b] clamped to [0, k] (NULL: k).  For i < m: if draft i is accepted emit it and
 * go on, unless it finishes the sequence (end_id or one of the row's stop ids); otherwise emit the residual token and stop.  At
 * i == m emit the sampler's own pick of row m (the lane-0 draw: the bonus token) and stop.  A position without a valid token is
 * always rejected and emits end_id (finished), as the sampler does.  out_tokens, out_count, out_logprob (the raw log-softmax of the
 * emitted token on the TARGET row), seq_len, finished, the history append, last_token, cached_len and step_rows follow count exactly
 * as in llmie_spec_verify; a sequence finished on entry is left alone, and ext's top-N outputs are written for every row, as there.
 * Guarantees: same inputs, same bits (integer sums, a scan in a fixed order, no float atomics); a sequence's outputs depend neither
 * on its slot nor on the other sequences; with a greedy target the emitted tokens are those of plain greedy decoding whatever the
 * drafter did; with draft_logits and draft_params_dev bit-equal to the target's rows and parameters and no ext, every draft is
 * accepted (P == Q turns the comparison into U(1) - 1 < 2^24).
 * Refused on the host before any launch: whatever llmie_spec_verify refuses, in its order, under this entry's name;
 * LLMIE_ERR_INVALID_ARG: NULL draft_logits / draft_params_dev; LLMIE_ERR_UNSUPPORTED: vocab > 2^19 (S_P, S_Q < 2^51 keep both sides
 * of the comparison below 2^107 and (U - 1) * SR inside 128 bits); LLMIE_ERR_WORKSPACE: NULL, short
 * (llmie_spec_verify_sampled_workspace_bytes: two key rows per position; 0 for non-positive or unsupported sizes) or not 16-byte
 * aligned.  Two launches (one 1024-thread workgroup per row prepares the target and the draft row, decides and leaves a fixed-size
 * record; one pass per sequence walks the records).  No allocation, no synchronisation, legal inside a graph capture: every
 * operand is read on the device. */
size_t llmie_spec_verify_sampled_workspace_bytes(int batch, int k, int vocab);
int llmie_spec_verify_sampled(const void *logits /* [batch*(k+1), vocab], row r = b*(k+1)+i */,
                              const void *draft_logits /* [batch, k, vocab], dtype */, int batch, int k, int vocab,
                              const int32_t *draft_ids /* [batch, k] */, const int32_t *draft_len /* [batch], NULL = k; clamped to [0,k] */,
                              const llmie_sampling_params *params_dev /* [batch] */,
                              const llmie_sampling_params *draft_params_dev /* [batch] */, int32_t *history, int history_stride,
                              int32_t *history_len, int history_append, int32_t *seq_len, uint8_t *finished,
                              int32_t *out_tokens /* [batch, k+1] */, int32_t *out_count /* [batch] */,
                              int32_t *out_accepted /* [batch], nullable */, float *out_logprob /* [batch,k+1], nullable */,
                              int32_t *last_token /* [batch], nullable */, int32_t *cached_len /* [batch], nullable, in/out */,
                              int32_t *step_rows /* [batch], nullable, in/out */, int step, const int32_t *step_dev, int end_id,
                              void *workspace, size_t workspace_bytes, llmie_dtype dtype, llmie_stream stream,
                              const llmie_sampling_ext *ext /* nullable */);

/* ABI 3 (an addition).  llmie_ngram_draft: prompt-lookup drafting.  tokens [batch, stride] holds each sequence's tokens so far
 * (prompt included), len [batch] their count; they may be the sampler's history / history_len when the caller put the prompt
 * there.  Per sequence, L = len[b] clamped to [0, stride].  out_ids[b, 0] = tokens[b, L - 1] (pad_id when L == 0): the last
 * emitted token, input 0 of the verify chunk.  No drafts (out_draft_len[b] = 0) when finished != NULL and finished[b] != 0, or
 * L < min_n + 1.  Otherwise, for n = min(max_n, L - 1) down to min_n, with S = tokens[L - n .. L): a match is a start
 * p <= L - n - 1 with tokens[p .. p + n) == S; of the matches take the largest p with p + n + k <= L (a full continuation), if
 * there is none the largest p at all; the first n with a match wins.  m = min(k, L - p - n) and the drafts are
 * tokens[p + n .. p + n + m): out_draft_ids[b, 0..m), out_ids[b, 1..m], out_draft_len[b] = m.  Slots past m hold pad_id.
 * 1 <= min_n <= max_n <= 8 and 1 <= k <= LLMIE_SPEC_MAX_DRAFT (LLMIE_ERR_INVALID_ARG below, LLMIE_ERR_UNSUPPORTED above the
 * bounds); stride is any positive value.  One launch, one workgroup per sequence, one sweep over the row for every n at once
 * (16-byte loads where the row is 16-byte aligned); "the largest p" is an integer maximum: same inputs, same bits.  No
 * allocation, no synchronisation, legal inside a graph capture. */
int llmie_ngram_draft(const int32_t *tokens /* [batch, stride] */, int stride, const int32_t *len /* [batch] */,
                      const uint8_t *finished /* nullable */, int batch, int k, int max_n, int min_n, int pad_id,
                      int32_t *out_ids /* [batch, k+1]: the verify chunk's input ids */, int32_t *out_draft_ids /* [batch, k] */,
                      int32_t *out_draft_len /* [batch] */, llmie_stream stream);

/* ABI 3 (an addition).  TREE speculative decoding: several alternatives per position verified in one forward.  No reference launcher.
 * A sequence's chunk has n node slots, 1 <= n <= LLMIE_SPEC_TREE_MAX_NODES, the same stride for every sequence.  Node 0 is the last
 * emitted token (input 0 of the linear chunk); nodes 1 .. n - 1 are drafts; parent[b, i] names node i's parent.
 *
 * llmie_spec_tree_prepare: parent [batch, n] -> depth_out [batch, n] (int32), anc_out [batch, n] (uint64).  count =
 * node_count[b] clamped to [1, n] (node_count == NULL: n).  Node 0: depth 0, anc 1.  Node i >= 1 is LIVE iff i < count and
 * 0 <= parent[b, i] < i and the parent is live; a live node has depth = depth[parent] + 1 and anc = anc[parent] | (1 << i) -- bit j
 * of anc[i] says that node j lies on the path root -> i, i included; a dead node has depth 0 and anc = 1 << i.  So "live" is "bit 0
 * of anc is set", the one liveness rule every consumer uses.  One launch; everything is read on the device; legal inside a graph
 * capture.  LLMIE_ERR_INVALID_ARG: NULL parent / depth_out / anc_out, batch < 1, n < 1; LLMIE_ERR_UNSUPPORTED: n above the maximum.
 *
 * llmie_spec_verify_tree: EXACT-MATCH verification of a tree.  The operands are those of llmie_spec_verify with k -> n, draft_ids ->
 * node_ids [batch, n] (the token of each node; slot 0 is not read), draft_len -> parent, depth, anc [batch, n] as
 * llmie_spec_tree_prepare left them; out_tokens, out_logprob and out_path (may be NULL) are [batch, n]; logits are
 * [batch * n, vocab], row r = b * n + i follows node i; mask_index and the top-N outputs of ext are indexed by r.
 * pick_i is the token llmie_sample_logits_ext returns for row (b, i) alone at Philox step s_b + depth_i, on the history of b
 * followed -- history_append != 0, as far as history_stride lets depth_i appends reach -- by node_ids of the nodes on the path
 * root -> i, root excluded and i included, in depth order.  (A dead node samples at depth 0 on the stored history; nothing reads
 * its pick.)  The walk: cur = 0; emit pick_cur, out_path[b, m] = cur; stop if pick_cur finishes the sequence; otherwise take the
 * LOWEST live j with parent[b, j] == cur and node_ids[b, j] == pick_cur; none: stop; else cur = j and go on.  count is in [1, n];
 * later slots of out_path are -1; out_tokens, out_count, out_logprob, seq_len, finished, the history append, last_token,
 * cached_len += count, step_rows += count, a sequence finished on entry (left alone) and the top-N outputs (every row) are exactly
 * llmie_spec_verify's.  With parent[i] = i - 1, n = k + 1, node_ids[b, i] = draft_ids[b, i - 1] and node_count = draft_len + 1 every
 * output and every state array equals llmie_spec_verify's bit for bit.  Refused on the host before any launch: whatever
 * llmie_spec_verify refuses, in its order and under this entry's name, with n < 1 (LLMIE_ERR_INVALID_ARG), NULL node_ids /
 * out_tokens / out_count, NULL parent / depth / anc, n above the maximum (LLMIE_ERR_UNSUPPORTED) and the workspace rule on
 * llmie_spec_verify_tree_workspace_bytes in the places of the k checks.  Two launches (one 1024-thread workgroup per node: the path
 * tokens, at most 63, are gathered into LDS first; one pass per sequence walks the tree in LDS); no allocation, no
 * synchronisation, legal inside a graph capture; same inputs, same bits; no dependence on slot or neighbours.
 *
 * llmie_kv_tree_commit: behind the verify, accepted node out_path[b, m] sits at cache slot base_len[b] + out_path[b, m] and belongs
 * at base_len[b] + m (its K row already carries the right rotation: depth(out_path[m]) = m).  Moves the K and V rows of every
 * layer and kv head for m < out_count[b] (clamped to [0, n]); rows with out_path[m] == m stay; count 0 does nothing.  Dense caches
 * [layers, batch, kvh, max_seq_len, head_size] (block_table NULL) or pools [layers, num_pages, kvh, 128, head_size] through
 * block_table [batch, max_pages]; elem_bytes 2 (fp16) or 1 (e4m3).  A byte copy with the semantics "all sources read, then all
 * destinations written": a destination slot may be a later source, and source and destination may lie in different pages.  A row
 * whose source or destination lies outside the cache (or the table) is skipped.  base_len is the history_lengths array THE FORWARD
 * ran with: it must not be the array the verify advanced (cached_len) -- keep two arrays and copy cached -> base afterwards.
 * LLMIE_ERR_INVALID_ARG: NULL caches / base_len / out_path / out_count, non-positive sizes, n < 1, elem_bytes not 1 or 2, a block
 * table with max_pages < 1 or num_pages < 1, caches not 16-byte aligned; LLMIE_ERR_UNSUPPORTED: n above the maximum,
 * head_size * elem_bytes not a multiple of 16 or above 512.  One launch (one workgroup per (layer x kv head, sequence, K or V) stages
 * its rows in LDS, a barrier, then the stores); legal inside a graph capture.
 *
 * llmie_ngram_draft_tree: a tree drafter that needs no second model, on llmie_ngram_draft's operands.  L, "no drafts" (then
 * out_node_count[b] = 1) and the matches are those of llmie_ngram_draft.  Candidates: for n' = min(max_n, L - 1) down to min_n, every
 * n' that has a match contributes the continuation start llmie_ngram_draft would choose with max_n = n' (the largest start with k
 * tokens behind it, else the largest at all); the first `branches` DISTINCT starts are kept, 1 <= branches <= 8, each with
 * min(k, L - start) tokens, 1 <= k <= LLMIE_SPEC_MAX_DRAFT.  Trie merge, in that order: from the root, every token reuses the
 * lowest existing child of the current node that carries it, else appends a new node while fewer than n exist; a candidate is cut
 * where the budget ends.  Node order is creation order, so parent < child.  out_ids [batch, n]: node 0 the last token (pad_id when
 * L == 0), unused slots pad_id; out_parent [batch, n]: -1 for node 0 and unused slots; out_node_count [batch].  With branches = 1
 * the ids, the chain and node_count - 1 equal llmie_ngram_draft's outputs.  Bounds as llmie_ngram_draft's (LLMIE_ERR_INVALID_ARG
 * below, LLMIE_ERR_UNSUPPORTED above), with n in [1, LLMIE_SPEC_TREE_MAX_NODES].  One launch, legal inside a graph capture. */
#define LLMIE_SPEC_TREE_MAX_NODES 64
int llmie_ngram_draft_tree(const int32_t *tokens /* [batch, stride] */, int stride, const int32_t *len /* [batch] */,
                           const uint8_t *finished /* nullable */, int batch, int n, int k, int branches, int max_n, int min_n, int pad_id,
                           int32_t *out_ids /* [batch, n] */, int32_t *out_parent /* [batch, n] */, int32_t *out_node_count /* [batch] */,
                           llmie_stream stream);
int llmie_spec_tree_prepare(const int32_t *parent /* [batch, n] */, const int32_t *node_count /* [batch], NULL = n; clamped to [1,n] */,
                            int batch, int n, int32_t *depth_out /* [batch, n] */, uint64_t *anc_out /* [batch, n] */, llmie_stream stream);
size_t llmie_spec_verify_tree_workspace_bytes(int batch, int n, int vocab);
int llmie_spec_verify_tree(const void *logits /* [batch*n, vocab], row r = b*n+i */, int batch, int n, int vocab,
                           const int32_t *node_ids /* [batch, n] */, const int32_t *parent /* [batch, n] */,
                           const int32_t *depth /* [batch, n] */, const uint64_t *anc /* [batch, n] */,
                           const llmie_sampling_params *params_dev /* [batch] */, int32_t *history, int history_stride,
                           int32_t *history_len, int history_append, int32_t *seq_len, uint8_t *finished,
                           int32_t *out_tokens /* [batch, n] */, int32_t *out_count /* [batch] */, int32_t *out_path /* [batch, n], nullable */,
                           float *out_logprob /* [batch, n], nullable */, int32_t *last_token /* [batch], nullable */,
                           int32_t *cached_len /* [batch], nullable, in/out */, int32_t *step_rows /* [batch], nullable, in/out */, int step,
                           const int32_t *step_dev, int end_id, void *workspace, size_t workspace_bytes, llmie_dtype dtype,
                           llmie_stream stream, const llmie_sampling_ext *ext /* nullable */);
int llmie_kv_tree_commit(void *k_cache, void *v_cache, const int32_t *block_table /* [batch, max_pages] or NULL: dense */,
                         const int32_t *base_len /* [batch]: the forward's history_lengths */, const int32_t *out_path /* [batch, n] */,
                         const int32_t *out_count /* [batch] */, int batch, int n, int layers, int kv_head_num, int max_seq_len,
                         int head_size, int max_pages, int num_pages, int elem_bytes, llmie_stream stream);

/* ABI 3 (an addition).  Multi-LoRA: per-row adapters on top of a projection.  No reference launcher.
 *
 * For a projection y = x . W^T (W is [N, K]; x [rows, K], y [rows, N], fp16, row-major), row m carrying adapter slot s = slot[m] gets
 *   y[m, n] = fp16( float(y[m, n]) + scale_s * sum_r B_s[n, r] * t[m, j(n) * rank_s + r] ),   t[m, :] = x[m, :] . A_s^T
 * A_s is [blocks * rank_s, K] and B_s is [N, rank_s], both fp16, row-major, 16-byte aligned.  The output columns are cut into
 * `blocks` (1..3) column blocks of host-given widths (QKV: q / k / v; gate_up: gate / up; o and down: one) and j(n) is the block of
 * column n; block j uses rows [j * rank, (j + 1) * rank) of A -- PEFT's separate q_proj / k_proj / v_proj (gate_proj / up_proj)
 * adapters stacked onto the fused matrices.  A module whose A / B pointer pair is NULL contributes nothing.  Every sum is fp32; t
 * is summed over K in fp32 (the K slices in a fixed order) and rounded to fp16 ONCE, as the operand of the second product; scale is
 * applied to the fp32 sum before the update.  rank_s in {8, 16, 32, 64}; slots of different rank may meet in one call.
 * A row is left bit for bit as it was when its slot is -1, lies outside [0, slots), or names a slot of rank 0 (an empty slot).
 * fp16 activations only (LLMIE_F32: LLMIE_ERR_UNSUPPORTED).  No atomics on results; the K split is a host function of K alone; a
 * row belongs to exactly one tile of <= 16 rows of one slot and every row of a tile is computed on its own: same inputs, same
 * bits, and a row's bits depend neither on its position nor on which other rows or slots share the call.
 *
 * Everything that may change between steps lives in DEVICE memory read at launch: the slot table (per slot its rank and scale, per
 * layer and module the A / B pointers) and the per-row or per-sequence slot array.  A captured step serves a new adapter mix, or a
 * slot reloaded with another adapter, on replay.
 *   llmie_lora_table_bytes(slots, layers) = slots * (16 + 64 * layers): [slots] x {int32 rank, float scale, 8 bytes of padding},
 *     then [slots][layers][4 modules][2] device pointers (A, B).  A table of zero bytes is a table of empty slots.  0 for
 *     non-positive sizes or slots > LLMIE_LORA_MAX_SLOTS.
 *   llmie_lora_slot_load writes one slot from a HOST description (NULL: empties the slot).  Enqueued on `stream` as kernel launches
 *     whose arguments carry the values (no host buffer has to outlive the call); not meant for a captured region.
 *   llmie_lora_workspace_bytes(max_rows, slots, max_rank_total), with tiles = max_rows / 16 + min(slots, max_rows) and every term
 *     rounded up to 256 bytes: 256 (the plan's header) + 4 * max_rows (the slot of every row) + 4 * tiles (the slot of every tile) +
 *     64 * tiles (16 row indices per tile, -1 = padding) + LLMIE_LORA_MAX_KSPLIT * tiles * 16 * max_rank_total * 4 (the fp32
 *     partials of t).  max_rank_total: the largest blocks * 64 of any llmie_lora_apply call on the workspace (192 covers QKV).
 *   llmie_lora_plan, ONE launch per forward call: groups the rows of each slot, in row order, into tiles of <= 16 rows and leaves
 *     the plan in the workspace.  lengths == NULL: slot is [rows]; else slot is [batch] and row t takes the slot of the sequence it
 *     belongs to when the sequences lie back to back with lengths[b] rows each (rows behind their sum: -1).  Nothing is read back:
 *     every later grid is sized to the bound `tiles` and surplus tiles exit at once.
 *   llmie_lora_apply, TWO launches: shrink (grid tiles x K slices: fp32 partials of t by v_mfma_f32_16x16x32_f16, both operand
 *     fragments 16-byte loads from global memory, an A matrix read once per tile) and expand (grid tiles x groups of 256 columns:
 *     sums the K slices, the transposed product B . t^T so that a lane owns 4 consecutive columns of one row, scale, 8-byte
 *     read-modify-write of y).  Reads the plan the last llmie_lora_plan left in `workspace` for the same rows and slots (a
 *     workspace whose plan is of another shape: the launches do nothing).
 * Refused on the host before any launch.  LLMIE_ERR_INVALID_ARG: NULL pointers; non-positive sizes; a slot, layer or module outside
 * its range; a rank outside {8, 16, 32, 64}; an A without its B; fewer than 1 or more than 3 blocks; block widths not summing to N.
 * LLMIE_ERR_UNSUPPORTED: LLMIE_F32; K % 32 != 0; a block width that is not a multiple of 16; x, y, A or B not 16-byte aligned;
 * slots > LLMIE_LORA_MAX_SLOTS.  LLMIE_ERR_WORKSPACE: NULL, short or not 256-byte aligned.  No launch allocates or synchronises. */
#define LLMIE_LORA_MAX_SLOTS 1024
#define LLMIE_LORA_MAX_KSPLIT 8
#define LLMIE_LORA_QKV 0
#define LLMIE_LORA_O 1
#define LLMIE_LORA_GATE_UP 2
#define LLMIE_LORA_DOWN 3
typedef struct {
    const void *a[4]; /* per module (LLMIE_LORA_*): A [blocks * rank, K], device, fp16; NULL = the adapter lacks the module */
    const void *b[4]; /* per module: B [N, rank], device, fp16 */
} llmie_lora_layer;
typedef struct { /* host struct */
    int rank;    /* 8, 16, 32 or 64 */
    float scale; /* lora_alpha / rank */
    int layers;  /* entries of `layer`: the table's layer count */
    const llmie_lora_layer *layer;
} llmie_lora_adapter;
size_t llmie_lora_table_bytes(int slots, int layers);
int llmie_lora_slot_load(void *table_dev, int slots, int layers, int slot, const llmie_lora_adapter *host_desc, llmie_stream stream);
size_t llmie_lora_workspace_bytes(int max_rows, int slots, int max_rank_total);
int llmie_lora_plan(const int32_t *slot_dev, const int32_t *lengths_dev /* nullable */, int batch, int rows, const void *table_dev,
                    int slots, void *workspace, size_t workspace_bytes, llmie_stream stream);
int llmie_lora_apply(const void *x /* [rows, K] */, void *y /* [rows, N] in/out */, int rows, int K, int N, int blocks,
                     const int *block_widths /* host, [blocks] */, const void *table_dev, int slots, int layers, int layer, int module,
                     void *workspace, size_t workspace_bytes, llmie_dtype dtype, llmie_stream stream);

/* ABI 3 (an addition).  Per-request adapters in the engine.  While a table is attached, llmie_decoder_forward, _forward_paged,
 * _forward_ragged, _forward_paged_ragged, llmie_decoder_prefill and _prefill_paged run the "lora" launch sequence: the unfused
 * decode sequence (the general prefill sequence: in-place norms, the plain QKV form with the RoPE + append launch in front of the
 * flash kernel, gate/up as projection + llmie_silu_and_mul) with llmie_lora_apply behind the QKV projection (input: the normalised
 * rows; before RoPE), the O projection (input: the attention output), the gate/up projection (input: the FFN-normalised rows; added
 * to the un-activated buffer) and the down projection (input: the SwiGLU output), and ONE llmie_lora_plan per call.  The base
 * projections run as before, on whatever route their planner picks: fp16, int8 or int4 weights.  seq_slot_dev[b] is the slot of
 * batch row b in the decode entries and of sequence b in the prefill entries; it and the table are read on the device at every
 * launch.  workspace: llmie_decoder_lora_workspace_bytes(cfg, max_tokens, slots) = llmie_lora_workspace_bytes(max(max_tokens,
 * cfg->max_batch), slots, 192) bytes, the attach call's own (llmie_decoder_workspace_bytes and
 * llmie_decoder_prefill_workspace_bytes keep their values); a call with more rows than it covers is LLMIE_ERR_WORKSPACE.  The table
 * must have cfg->num_layers layers.  llmie_decoder_plan_name and llmie_decoder_prefill_layer_plan describe the sequence under
 * LLMIE_PLAN_LORA.  llmie_decoder_lora_detach restores the previous sequences exactly.
 * LLMIE_ERR_UNSUPPORTED: an LLMIE_F32 engine; an LLMIE_W_FP8 engine (its sequences never materialise fp16 normalised rows); an
 * LLMIE_DEC_PACKED_ONLY engine (it has no row-major route for the base projections); hidden or inter sizes that are not multiples
 * of 32, or q / kv widths that are not multiples of 16. */
#define LLMIE_PLAN_LORA 1024u /* an adapter table is attached (llmie_decoder_lora_attach) */
size_t llmie_decoder_lora_workspace_bytes(const llmie_decoder_config *cfg, int max_tokens, int slots);
int llmie_decoder_lora_attach(llmie_decoder *dec, const void *table_dev, int slots, const int32_t *seq_slot_dev, void *workspace,
                              size_t workspace_bytes);
int llmie_decoder_lora_detach(llmie_decoder *dec);

/* ABI 3 (an addition; llmie_decoder_config is not touched).  Sliding-window attention with sink tokens on an engine, per layer: the
 * mask stated at llmie_decoder_mha_window (query i sees key j iff j <= i and (i - j < W or j < S); absolute positions, RoPE unchanged).
 * layer_window: host array [num_layers], the window W of every layer, 0 = full attention on that layer (alternating local / global
 * stacks); NULL clears every window (sinks must be 0).  sinks: the S of every windowed layer.  The state lives on the engine and is
 * read when a call is planned (the llmie_decoder_lora_attach pattern): from then on every decode entry (forward, _ragged, _paged,
 * _paged_ragged, with any weight format, adapters, the speculative and scoring entries) runs the windowed instantiation of the
 * split-KV kernel on the windowed layers -- grid and time bounded by the window, not by the context -- and every prefill entry the
 * windowed instantiation of its flash kernel, which walks only the key tiles some query of the workgroup sees.  Only the attention
 * launches change; with no window set nothing does, and llmie_decoder_set_window(dec, NULL, 0) restores today's bits.
 * LLMIE_ERR_INVALID_ARG: a negative window or sinks; sinks without a window on any layer.  LLMIE_ERR_UNSUPPORTED: an engine whose
 * decode attention has no windowed form (fp32; head sizes other than 64 / 128; head ratios other than 1 / 2 / 4 / 8; with an e4m3 cache also ratio 8).
 * A call whose operands send its attention to the generic kernel (unaligned buffers) fails with LLMIE_ERR_UNSUPPORTED while a window
 * is set: it would attend to everything.  llmie_decoder_plan_name and llmie_decoder_prefill_layer_plan answer for a windowed call
 * under LLMIE_PLAN_WINDOW (same sequences; NULL for an engine set_window refuses; the layer plan ends in " attn_window=1"). */
#define LLMIE_PLAN_WINDOW 2048u /* a sliding window is set on some layer (llmie_decoder_set_window) */
int llmie_decoder_set_window(llmie_decoder *dec, const int32_t *layer_window /* host, [num_layers], 0 = full; NULL clears */, int sinks);

/* ABI 3 (additions; llmie_decoder_config is not touched).  The two attention properties of gpt-oss / Llama-3 checkpoints on an engine.
 *
 * llmie_decoder_set_head_sinks: the learned per-head sink logits stated at llmie_decoder_mha_sink, head_sink_dev = DEVICE array
 * [num_layers, head_num] of fp32 (row l = layer l; -INFINITY = no sink for that head); NULL clears.  The pointer is kept on the
 * engine -- the array must stay alive while it is set -- and read when a call is planned, in the pattern of llmie_decoder_set_window;
 * its VALUES are read on the device at every launch, so a captured step replays with new values.  From then on every decode entry
 * and every prefill entry (and the spec, score, LoRA and MoE sequences built on them) runs the SINK instantiation of its attention
 * launch with the layer's row; windows compose.  Only the attention launches change; llmie_decoder_set_head_sinks(dec, NULL) restores
 * today's bits.  LLMIE_ERR_UNSUPPORTED: an engine whose decode attention has no such form (fp32; head sizes other than 64 / 128; head
 * ratios other than 1 / 2 / 4 / 8; with an e4m3 cache also ratio 8).  A call whose operands send its attention to the generic kernel
 * (unaligned buffers) fails with LLMIE_ERR_UNSUPPORTED while sinks are set.  llmie_decoder_plan_name and
 * llmie_decoder_prefill_layer_plan answer for such a call under LLMIE_PLAN_HEAD_SINK (same sequences; NULL for an engine
 * set_head_sinks refuses; the layer plan ends in " attn_head_sink=1", after " attn_window=1" when both are set).
 *
 * llmie_decoder_set_rope_scaling: refills the engine's (cos, sin) table with llmie_rope_table_fill(max_seq_len, head_size, rotary_dim,
 * rotary_base, scaling) and uploads it with one SYNCHRONOUS copy: not inside a stream capture, and not while a call that reads the
 * table is in flight.  NULL restores the create-time table bit for bit.  Every fused path reads the table, so decode, prefill and the
 * entries built on them rotate by the new angles.  LLMIE_ERR_UNSUPPORTED: an engine whose decode attention does not take the table
 * (head sizes outside {32,64,128,256} or head ratios outside {1,2,4,8}: those steps rotate with llmie_rope_decode by rotary_base);
 * the refusals of llmie_rope_table_fill apply, and a refused call leaves the table as it was. */
#define LLMIE_PLAN_HEAD_SINK 4096u /* head sinks are set (llmie_decoder_set_head_sinks) */
int llmie_decoder_set_head_sinks(llmie_decoder *dec, const float *head_sink_dev /* device, [num_layers, head_num]; NULL clears */);
int llmie_decoder_set_rope_scaling(llmie_decoder *dec, const llmie_rope_scaling *scaling /* host; NULL = the create-time table */);

/* ABI 3 (an addition; llmie_decoder_config is not touched).  QK-norm (stated at llmie_qk_norm) on an engine: q_gamma_dev / k_gamma_dev =
 * DEVICE arrays [num_layers, head_size] of fp16 (row l = layer l), 16-byte aligned; both NULL clears.  The pointers and eps are kept
 * on the engine -- the arrays must stay alive while they are set -- and read when a call's attention launch is built, in the pattern
 * of llmie_decoder_set_head_sinks; the VALUES are read on the device at every launch.  From then on every decode entry runs the QKN
 * instantiation of its attention launch, and every prefill entry plans the QKV forms without the RoPE epilogue (plain, plain_e4m3,
 * unpack_plain, splitk: what LLMIE_SW_NO_QKV_ROPE_FUSION plans) and normalises in the RoPE + append launch in front of the flash
 * kernel; the spec, score, beam, LoRA and MoE sequences built on them follow.  llmie_decoder_set_qk_norm(dec, NULL, NULL, eps)
 * restores today's bits.  LLMIE_ERR_INVALID_ARG: exactly one NULL; an array not 16-byte aligned; eps < 0 or NaN.
 * LLMIE_ERR_UNSUPPORTED: an engine whose decode attention has no such form (fp32; head sizes other than 64 / 128; head ratios other
 * than 1 / 2 / 4 / 8; with an e4m3 cache also ratio 8); a layer with a QKV bias; a window or head sinks set on the engine -- and
 * llmie_decoder_set_window / llmie_decoder_set_head_sinks with a non-NULL argument refuse while QK-norm is set.  A call whose
 * operands send its attention to the generic kernel (unaligned buffers) fails with LLMIE_ERR_UNSUPPORTED while QK-norm is set and
 * writes nothing.  llmie_decoder_plan_name and llmie_decoder_prefill_layer_plan answer for such a call under LLMIE_PLAN_QK_NORM
 * (decode: same sequences; NULL for an engine set_qk_norm refuses; the layer plan ends in " qk_norm=1"). */
#define LLMIE_PLAN_QK_NORM 8192u /* QK-norm is set (llmie_decoder_set_qk_norm) */
int llmie_decoder_set_qk_norm(llmie_decoder *dec, const void *q_gamma_dev, const void *k_gamma_dev /* device, [num_layers, head_size] fp16;
                              both NULL clears */, float eps);

/* ABI 3 (an addition; llmie_decoder_config is not touched).  A draft tree on an engine: depth_dev / anc_dev = DEVICE arrays
 * [batch, stride] as llmie_spec_tree_prepare leaves them (int32 / uint64), 1 <= stride <= LLMIE_SPEC_TREE_MAX_NODES; NULL, NULL, 0
 * clears.  The pointers are kept on the engine, in the pattern of llmie_decoder_set_qk_norm; the VALUES are read on the device at
 * every launch, so a captured step follows a new tree on replay.  While a tree is set, every prefill entry (llmie_decoder_prefill,
 * _prefill_paged and the LoRA and MoE sequences built on them) treats position i < input_lengths[b] of sequence b as node i:
 *   RoPE + append: q and k are rotated by the table row history[b] + clamp(depth[b, i], 0, i); k / v go to slot history[b] + i;
 *   attention: query i sees key t iff t < history[b], or t = history[b] + j with bit j of
 *     (anc[b, i] & ((2 << i) - 1)) | (1 << i) set (64-bit): bits above i are ignored and the self bit is forced, so no row is
 *     fully masked.
 * Such a call always plans the 64-row flash form (q64w4t1) behind the RoPE + append launch and the QKV forms without the RoPE
 * epilogue, as QK-norm does; it composes with QK-norm and the e4m3 cache.  A chain -- depth[i] = i, anc[i] = (2 << i) - 1 -- gives
 * the bits of the same call without a tree wherever that call plans q64w4t1.  The decode entries ignore the tree.
 * LLMIE_ERR_INVALID_ARG: exactly one array NULL, stride outside [1, 64] (or not 0 when clearing), misaligned arrays; a prefill call
 * with max_q_len > stride while a tree is set.  LLMIE_ERR_UNSUPPORTED, nothing written: an engine without a prefill path; a sliding
 * window or head sinks set on the engine -- and llmie_decoder_set_window / llmie_decoder_set_head_sinks with a non-NULL argument
 * refuse while a tree is set (both are follow-ups).  llmie_decoder_plan_name and llmie_decoder_prefill_layer_plan answer for such a
 * call under LLMIE_PLAN_TREE (refused together with LLMIE_PLAN_WINDOW / LLMIE_PLAN_HEAD_SINK; the layer plan ends in " tree"). */
#define LLMIE_PLAN_TREE 16384u /* a draft tree is set (llmie_decoder_set_tree) */
int llmie_decoder_set_tree(llmie_decoder *dec, const int32_t *depth_dev, const uint64_t *anc_dev /* device, [batch, stride]; both NULL clears */,
                           int stride);

/* ABI 3 (an addition).  Mixture-of-experts FFN, Mixtral / Qwen-MoE semantics: every row is routed to top_k of `experts` expert FFNs.
 * fp16 activations and fp16 experts only.  Operands (device, 16-byte aligned): x [rows, hidden]; router Wr [experts, hidden];
 * gate_up [experts, 2 * inter, hidden] with rows [0, inter) of an expert its gate and [inter, 2 inter) its up matrix, as the dense
 * gate_up; down [experts, hidden, inter]; resid [rows, hidden] or NULL; y [rows, hidden].  `inter` is the EXPERT inter size.
 * 1 <= experts <= LLMIE_MOE_MAX_EXPERTS, 1 <= top_k <= min(experts, LLMIE_MOE_MAX_TOP_K), hidden % 64 == 0, inter % 64 == 0.
 *
 * The arithmetic, for one row x (E = experts, k = top_k, Ie = inter):
 *   router     r[e] = sum_i x[i] * Wr[e][i]: fp16 inputs, fp32 accumulation, summation order unspecified.
 *   selection  the k largest logits ranked by (logit descending, expert id ascending): e_0 .. e_{k-1}, logits r_0 >= .. >= r_{k-1}.
 *              A NaN logit ranks as -inf.  Every emitted id lies in [0, E) whatever the input.
 *   weights    fp32.  Default (Mixtral): w_j = exp(r_j - r_0) / sum_{j < k} exp(r_j - r_0) over the selected logits (= softmax over
 *              all experts, renormalised over the selected).  LLMIE_MOE_SOFTMAX_ALL (Qwen norm_topk_prob = false): w_j =
 *              exp(r_j - r_0) / sum_{e < E} exp(r[e] - r_0), no renormalisation.
 *   expert     for rank j: a_j = fp16(silu(g) * u) with g, u the fp32 accumulations of x against expert e_j's gate and up rows, SiLU
 *              and the product in fp32, ONE rounding; d_j = the fp32 accumulation of a_j against expert e_j's down rows.
 *   combine    y = fp16((w_0 d_0 + w_1 d_1 + ... in rank order, fp32) + resid): ONE rounding.  No atomics on results.
 *   A row whose largest logit is not finite -- every logit a NaN or -inf, or a +inf logit -- has NaN weights (exp(r_j - r_0) of
 *   inf - inf) and therefore a NaN output row: a non-finite router input shows in y, as it would after a dense FFN.  Its ids are valid.
 * Bit-reproducible: the bits of an output row depend on that row's input, the weights and the route (below) only -- not on the
 * row's position and not on the other rows of the call.
 *
 * Two routes, chosen by a pure host function of (rows, hidden, inter, experts, top_k, flags):
 *   gemv     rows <= 4 (and hidden, inter <= 16384): route, gate/up + SwiGLU (grid: blocks of 16 inter columns x pairs; a workgroup
 *            reads its (row, rank) pair's expert id on the device and streams that expert's rows), down + combine (grid: blocks of
 *            16 hidden columns x rows; walks the row's k experts in rank order).  3 launches; at one row exactly the k selected
 *            experts are read.
 *   grouped  otherwise: route, plan (one workgroup: each expert's pairs in (row, rank) order cut into tiles of <= 16 * RT pairs; RT =
 *            4 once rows * top_k / experts >= 32, else 1), gate/up + SwiGLU and down on v_mfma_f32_16x16x32_f16 over
 *            tiles = rows * top_k / (16 RT) + min(experts, rows * top_k) workgroup rows (surplus ones exit on the device tile count:
 *            nothing is read back, a captured call replays with other routings), combine.  5 launches.
 *   LLMIE_MOE_FORCE_GEMV (rows <= 16) and LLMIE_MOE_FORCE_GROUPED override the choice; LLMIE_MOE_FORCE_RT1 / _RT4 the tile height of
 *   the grouped route (a row's bits do not depend on it).
 * llmie_moe_workspace_bytes(max_rows, ...) covers llmie_moe_ffn at every rows <= max_rows under any flags (256-byte aligned
 * sections: header, expert ids, weights, a, the tile list, d); 0 for a shape the entries refuse.  llmie_moe_ffn_plan answers one
 * line, "route=gemv|grouped rt=.. tiles=.. route_grid=.. plan_grid=.. gate_up_grid=AxB down_grid=AxB combine_grid=AxB ws=BYTES"
 * (ws: what that call needs of its workspace), or NULL + llmie_last_error() where llmie_moe_ffn would refuse the shape or flags.
 * llmie_moe_route runs the route launch alone: expert_out [rows, top_k] int32, weight_out [rows, top_k] fp32.
 * Refused on the host before any launch.  LLMIE_ERR_INVALID_ARG: NULL pointers (resid excepted), non-positive sizes, unknown or
 * contradictory flags.  LLMIE_ERR_UNSUPPORTED: LLMIE_F32; experts or top_k outside the ranges above; hidden or inter not a
 * multiple of 64; an operand not 16-byte aligned; LLMIE_MOE_FORCE_GEMV above 16 rows.  LLMIE_ERR_WORKSPACE: NULL, short or not
 * 256-byte aligned.  No entry allocates or synchronises; all are legal inside a graph capture.  y may be the buffer of x (the engine
 * runs it in place): x is last read before y is first written. */
#define LLMIE_MOE_MAX_EXPERTS 128
#define LLMIE_MOE_MAX_TOP_K 8
#define LLMIE_MOE_SOFTMAX_ALL 1u
#define LLMIE_MOE_FORCE_GEMV 2u
#define LLMIE_MOE_FORCE_GROUPED 4u
/* measurement only (tools/moebench.py compares the tile heights): not a serving control, a row's bits do not depend on them */
#define LLMIE_MOE_FORCE_RT1 8u  /* grouped route: tiles of 16 pairs whatever the row count */
#define LLMIE_MOE_FORCE_RT4 16u /* grouped route: tiles of 64 pairs whatever the row count */
size_t llmie_moe_workspace_bytes(int max_rows, int hidden, int inter, int experts, int top_k);
const char *llmie_moe_ffn_plan(int rows, int hidden, int inter, int experts, int top_k, unsigned flags);
int llmie_moe_route(const void *x, const void *router, int rows, int hidden, int experts, int top_k, unsigned flags,
                    int32_t *expert_out /* [rows, top_k] */, float *weight_out /* [rows, top_k] */, llmie_dtype dtype, llmie_stream stream);
int llmie_moe_ffn(const void *x, const void *router, const void *gate_up, const void *down, const void *resid /* nullable */, void *y,
                  int rows, int hidden, int inter, int experts, int top_k, unsigned flags, void *workspace, size_t workspace_bytes,
                  llmie_dtype dtype, llmie_stream stream);

/* ABI 3 (an addition).  The _ex entries: MXFP4 experts, router and expert biases and gpt-oss's clamped SwiGLU.  Each takes the operands
 * of its counterpart above with one expert descriptor -- a HOST struct, copied by the call -- in place of the router / gate_up / down
 * pointers.  Everything said above (shapes, selection, weights, routes, flags, workspace, bit-reproducibility, no atomics) holds; the
 * additions to the arithmetic:
 *   router     r[e] = (the fp32 sum) + float(router_bias[e]): one fp32 add.
 *   gate/up    g, u = the fp32 accumulation of x against the expert's gate and up rows, + float(gate_up_bias[e][n]) and
 *              + float(gate_up_bias[e][inter + n]).  LLMIE_W_MXFP4: the rows are the exact values of the codes, (-1)^s * {0, .5, 1,
 *              1.5, 2, 3, 4, 6} * 2^e(block of 32); both routes multiply the unscaled codes (exact fp16 numbers) and apply the block's
 *              2^e to the block's fp32 partial sum -- gemv: per lane and block; grouped: to the MFMA's 16 x 16 tile of that block.
 *   act        LLMIE_MOE_ACT_SWIGLU: a = fp16(silu(g) * u).  LLMIE_MOE_ACT_SWIGLU_CLAMPED: g' = min(g, limit), u' = clamp(u, -limit,
 *              limit), a = fp16((u' + 1) * g' / (1 + expf(-alpha * g'))): ONE rounding (gpt-oss: alpha 1.702, limit 7).
 *   down       d_j = (the fp32 accumulation) + float(down_bias[e_j][c]);  combine  y = fp16(sum_j w_j d_j (rank order) + resid).
 * MXFP4 experts are laid out exactly as llmie_quantize_mxfp4 writes the flattened [experts * 2 inter, hidden] and [experts * hidden,
 * inter] matrices: codes uint8, two per byte, and one e8m0 byte per 32 k, block exponents in the pinned range [-23, 13]; outside
 * it, or for a 0xFF block, results are unspecified but the call stays in bounds and terminates.  A loader of gpt-oss checkpoints
 * de-interleaves the even / odd gate / up columns into [gate; up] first.
 * With format LLMIE_W_F16, no bias and LLMIE_MOE_ACT_SWIGLU, llmie_moe_ffn_ex launches what llmie_moe_ffn launches and returns its bits.
 * llmie_moe_workspace_bytes covers the _ex entries in both formats (the MXFP4 routes use the same sections).  llmie_moe_ffn_plan_ex:
 * the line of llmie_moe_ffn_plan for that format followed by " format=f16|mxfp4 act=swiglu|swiglu_clamped".  MXFP4 experts take the
 * gemv route up to 16 rows (fp16: 4), where it is measured ahead of the grouped one; RT as above.
 * llmie_moe_route_ex reads the descriptor's router and router_bias only.
 * Refused on the host before any launch, beyond what the counterparts refuse.  LLMIE_ERR_UNSUPPORTED: a format other than
 * LLMIE_W_F16 / LLMIE_W_MXFP4; router, gate_up (codes) or down (codes) not 16-byte aligned; a bias not 2-byte aligned (scale bytes
 * need no alignment).  LLMIE_ERR_INVALID_ARG: a NULL descriptor, router, gate_up or down; a NULL scale with LLMIE_W_MXFP4; a
 * non-NULL scale with LLMIE_W_F16; an unknown act; with the clamped act a limit that is not finite and > 0 or an alpha that is
 * not finite. */
typedef enum { LLMIE_MOE_ACT_SWIGLU = 0, LLMIE_MOE_ACT_SWIGLU_CLAMPED = 1 } llmie_moe_act;
typedef struct {
    llmie_weight_format format;          /* LLMIE_W_F16 or LLMIE_W_MXFP4; anything else LLMIE_ERR_UNSUPPORTED */
    const void *router;                  /* [E, H] fp16; NULL in an engine layer list = the layer keeps its dense FFN */
    const void *router_bias;             /* nullable, [E] fp16 */
    const void *gate_up, *gate_up_scale; /* F16: [E, 2Ie, H], scale NULL.  MXFP4: codes uint8 [E, 2Ie, H/2], e8m0 uint8 [E, 2Ie, H/32] */
    const void *gate_up_bias;            /* nullable, [E, 2Ie] fp16: [0, Ie) gate, [Ie, 2Ie) up */
    const void *down, *down_scale;       /* F16: [E, H, Ie].  MXFP4: [E, H, Ie/2] + [E, H, Ie/32] */
    const void *down_bias;               /* nullable, [E, H] fp16 */
    llmie_moe_act act; float alpha, limit; /* CLAMPED only (gpt-oss: 1.702, 7.0); limit > 0 and finite, alpha finite */
} llmie_moe_experts;
const char *llmie_moe_ffn_plan_ex(int rows, int hidden, int inter, int experts, int top_k, unsigned flags, llmie_weight_format format,
                                  llmie_moe_act act);
int llmie_moe_route_ex(const void *x, const llmie_moe_experts *ex, int rows, int hidden, int experts, int top_k, unsigned flags,
                       int32_t *expert_out /* [rows, top_k] */, float *weight_out /* [rows, top_k] */, llmie_dtype dtype, llmie_stream stream);
int llmie_moe_ffn_ex(const void *x, const llmie_moe_experts *ex, const void *resid /* nullable */, void *y, int rows, int hidden, int inter,
                     int experts, int top_k, unsigned flags, void *workspace, size_t workspace_bytes, llmie_dtype dtype, llmie_stream stream);

/* ABI 3 (an addition; llmie_decoder_config is not touched).  Experts on an engine, the llmie_decoder_lora_attach pattern.  layers:
 * HOST array [num_layers], copied; a layer whose router is NULL keeps its dense FFN (interleaved dense / sparse stacks), every other
 * layer runs llmie_moe_ffn (router [experts, hidden], gate_up [experts, 2 * inter, hidden], down [experts, hidden, inter], fp16,
 * device, 16-byte aligned) in place of its gate/up and down launches; `inter` is the expert inter size and need not equal
 * cfg->inter_size.  The dense gate_up / down of a sparse layer are still what llmie_decoder_create was given (valid matrices of
 * cfg->inter_size: the create call may pack them) and are not read by a call.  While attached, llmie_decoder_forward, _forward_paged,
 * _forward_ragged, _forward_paged_ragged run the "moe" sequence -- the unfused decode sequence, with the fused attention launch
 * carrying paged / e4m3 caches and ragged lengths where the geometry has it, as the lora sequence -- and llmie_decoder_prefill /
 * _prefill_paged the general prefill sequence in its in-place-norm forms; in both, the FFN of a sparse layer is route + expert
 * launches on the FFN-normalised rows with the layer's residual through `resid`, accounted under LLMIE_OP_FFN_NORM (route),
 * LLMIE_OP_GATE_UP_SWIGLU (plan, gate/up) and LLMIE_OP_DOWN_GEMM (down, combine).  The
 * attention projections keep the engine's weight format; a sliding window combines freely.  flags: LLMIE_MOE_*.
 * workspace: llmie_decoder_moe_workspace_bytes(cfg, max_tokens, inter, experts, top_k) = llmie_moe_workspace_bytes(max(max_tokens,
 * cfg->max_batch), hidden, ...) bytes, the attach call's own, 256-byte aligned; a call with more rows than it covers is
 * LLMIE_ERR_WORKSPACE before anything is enqueued.  llmie_decoder_plan_name and llmie_decoder_prefill_layer_plan answer for an
 * engine without experts.  llmie_decoder_moe_detach restores the previous sequences exactly.
 * LLMIE_ERR_UNSUPPORTED: an engine that is not fp16 with fp16 / int8 / int4 weights, LLMIE_DEC_PACKED_ONLY, hidden % 64 != 0, an
 * adapter table attached at the same time (either order), and what llmie_moe_ffn refuses of the expert geometry. */
typedef struct {
    const void *router, *gate_up, *down; /* router == NULL: the layer keeps its dense FFN */
} llmie_moe_layer;
size_t llmie_decoder_moe_workspace_bytes(const llmie_decoder_config *cfg, int max_tokens, int inter, int experts, int top_k);
int llmie_decoder_moe_attach(llmie_decoder *dec, const llmie_moe_layer *layers /* host, [num_layers], copied */, int inter, int experts,
                             int top_k, unsigned flags, void *workspace, size_t workspace_bytes);
/* The same with expert descriptors (llmie_moe_ffn_ex): layers is a HOST array [num_layers], copied; a layer whose router is NULL keeps
 * its dense FFN, every other layer runs llmie_moe_ffn_ex on its descriptor -- the same "moe" sequences, accounting, workspace and
 * refusals as llmie_decoder_moe_attach.  The engine's own weight format stays fp16 / int8 / int4 whatever the experts' format
 * (gpt-oss keeps its attention unquantised).  Refused in addition: what llmie_moe_ffn_ex refuses of a sparse layer's descriptor;
 * LLMIE_ERR_UNSUPPORTED for sparse layers that disagree in format or act.  llmie_decoder_moe_detach detaches either kind. */
int llmie_decoder_moe_attach_ex(llmie_decoder *dec, const llmie_moe_experts *layers /* host, [num_layers], copied */, int inter, int experts,
                                int top_k, unsigned flags, void *workspace, size_t workspace_bytes);
int llmie_decoder_moe_detach(llmie_decoder *dec);

/* Prefill through all layers = LlamaContextDecoder<T>::forward (src/layers/context_decoder.cpp:58-199,
 * context_attention.cpp:143-312) on PACKED tokens: hidden_in/out [num_tokens, H] hold the sequences back to back
 * (input_lengths[b] tokens each, device int32), history_lengths[b] tokens of each sequence are already in the caches;
 * k/v of the new tokens are appended at history+pos.  Attention is a flash kernel: causal mask from the lengths,
 * no padding buffers, no [bs,nh,q,k] score matrix.  fp16 engines with fp16 or fp8 weights (fp8: every projection
 * input is quantised per token, llmie_linear_fp8 semantics) and head_size 128.
 * Caches are [L, batch, kvh, max_seq, hs] with the batch of THIS call.  workspace: caller-owned scratch. */
size_t llmie_decoder_prefill_workspace_bytes(const llmie_decoder_config *cfg, int max_tokens, int max_batch);
int llmie_decoder_prefill(llmie_decoder *dec, const void *hidden_in, void *hidden_out, void *k_cache, void *v_cache,
                          const int32_t *input_lengths, const int32_t *history_lengths, int batch, int num_tokens,
                          int max_q_len, void *workspace, size_t workspace_bytes, llmie_stream stream);

/* LM head + top-k + sampling tail (llama.cpp:247-318): final RMSNorm(gamma) -> logits =
 * x . lm_head[V,H]^T -> top-K -> sample.  logits[bs,V] and topk buffers caller-owned.
 * `hidden` is CLOBBERED and its content afterwards is unspecified: the fused-norm GEMV form (fp16, small batches) leaves it
 * as it was, every other form RMS-normalises it in place as the reference does (llama.cpp:247) -- do not read it, and do not
 * call this twice on one buffer.  Candidates the top-k could not fill (NaN logits) are skipped by the sampler; a row without
 * any valid candidate emits end_id and sets finished.  In fp16 the sampler keeps exp(v - max) in fp32 where sampling.cu:31
 * rounds it to T first: the chosen token can differ at a bin edge (parity unpinned there, the cuRAND stream is not reproducible
 * either). */
int llmie_lm_head_sample(llmie_decoder *dec, void *hidden /* [bs,H]; clobbered (may be normalised in place) */,
                         const void *final_norm_gamma, const llmie_matrix *lm_head,
                         llmie_weight_format lm_fmt, void *logits,
                         int32_t *tmp_ids, void *tmp_vals, int32_t *topk_ids, void *topk_vals,
                         int K, int blocks_per_row, int32_t *seq_len, uint8_t *finished,
                         int32_t *out_ids, int batch, int step, const int32_t *step_dev,
                         int end_id, llmie_stream stream);

/* ABI 3.  llmie_lm_head_sample with the tail of the step fused into ONE launch behind round 1 of the top-k: round 2 + sampling
 * (bit-identical ids / values / picks / seq_len / finished) + -- if next_hidden != NULL -- the next step's input embedding
 * (next_hidden[b, :] = embed_table[out_ids[b], :], llmie_input_embedding's rule for ids outside the table; llama.cpp:219 of the
 * next token) + -- if advance_step != 0 -- *step_dev += 1 once every row has read it (llmie_advance_step).  Replaces four
 * launches of the batch-1 step (top-k round 2, sampling, advance_step, input_embedding). */
int llmie_lm_head_sample_next(llmie_decoder *dec, void *hidden, const void *final_norm_gamma, const llmie_matrix *lm_head,
                              llmie_weight_format lm_fmt, void *logits, int32_t *tmp_ids, void *tmp_vals, int32_t *topk_ids,
                              void *topk_vals, int K, int blocks_per_row, int32_t *seq_len, uint8_t *finished, int32_t *out_ids,
                              int batch, int step, int32_t *step_dev, int end_id, const void *embed_table, void *next_hidden,
                              int advance_step, llmie_stream stream);

/* ABI 3.  The LM head of llmie_lm_head_sample (final norm, or the fused-norm GEMV where that route applies) followed by
 * llmie_sample_logits on the decoder's vocab_size and dtype, with llmie_lm_head_sample_next's options: next_hidden[b] =
 * embed_table[out_ids[b]] if next_hidden != NULL, and *step_dev += 1 once every row has read it if advance_step != 0.  The
 * sampler is one launch (LM head + 1, or + 2 with a separate final norm). */
int llmie_lm_head_sample_params(llmie_decoder *dec, void *hidden, const void *final_norm_gamma, const llmie_matrix *lm_head,
                                llmie_weight_format lm_fmt, void *logits, const llmie_sampling_params *params_dev, int32_t *history,
                                int history_stride, int32_t *history_len, int history_append, int32_t *seq_len, uint8_t *finished,
                                int32_t *out_ids, float *out_logprob, int batch, int step, int32_t *step_dev, int end_id,
                                const void *embed_table, void *next_hidden, int advance_step, void *workspace, size_t workspace_bytes,
                                llmie_stream stream);

/* ABI 3 (an addition).  llmie_lm_head_sample_params with the controls of llmie_sample_logits_ext in its sampler launch (still
 * one launch behind the LM head).  ext == NULL or an empty struct: llmie_lm_head_sample_params itself. */
int llmie_lm_head_sample_ext(llmie_decoder *dec, void *hidden, const void *final_norm_gamma, const llmie_matrix *lm_head,
                             llmie_weight_format lm_fmt, void *logits, const llmie_sampling_params *params_dev, int32_t *history,
                             int history_stride, int32_t *history_len, int history_append, int32_t *seq_len, uint8_t *finished,
                             int32_t *out_ids, float *out_logprob, int batch, int step, int32_t *step_dev, int end_id,
                             const void *embed_table, void *next_hidden, int advance_step, void *workspace, size_t workspace_bytes,
                             llmie_stream stream, const llmie_sampling_ext *ext);

/* Per-kernel timing of the engine (eager launches only, never inside graph capture): between
 * profile_begin and profile_end every kernel the engine launches is bracketed by hipEvents
 * recorded on the launch stream.  profile_end synchronises the stream (the one entry point that
 * does) and returns, per op kind, the summed device time in ms and the number of launches. */
enum {
    LLMIE_OP_ATTN_NORM = 0, LLMIE_OP_QKV_GEMM, LLMIE_OP_ROPE, LLMIE_OP_MHA, LLMIE_OP_O_GEMM,
    LLMIE_OP_FFN_NORM, LLMIE_OP_GATE_UP_SWIGLU, LLMIE_OP_DOWN_GEMM, LLMIE_OP_FINAL_NORM,
    LLMIE_OP_LM_HEAD, LLMIE_OP_TOPK, LLMIE_OP_SAMPLING,
    LLMIE_OP_CHAIN, /* ABI 3: one persistent launch = O -> gate/up -> down -> next QKV of the packed batch-decode path */
    LLMIE_OP_COUNT /* prefill re-uses the layer op kinds */
};
int llmie_decoder_profile_begin(llmie_decoder *dec, int max_events);
int llmie_decoder_profile_end(llmie_decoder *dec, llmie_stream stream, double *ms_by_op /*[LLMIE_OP_COUNT]*/,
                              int *launches_by_op /*[LLMIE_OP_COUNT]*/);

/* ABI 3.  The persistent chain launches of the batch-decode path (4 < batch <= 32) synchronise their workgroups with in-kernel
 * grid barriers whose spins are bounded: a barrier that expires (a workgroup was not resident) sets a device-side error word and
 * the launch returns early instead of hanging.  This call synchronises `stream`, reads the word and returns LLMIE_ERR_LAUNCH with
 * a message if it is set (and clears it); LLMIE_OK otherwise.  Not on the compute path: for tests and health checks. */
int llmie_decoder_status(llmie_decoder *dec, llmie_stream stream);
/* ABI 3, diagnostic: arm (device pointer to 256 x 16 uint64) or disarm (NULL) the phase-edge timestamps of the chain launches:
 * per workgroup the s_memrealtime (100 MHz) values at kernel start, then before / behind every grid barrier, then at the end. */
int llmie_decoder_debug_stamps(llmie_decoder *dec, void *stamps_dev);

/* device-side helper for graph replay: *step_dev += 1 */
int llmie_advance_step(int32_t *step_dev, llmie_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMIE_H */
