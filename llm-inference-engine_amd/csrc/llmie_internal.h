// Internal (non-ABI) entry points shared between translation units of libllmie.so.
#pragma once
#include "device_utils.cuh"

#include <type_traits>

namespace llmie {

enum : int { EPI_NONE_ = 0, EPI_SWIGLU_ = 1 };

// fp16 activations, fp16 W[N,K]; epi = 0 plain (bias/residual optional), 1 = SwiGLU over row
// pairs (i, N/2+i) writing y[M, N/2].  Defined in linear.hip.
// Caller-owned fp32 scratch for split-K slabs (nothing on the compute path allocates).  p == nullptr: the split-K forms are
// not available to the call (fp16 falls back to its non-split kernels; shapes that only have a split-K form fail with
// LLMIE_ERR_WORKSPACE); p != nullptr but too small / not 16-byte aligned: LLMIE_ERR_WORKSPACE.
struct SlabWs {
    float *p;
    size_t floats;
};
size_t linear_splitk_ws_floats(int wbits, int M, int K, int N);   // 0 = the shape has no split-K form

// ---- which kernel a projection runs on: decided once, by a pure host function per weight family (linear.hip) ----
enum LinearRoute : int {
    LR_REFUSED = 0,
    // fp16 weights
    LR_GEMV_KSPLIT, LR_GEMV_LDS, LR_SPLITK, LR_SPLITK_PASSES, LR_SKINNY, LR_SWIGLU256, LR_TILES256, LR_TILES256_PART, LR_TILES128, LR_GENERIC,
    // int8 / int4 weights
    LR_W8_G8P, LR_W8_G8P_SWIGLU, LR_W8_SPLITK_PASSES, LR_WQ_IMAGE_PREFILL, LR_WQ_IMAGE_LAST, LR_WQ_GEMV, LR_W4_SPLITK, LR_W4_CHUNKS,
    LR_W8_SPLITK, LR_W8_SKINNY,
    // MXFP4 weights (mxfp4_linear.hip)
    LR_MX4_GEMV, LR_MX4_MFMA, LR_MX4_CHUNKS,
    // e4m3 weights x per-token e4m3 activations (fp8_linear.hip)
    LR_FP8_GEMV, LR_FP8_GEMM256, LR_FP8_SPLITK,
};
enum LinearRefusal : int {
    LREF_NONE = 0, LREF_F16_SWIGLU, LREF_SLABS, LREF_W4_SPLITK, LREF_WQ_NORM, LREF_WQ_SWIGLU, LREF_WQ_SHAPE, LREF_MX4_SHAPE, LREF_MX4_EPI,
    LREF_F16_NORM, LREF_FP8_SHAPE, LREF_FP8_ACT, LREF_FP8_GEMV,
};
// ---- a projection call, from the C entry (or the engine) to the launch: two structs.  A new operand is added to LinearOperands, at the
// entries that fill it, in linear_call() where a planner has to see it, and at the launch that reads it.  The weight format (`bits`:
// 16 / 8 / 4, WF_FP8, WF_MXFP4) decides the element types behind the void pointers: x, y, bias, residual, gamma, pre_bias are fp16 in
// every format; scale is fp16 per row (int8) or per group (int4), fp32 per row (fp8), e8m0 bytes per 32 k (MXFP4), unused (fp16).
struct LinearOperands {   // y = [swiglu]( rmsnorm(x + pre_bias) * gamma . w^T ) (+ bias) (+ residual); gamma null: no norm
    const void *x, *w, *scale;
    void *y;
    int M, K, N, epi, group;   // epi: EPI_NONE_ / EPI_SWIGLU_ (N = two_inter, y is [M, N / 2]); group: int4 scale group
    const void *bias, *residual, *gamma, *pre_bias;
    float eps;
};
struct LinearScratch {    // caller-owned, each area optional (null): a route that needs a missing one is not planned, or refused
    SlabWs slabs;                     // fp32 split-K slabs
    void *image;                      // fp16 image of quantised weights
    size_t image_bytes;
    void *act;                        // fp8: e4m3 activations + per-token scales (fp8_act_bytes, 256-byte aligned)
    size_t act_bytes;
};
// The call as the planners see it: shape, epilogue, which operands are there and how far each pointer is from 16-byte alignment
// (address % 16; 0 for a null pointer; the fp8 activation area: % 256), and the caller's scratch.  bits = 16: fp16 weights (group /
// scale / image unused).
struct LinearCall {
    int bits, M, K, N, epi, group;
    bool bias, residual, gamma, pre_bias;
    unsigned mis_x, mis_w, mis_y, mis_bias, mis_residual, mis_gamma, mis_pre_bias, mis_scale, mis_image;
    bool slabs;            // split-K slab workspace present
    size_t slab_floats;
    bool image;            // scratch for the fp16 image of quantised weights present
    size_t image_bytes;
    bool act;              // fp8 activation scratch present
    size_t act_bytes;
    unsigned mis_act;      // its address % 256
};
struct LinearPlan {
    int route;             // LinearRoute
    int refusal;           // LinearRefusal of LR_REFUSED
    size_t slab_floats;    // what the route needs of the caller's scratch (0: nothing)
    size_t image_bytes;
    int pass_rows;         // activation rows per pass of the split-K and row-chunk routes
    int inner;             // fp16 image routes: the route of the fp16 GEMM on the image
};
inline unsigned mis16(const void *p) { return static_cast<unsigned>(reinterpret_cast<uintptr_t>(p) % 16); }
// the call with every pointer aligned, no bias / residual / norm and all the scratch a route may ask for: what the size queries plan
LinearCall linear_call_sizing(int bits, int M, int K, int N, int epi, int group = 128);
LinearCall linear_call(int bits, const LinearOperands &o, const LinearScratch &s);
LinearPlan plan_linear_f16(const LinearCall &c);
LinearPlan plan_linear_wq(const LinearCall &c);
LinearPlan plan_linear_fp8(const LinearCall &c);
const char *linear_route_name(int route);
int linear_refuse(const LinearCall &c, const LinearPlan &p);   // sets the refusal's error text, returns its error code
// slab floats to reserve for an fp16 projection of M rows (>= the plan's: see linear.hip)
size_t linear_f16_reserve_slab_floats(int M, int K, int N);
// The projection in the weight format `bits`: plans the call with the format's planner and launches the plan, or refuses.  Every call
// site of the engine comes through here; the per-format launchers below are what it switches over.
int linear_run(int bits, const LinearOperands &o, const LinearScratch &s, hipStream_t st);
// fp16 weights W[N, K] (linear.hip).  gamma: rmsnorm(x + pre_bias) * gamma fused in front -- the GEMV routes only
// (LLMIE_ERR_UNSUPPORTED otherwise, so that the caller can run the norm as its own kernel)
int linear_f16_nk(const LinearOperands &o, const LinearScratch &s, hipStream_t st);
bool gemv_f16_eligible(int M, int K, const void *x, const void *W);

// split-K skinny MFMA GEMM (fp16 or int8 weights), any M processed 64 tokens per pass; epi may be SwiGLU; linear.hip
// partial products of a split-K projection: fp32 slabs [KS][M][N] in the caller's SlabWs
struct SplitKSlabs {
    float *slab;
    int KS, M, N;
};
enum : int { WF_FP8 = 108 };  // wbits code of e4m3 weights + e4m3 activations (16 / 8 = fp16 / int8 weights, fp16 activations)
enum : int { WF_MXFP4 = 204 }; // LinearCall::bits of MXFP4 weights (e2m1 codes + e8m0 block scales) under fp16 activations
int linear_splitk_partial(int wbits, const void *x, const void *W, int M, int K, int N, hipStream_t st, SplitKSlabs *out,
                          SlabWs ws, const half_t *gscale = nullptr /* wbits 4: group-128 scales [N, K/128], applied in the kernel */);
int splitk_finalize(const SplitKSlabs &sk, const SlabScale &sc, half_t *y, int epi, const half_t *bias, const half_t *residual,
                    hipStream_t st);
bool splitk_rownorm_eligible(int N);
// y (fp16, may be null) and/or xq + xscale (per-token e4m3, may be null) receive the normalised row
int splitk_rownorm(const SplitKSlabs &sk, const SlabScale &wscale, const half_t *bias, half_t *resid, const half_t *gamma,
                   float eps, half_t *y, uint8_t *xq, float *xscale, hipStream_t st);
// RMSNorm (plain or add-residual-bias form) emitting per-token e4m3 instead of the normalised fp16 row; norm.hip
bool rmsnorm_quant_eligible(int hidden);
int rmsnorm_quant_f16(const half_t *x, half_t *resid, const half_t *bias, const half_t *gamma, float eps, int tokens, int hidden,
                      bool fused, uint8_t *xq, float *xscale, hipStream_t st);
// out-of-place RMSNorm (x untouched): the prefill's residual stream stays in its own buffer; norm.hip
bool rmsnorm_oop_eligible(int hidden);
int rmsnorm_oop_f16(const half_t *x, half_t *y, const half_t *gamma, float eps, int tokens, int hidden, hipStream_t st);
// per-token e4m3 quantisation of fp16 rows (scale amax/448); fp8_linear.hip
int quantize_rows_fp8(const half_t *x, uint8_t *xq, float *xscale, int M, int K, hipStream_t st);
int linear_splitk(int wbits, const LinearOperands &o, const LinearScratch &s, hipStream_t st);
// The 256-row tiled GEMM family (gemm8p.cuh eight-phase, gemm256.cuh two-stage; K % 64 == 0 fp16, K % 128 == 0 fp8; 16-byte aligned
// operands); linear.hip.  Operand formats: fp16; e4m3 weights and activations (xscale per token, wscale per weight row, fp32); int8
// weights [N, K] under fp16 activations (`wscale` carries their fp16 per-row scales).  The values are llmie_gemm256_tiles' codes.
enum G256Operands : int { G256_F16 = 0, G256_E4M3 = 1, G256_W8 = 2 };
enum G256Form : int { G256_PLAIN = 0, G256_SWIGLU = 1, G256_QKV_ROPE = 2 };
// The tile plan of one projection: one or two launches, each over the column tiles [col0, col0 + tiles * width) of the output
struct G256Range {
    bool eight_phase;   // gemm8p.cuh; false: gemm256_kernel, where the eight-phase kernels' 32-bit DMA offsets do not fit
    int width, col0, tiles;
};
struct G256Plan {
    int ranges;
    G256Range range[2];
};
// N: weight rows (SwiGLU form: two_inter; its ranges are columns of the [M, I] output).  Pure host code.
G256Plan plan_gemm256(G256Form form, G256Operands ops, int M, int N, int K);
bool gemm256_fills(int M, int N);
bool gemm256_swiglu_fills(int M, int two_inter);
int gemm256_narrow_rounds(int M, int N);   // rounds of the chip that the all-narrow (256 x 128) grid of the plain form takes
// do the eight-phase kernels' 32-bit DMA offsets reach every element of N rows of K elements?
bool gemm8p_fits(int N, int K, int elem_bytes);
void gemm256_launch(G256Operands ops, const void *x, const void *W, half_t *y, int M, int N, int K, const half_t *bias,
                    const half_t *residual, const float *xscale, const float *wscale, hipStream_t st);
void gemm256_swiglu_launch(G256Operands ops, const void *x, const void *W, half_t *y, int M, int two_inter, int K, const float *xscale,
                           const float *wscale, hipStream_t st);
// QKV projection with RoPE + KV-cache append as its epilogue (gemm8p.cuh ROPE forms): q columns -> qkv (rotated), k / v columns ->
// the caches only
bool gemm256_qkv_rope_eligible(G256Operands ops, int M, int N, int K, const void *x, const void *W, const void *wscale, const void *qkv);
// rap: the epilogue's layer-invariant operands in DEVICE memory (prefill_token_table writes them); bias: the layer's QKV bias or null
void gemm256_qkv_rope_launch(G256Operands ops, const void *x, const void *W, half_t *qkv, int M, int N, int K, const float *xscale,
                             const float *wscale, const half_t *bias, const QkvRopeArgs *rap, int layer, hipStream_t st);
// fp16 image of int8 / int4 weights (row scales / group scales applied, one rounding): the operand of the prefill-sized
// projections that have no in-kernel de-quantising form; quant_linear.hip
int dequantize_weights_f16(int wbits, const void *wq, const half_t *scale, half_t *w16, int N, int K, int group, hipStream_t st);
// rows from which a weight-only projection runs as an MFMA-bound tiled GEMM (prefill) instead of split-K passes
constexpr int kWqPrefillRows = 192;
// bytes of fp16 scratch to reserve for linear_wq at M rows beside the split-K slabs (0: none); linear.hip
size_t linear_wq_dequant_bytes(int wbits, int M, int K, int N);
// [fp16 image | slabs] split of a caller workspace, as llmie_linear_workspace_bytes sizes it (a workspace too small for the image is
// all slabs); linear.hip
struct WqWorkspace {
    void *deq;
    size_t deq_bytes;
    SlabWs slabs;
};
WqWorkspace wq_workspace(int wbits, int M, int K, int N, void *workspace, size_t workspace_bytes);
// MXFP4 weight-only linear (mxfp4_linear.hip): launches what plan_linear_wq plans for bits = WF_MXFP4.  image: room for the fp16
// image of the matrix (the route from kWqPrefillRows rows), or null
constexpr int kMx4GemvRows = 8, kMx4MfmaRows = 64;
int dequantize_mxfp4_f16(const uint8_t *wq, const uint8_t *scale, half_t *w16, int N, int K, hipStream_t st);
int linear_mxfp4(const LinearOperands &o, const LinearScratch &s, hipStream_t st);
// quantised-weight (int8 / int4) decode GEMV on the K-split kernel; defined in linear.hip
struct GemvArgs;
bool ksplit_eligible(int M, int K, int wbits);
void gemv_q_launch(int wbits, int M, const GemvArgs &a, hipStream_t st);   // needs ksplit_eligible(M, K, wbits)
bool gemv_fp8_launch(int M, const GemvArgs &a, hipStream_t st);
// fp8 linear on the GEMV path (M <= 8, ksplit_eligible(M, K, 8)); optional fused norm prologue / SwiGLU epilogue; fp8_linear.hip
int linear_fp8_gemv(const LinearOperands &o, hipStream_t st);
// e4m3 weights: launches what plan_linear_fp8 plans.  The activation scratch (>= fp8_act_bytes(M, K), 256-byte aligned) receives the
// quantised activations, the slabs the split-K partial sums (engine: one slab area serves every projection); fp8_linear.hip
inline size_t fp8_align(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }
inline size_t fp8_act_bytes(int M, int K) {   // quantised activations + per-token scales
    return fp8_align(static_cast<size_t>(M) * K) + fp8_align(static_cast<size_t>(M) * sizeof(float));
}
int linear_fp8(const LinearOperands &o, const LinearScratch &s, hipStream_t st);
// weight-only int8/int4 linear with optional fused norm prologue / SwiGLU epilogue (quant_linear.hip): launches what
// plan_linear_wq plans -- at M >= kWqPrefillRows int8 through the eight-phase kernels' int8 form where eligible, else (and int4) a
// de-quantised fp16 image in the scratch's image area + the fp16 GEMM; without one those shapes keep the split-K passes
int linear_wq(int wbits, const LinearOperands &o, const LinearScratch &s, hipStream_t st);

// ---- packed-weight batch-decode projections (pk_gemm.cuh / pk_linear.hip): 1 <= M <= 32 rows on tile-packed weight images ----
enum : int { PKF_F16 = 16, PKF_I8 = 8, PKF_I4 = 4, PKF_FP8 = 108 };                 // = PK_F16 ... of pk_gemm.cuh
enum : int { PKE_PLAIN = 0, PKE_SWIGLU = 1 };
enum : int { PKX_X = 1, PKX_Y = 2, PKX_RES = 4 };                                    // operands in the x32 activation layout
size_t pk_packed_bytes(int wf, int N, int K, int swiglu);
size_t pk_packed_scale_bytes(int wf, int N, int K, int swiglu);   // int4: the group-scale image beside the weight image (else 0)
int pk_pack(int wf, const void *src, const void *src_scale, void *dst, void *dst_scale, int N, int K, int swiglu, hipStream_t st);
// image -> fp16 row-major [N, K] with the scales applied (fp16 / int8 / int4 images; scale = the caller's row / group-128 scales)
int pk_unpack_f16(int wf, const void *packed, const half_t *scale, half_t *w16, int N, int K, int swiglu, hipStream_t st);
bool pk_eligible(int wf, int M, int K, int N, int epi);
size_t pk_slab_floats(int wf, int M, int K, int N);
// one projection on a packed image: y = [swiglu]( rmsnorm(x + pre_bias) * gamma . W^T ) (+ residual); x32_flags: PKX_*; the slabs
// serve a K split over workgroups (null: none).  What pk_linear launches and pk_chain_add makes a phase of.
struct PkOperands {
    const half_t *x;
    const void *Wp, *scale;
    half_t *y;
    int K, N, epi, x32_flags;
    const half_t *residual, *gamma, *pre_bias;
    float eps;
    float *slab_ws;
    size_t slab_ws_floats;
};
int pk_linear(int wf, int M, const PkOperands &o, hipStream_t st);
int x32_convert(const half_t *src, half_t *dst, int M, int K, int to_x32, hipStream_t st);
// Persistent chain (pk_chain_kernel): up to 5 dependent phases -- each a pk_linear of the same format and row count whose x is an
// x32 image -- in ONE launch with grid barriers in between and the next phase's weight ring prefetched across each barrier.
// `sync`: pk_chain_sync_bytes() ZEROED bytes of this launch; `err`: the owner's device error word (non-zero after a barrier
// timed out).  A failed pk_chain_add leaves the chain unusable (the caller falls back to the launch sequence).
struct PkChain {
    int wf, M, nph, lds;
    bool ok;
    unsigned long long *stamps;   // diagnostic: device buffer [256][16] of phase-edge timestamps (null: none)
    alignas(16) unsigned char args[1024];
};
void pk_chain_begin(PkChain *ch, int wf, int M);
int pk_chain_add(PkChain *ch, int slot /* 0 = O, 1 = gate/up, 2 = down, 4 = next QKV */, const PkOperands &o);
int pk_chain_launch(PkChain *ch, unsigned *sync, unsigned *err, hipStream_t st);
size_t pk_chain_sync_bytes();

// The KV cache of one call, as every attention / append launch sees it.  Dense: k / v are [L, batch, kvh, max_seq_len, hs] and
// block_table is null.  Paged: block_table is [batch, max_pages] pool pages of 128 tokens and k / v are the pools
// [L, num_pages, kvh, 128, hs].  fp8: the caches are e4m3 bytes, stored = e4m3(x / scale) (the scales are 1 otherwise).
struct KvView {
    void *k, *v;
    const int32_t *block_table;
    int max_pages, num_pages;
    int fp8;
    float k_scale, v_scale;
};
inline KvView kv_dense(void *k, void *v) { return KvView{k, v, nullptr, 0, 0, 0, 1.f, 1.f}; }
// The position of a decode step: `step` on the host or *step_dev; ragged: step_dev is an array, step_dev[b] = context length of
// sequence b including this token
struct DecodePos {
    int step;
    const int32_t *step_dev;
    int ragged;
};
// ---- decode attention (attention_decode.hip): one pure host planner decides the launch, one launcher runs the plan ----
enum DecodeAttnKind : int { DA_REFUSED = 0, DA_SPLIT, DA_GENERIC };
enum DecodeAttnRefusal : int {
    DAREF_NONE = 0, DAREF_RAGGED_LENGTHS, DAREF_X32, DAREF_PAGES, DAREF_SLAB_ALIGNMENT, DAREF_E4M3_FORM, DAREF_E4M3, DAREF_WORKSPACE,
    DAREF_PAGED_GEOMETRY, DAREF_SLABS_GEOMETRY, DAREF_ROPE_GEOMETRY, DAREF_RAGGED_GEOMETRY, DAREF_GENERIC_SPAN, DAREF_WINDOW, DAREF_HEAD_SINK, DAREF_QK_NORM,
};
// One decode attention call as the planner sees it: geometry, position form, which optional operands are there, how far each
// pointer is from 16-byte alignment (address % 16 AFTER the layer offset; 0 for a null pointer), and the caller's scratch.
struct DecodeAttnCall {
    llmie_dtype dtype;                 // activations (and the native cache)
    bool kv_e4m3, scales_positive;     // e4m3 cache bytes; both of its scales > 0
    int head_size, head_num, kv_head_num, batch, max_seq_len;
    int step;                          // host position (used when !step_dev)
    bool step_dev, ragged;             // *step_dev / one context length per sequence
    bool bias, rope, tickets, slabs, paged, out_x32;
    int max_pages, num_pages;          // paged
    unsigned mis_qkv, mis_bias, mis_k, mis_v;
    unsigned mis_slab, mis_wf, mis_wh8, slab_stride_mod4;   // slabs: slab % 16, wf % 16, wh % 8, (M * N) % 4
    bool workspace;
    size_t workspace_bytes;
    int window, sinks;                 // sliding window (0: full attention, sinks then 0) and sink tokens
    bool head_sink;                    // a learned sink logit per query head (device fp32 [head_num]) joins every softmax
    bool qk_norm;                      // per-head RMSNorm of q and k in front of RoPE (device gammas [head_size] each)
};
struct DecodeAttnPlan {
    int kind, refusal;                 // DecodeAttnKind, DecodeAttnRefusal of DA_REFUSED
    // DA_SPLIT: the instantiation decode_attn_split_kernel<T, hs, rep, 4, 8, e4m3 ? fp8kv_t : T>, chunks per workgroup, tokens per
    // workgroup (cpw chunks), grid (splits, kv heads, batch), partial slots per (sequence, head), the merge launch (none: one
    // split, or the in-launch merge by tickets)
    int hs, rep;
    bool e4m3;
    int cpw, chunk, grid[3], max_splits_ws;
    int window, sinks;                 // window > 0: the windowed instantiation; grid x counts live spans (attn_live_chunks)
    bool head_sink;                    // the SINK instantiation of the same launches (same grid, slots and merge)
    bool qk_norm;                      // the QKN instantiation of the split kernel (same grid, slots and merge)
    bool merge;
    int merge_grid[2], merge_block;
    // DA_GENERIC: grid (heads, batch), dynamic LDS
    size_t lds_bytes;
    size_t workspace_bytes;            // what the kind needs of the caller's scratch
};
DecodeAttnPlan plan_decode_attn(const DecodeAttnCall &c);
int decode_attn_refuse(const DecodeAttnCall &c, const DecodeAttnPlan &p);   // sets the refusal's error text, returns its error code
struct DecodeAttnShape {
    int batch, head_num, kv_head_num, head_size, max_seq_len;
    llmie_dtype dtype;
};
// operands of a call beside the cache and the position.  rope: [max_pos][head_size/2] (cos,sin) table fused in front, or null;
// tickets: [batch, kvh] zeroed arrival counters = in-launch merge, null = merge kernel; qkv_slabs: q/k/v are read from the QKV
// projection's split-K slabs (qkv unused) with qkv_scale; out_x32: out is the x32 activation image (batch <= 32), not [batch, H];
// window > 0: sliding-window attention with `sinks` sink tokens (include/llmie.h), 0 = full attention; head_sink: this layer's
// learned sink logits, device fp32 [head_num], or null; q_gamma / k_gamma: this layer's QK-norm gammas, device [head_size] each in
// the activation type, or both null, with qk_eps
struct DecodeAttnIo {
    const void *qkv, *qkv_bias;
    void *out, *workspace;
    size_t workspace_bytes;
    const float2 *rope;
    int rot_dim;
    int32_t *tickets;
    const SplitKSlabs *qkv_slabs;
    const SlabScale *qkv_scale;
    int out_x32;
    int window, sinks;
    const float *head_sink;
    const void *q_gamma, *k_gamma;
    float qk_eps;
};
// decode attention of one layer with bias, RoPE and the KV append fused in front: plan, refuse or launch
int decoder_mha_rope(const DecodeAttnShape &g, const DecodeAttnIo &io, const KvView &kv, const DecodePos &pos, int layer, hipStream_t st);

// prefill attention (RoPE + KV append + flash attention) on the packed QKV buffer; prefill.hip: one pure host planner decides the
// launch, one launcher runs the plan
struct PrefillAttnPlan {
    int q_rows, waves, row_tiles;   // prefill_flash_kernel<128, kv_e4m3, waves, row_tiles>: q_rows query rows per workgroup
    bool kv_e4m3;
    int grid[3];                    // (query tiles of the longest sequence, head_num, batch)
    bool rope_append;               // prefill_rope_append_kernel runs first (else the QKV projection's epilogue did RoPE + the append)
    int window, sinks;              // window > 0: the windowed instantiation (sliding window + sink tokens), 0: full causal attention
    bool head_sink;                 // the SINK instantiation of the same form: a learned sink logit per query head joins every row's softmax
    bool tree;                      // the TREE instantiations of both launches: the chunk of every sequence is a draft tree (q64w4t1 only)
};
// The draft tree of a prefill attention call (include/llmie.h, llmie_decoder_set_tree): device arrays [batch, stride] as
// llmie_spec_tree_prepare leaves them, or all null / 0
struct PrefillTree {
    const int32_t *depth;
    const uint64_t *anc;
    int stride;
};
// QK-norm of a prefill attention call (include/llmie.h, llmie_qk_norm): this layer's gammas, device fp16 [128] each, or both null; the
// RoPE + append launch normalises q and k in front of the rotation (so the plan must have rope_append, and the layer no QKV bias)
struct PrefillQkNorm {
    const half_t *q_gamma, *k_gamma;
    float eps;
};
PrefillAttnPlan plan_prefill_attn(int batch, int max_q_len, int head_num, bool kv_e4m3, bool rope_done, int window = 0, int sinks = 0,
                                  bool tree = false);
int prefill_attention_f16(const PrefillAttnPlan &plan, const KvView &kv, half_t *qkv, const half_t *qkv_bias, half_t *out,
                          const int32_t *cum_seqlens, const int32_t *history_len, const float2 *rope, int layer, int num_tokens,
                          int kv_head_num, int max_seq_len, int rotary_dim, hipStream_t st,
                          const float *head_sink = nullptr /* plan.head_sink: this layer's device fp32 [head_num] */,
                          const PrefillQkNorm &qkn = PrefillQkNorm{nullptr, nullptr, 0.f},
                          const PrefillTree &tree = PrefillTree{nullptr, nullptr, 0});
// short prefills: slab consumer of the QKV projection with RoPE + KV-cache append folded in (q -> qkv, k / v -> the caches only)
bool splitk_finalize_qkv_rope_eligible(const SplitKSlabs &sk, int head_size, const void *qkv, const void *bias);
int splitk_finalize_qkv_rope(const SplitKSlabs &sk, const SlabScale &sc, half_t *qkv, const half_t *qkv_bias, const KvView &kv,
                             const int32_t *cum_seqlens, const int32_t *history_len, const float2 *rope, int layer, int batch, int head_num,
                             int kv_head_num, int max_seq_len, int rotary_dim, hipStream_t st);
// tok_b[t] / tok_tpos[t] = sequence / cache position (history + position) of packed token t: operands of that epilogue
// (also copies `args` -- whose tok_b / tok_tpos it fills in -- to args_dev)
int prefill_token_table(const int32_t *cum_seqlens, const int32_t *history_len, int batch, int num_tokens, int32_t *tok_b, int32_t *tok_tpos,
                        QkvRopeArgs args, QkvRopeArgs *args_dev, hipStream_t st);

// ---- mixture-of-experts FFN (moe.hip): one pure host planner decides the launches, one launcher runs the plan by stages ----
// A call is three structs, from the C entry to the kernel launch.  What the planner reads and nothing else:
struct MoeCall {
    int rows, H, Ie, E, k;
    unsigned flags;                    // LLMIE_MOE_*
    llmie_weight_format format;        // of the experts: LLMIE_W_F16 or LLMIE_W_MXFP4
    bool ex;                           // the _ex epilogue is live: an expert bias, or the clamped act
};
inline bool moe_epilogue_live(const llmie_moe_experts &e) { return e.gate_up_bias || e.down_bias || e.act != LLMIE_MOE_ACT_SWIGLU; }
enum MoeRoute : int { MOE_GEMV = 0, MOE_GROUPED = 1 };
// the workspace carve: byte offsets behind the plan's 256-byte header; tile_* and d are 0-sized on the GEMV route
struct MoeCarve {
    size_t expert, weight, act, tile_expert, tile_pairs, d, bytes;
};
// What plan_moe answers for a MoeCall (which it keeps): the launcher, the plan text and the workspace rule read this and nothing else
struct MoePlan {
    MoeCall call;
    int route, rt, tiles, pairs;       // MoeRoute; grouped: the tile height 16 * rt and the host bound of the tile count
    int route_grid, gate_up_grid[2], down_grid[2], combine_grid[2];
    // the instantiations.  GEMV route: XC of moe_gemv_*_kernel (fp16 experts) or the (XB, KW) index of moe_mx4_gemv_*_kernel, for
    // the gate/up launch (K = H) and the down launch (K = Ie).  ex: the EX instantiations of the fp16 expert kernels
    int gate_up_cfg, down_cfg;
    bool ex;
    MoeCarve ws;
};
// the operands of a call: x, resid (or null) and y are [rows, H]; x and y may be one buffer
struct MoeOperands {
    const void *x, *resid;
    void *y;
    const llmie_moe_experts *experts;
    void *workspace;
    size_t workspace_bytes;
    llmie_dtype dtype;
};
// a call that passed every check, planned and carved: the plan and the kernel argument structs of moe.hip
struct MoePrepared {
    MoePlan plan;
    alignas(16) unsigned char args[256];
};
enum : unsigned { MOE_STAGE_ROUTE = 1, MOE_STAGE_GATE_UP = 2 /* grouped route: with the plan launch */, MOE_STAGE_DOWN = 4 /* with combine */,
                  MOE_STAGE_ALL = 7 };
// would llmie_moe_ffn / _ex take this shape and these flags?  The code and the message under `who`, and the plan (null: not wanted);
// nothing is launched
int moe_call_check(const char *who, const MoeCall &c, MoePlan *plan = nullptr);
int moe_experts_ok(const char *who, const llmie_moe_experts *ex);   // a descriptor's own checks: format, pointers, scales, act, alignment
// every check of llmie_moe_ffn_ex under the name `who`, then plan, carve and fill the kernel arguments.  shape: rows .. flags of the
// call (format and ex follow the descriptor).  planned: a plan made ahead for this very shape (the engine's, once per forward call),
// taken where the descriptor's format and epilogue are the ones it was made for; null: none
int moe_prepare(const char *who, const MoeCall &shape, const MoeOperands &o, const MoePlan *planned, MoePrepared *out);
int moe_launch(const MoePrepared &m, unsigned stages, hipStream_t st);   // nothing but the launches of these stages

// ---- the sampler family (sampling_params.hip, spec_decode.hip, topk_sampling.hip and the LM-head entries of engine.hip) ----
// A call is a few structs that say what its operands are, from the C entry to the kernel launch: a new operand is added to ONE struct,
// at the entries that fill it and at the launch that reads it.  The rows: logits [batch, vocab], one llmie_sampling_params per row
struct SampleRows {
    const void *logits;
    int batch, vocab;
    llmie_dtype dtype;
    const llmie_sampling_params *params;
    int end_id;
};
struct SampleState {   // the per-sequence state a call moves
    int32_t *history;
    int history_stride;
    int32_t *history_len;
    int history_append;
    int32_t *seq_len;
    uint8_t *finished;
};
struct SamplePos { int step; const int32_t *step_dev; };   // the Philox step: on the host, or *step_dev (which the tail may advance)
struct SampleOut { int32_t *out_id; float *out_logprob /* or null */; };
// The optional tail of a decode step: next_hidden[b] = embed[out_id[b]] (rows of `hidden` elements), and *step_dev += 1 by the last
// row to finish (`ticket` = one zeroed word).  All zero: none.
struct SampleTail {
    const void *embed;
    void *next_hidden;
    int hidden, advance;
    unsigned *ticket;
};
struct SampleWs { void *p; size_t bytes; };
// The host-side checks of llmie_sample_logits under the name `entry`; `out` is where the call writes its tokens.  The workspace is
// the caller's to size: sample_workspace_check is the one rule -- present, `need` bytes, 16-byte aligned -- and `query` the size
// query its message names (null: none).  sample_ext_check says whether an extension struct needs the EXT kernels: the launch gets
// ext != nullptr exactly then.
int sample_logits_check(const char *entry, const SampleRows &rows, const SampleState &state, const void *out);
int sample_workspace_check(const char *entry, SampleWs ws, size_t need, const char *query);
int sample_ext_check(int batch, int vocab, const llmie_sampling_ext *ext, bool *active, const char *entry = "sample_logits_ext");
size_t sample_logits_ws_row(int vocab);   // uint32 words of workspace per row
int sample_logits_launch(const SampleRows &rows, const SampleState &state, const SamplePos &pos, const SampleOut &out, const SampleTail &tail,
                         SampleWs ws, const llmie_sampling_ext *ext, hipStream_t st);
// fp16 / fp32 -> f(TypeTag<T>{}); (dtype, extension active) -> the <T, EXT> instantiation of a sampler kernel:
// f(TypeTag<T>{}, std::bool_constant<EXT>{}).  A kernel launch is written once, inside the callable.
template <class T> struct TypeTag { using type = T; };
template <class F> void dtype_dispatch(llmie_dtype dtype, F f) {
    if (dtype == LLMIE_F16) f(TypeTag<half_t>{});
    else f(TypeTag<float>{});
}
template <class F> void sample_dispatch(llmie_dtype dtype, bool ext, F f) {
    dtype_dispatch(dtype, [&](auto type) {
        if (ext) f(type, std::true_type{});
        else f(type, std::false_type{});
    });
}
// fused tail of a decode step (topk_sampling.hip): round 1 of the top-k alone, and round 2 + sampling + SampleTail in one launch
struct TopkOperands {   // llmie_topk's: round 1 -> (tmp_ids, tmp_vals) [rows, bpr * K] -> round 2 -> (ids, vals) [rows, K]
    int32_t *tmp_ids;
    void *tmp_vals;
    int32_t *ids;
    void *vals;
    int K, bpr;
};
int topk_round1_only(const void *probs, const TopkOperands &tk, int rows, int vocab, llmie_dtype dtype, hipStream_t st);
int decode_tail(const TopkOperands &tk, const SampleRows &rows, const SampleState &state, const SamplePos &pos, int32_t *out_id,
                const SampleTail &tail, hipStream_t st);

}  // namespace llmie
