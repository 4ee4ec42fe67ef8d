// Fused decoder engine: llmie_decoder_* and llmie_lm_head_sample.
// This is what LlamaSelfDecoder<T>::forward (self_decoder.cpp:24-122) and
// LlamaModel<T>::generateNextToken / LMHeadAndTopKSample (llama.cpp:219-318) run on.
//
// Differences from the reference's control flow, none of them numerical beyond rounding:
//   * zero allocation / zero synchronisation per token: all scratch lives in one caller-owned
//     workspace carved at create time (the reference mallocs+frees 5 buffers and syncs the
//     device ~10x per layer, self_attention.cpp:29-45,150);
//   * the position can live in device memory (step_dev) so the whole token step can be captured
//     once in a hipGraph and replayed;
//   * SwiGLU is the epilogue of the gate/up GEMV and the second residual add is the epilogue of
//     the down GEMV (reference: launchSiluAndMul / launchAddResidual as separate kernels).
#include "llmie_internal.h"

#include <cmath>
#include <cstdlib>
#include <new>
#include <vector>

using namespace llmie;

struct llmie_decoder {
    llmie_decoder_config cfg;
    std::vector<llmie_layer_weights> layers;
    int H, QKV, I;
    size_t esz;
    // workspace carve-up
    char *resid, *qkv, *mha, *act, *gu;
    void *attn_ws;
    size_t attn_ws_bytes;
    float2 *rope_table;  // [max_seq_len][head_size/2] (cos, sin), host-computed at create
    void *fp8_ws;        // LLMIE_W_FP8 engines: activation quantisation + split-K scratch of llmie_linear_fp8
    size_t fp8_ws_bytes;
    SlabWs slab_ws;      // fp32 slabs of the split-K projections (batch path, row-major engines)
    unsigned *tail_ticket = nullptr;   // one zeroed word: arrival ticket of the fused decode tail (llmie_lm_head_sample_next)
    // packed-weight batch path (gemv_max < batch <= 32): tile-packed images of the four matrices of every layer (built once at
    // create time into the caller's workspace: the MI355X's 288 GB buy a second, stream-friendly copy of the weights), the
    // activations between the packed kernels in the x32 layout, and the split-K slabs of the down projection
    struct PackedLayer {
        const unsigned char *qkv, *o, *gate_up, *down;
        const void *sc[4];   // int4: packed group-scale images of the four matrices (else null: the caller's row scales are used)
    };
    std::vector<PackedLayer> packed;
    int pk_wf = 0;                    // PKF_* of the engine's weight format, 0 = no packed path
    bool packed_only = false;         // LLMIE_DEC_PACKED_ONLY: the row-major matrices are gone, every path reads the images
    half_t *hx = nullptr, *actx = nullptr;   // x32 images: residual stream [32, H], SwiGLU output [32, I]
    half_t *mhax = nullptr;                  // x32 image of the attention output [32, H]
    float *pk_slab = nullptr;
    size_t pk_slab_floats = 0;
    // persistent chain launches of the packed path: one zeroed block of barrier counters per layer, one device error word
    unsigned char *pk_base = nullptr;   // first byte of the packed images (the workspace area carved for them)
    unsigned *pk_sync = nullptr, *pk_err = nullptr;
    unsigned long long *pk_stamps = nullptr;   // diagnostic: phase-edge timestamps of the LAST chain launch of a step
    // per-request adapters (llmie_decoder_lora_attach): the device slot table, the slot of every batch row / sequence, the attach
    // call's scratch.  table != nullptr: every forward / prefill entry runs the lora sequence
    struct Lora {
        const void *table = nullptr;
        int slots = 0;
        const int32_t *seq_slot = nullptr;
        void *ws = nullptr;
        size_t ws_bytes = 0;
    } lora;
    // mixture-of-experts FFN (llmie_decoder_moe_attach): per layer the router / expert matrices (router == nullptr: the layer keeps its
    // dense FFN), the expert geometry and the attach call's scratch.  layers non-empty: every forward / prefill entry runs the moe sequence
    struct Moe {
        std::vector<llmie_moe_experts> layers;   // (llmie_decoder_moe_attach: fp16 descriptors without biases, plain SwiGLU)
        // every call's description but its rows: the expert geometry, the attach flags, the experts' format (the engine's own weight
        // format is cfg.wfmt) and the first sparse layer's epilogue
        MoeCall call{};
        void *ws = nullptr;
        size_t ws_bytes = 0;
        bool on() const { return !layers.empty(); }
    } moe;
    // sliding-window attention (llmie_decoder_set_window): the window of every layer (0 = full attention; empty: none set) and the
    // sink tokens; read where a call's attention launches are planned
    std::vector<int> layer_window;
    int sinks = 0;
    int window_of(int layer) const { return layer_window.empty() ? 0 : layer_window[layer]; }
    // learned per-head sink logits (llmie_decoder_set_head_sinks): the caller's device array [num_layers, head_num] of fp32, or null;
    // read where a call's attention launches are planned, like the window
    const float *head_sinks = nullptr;
    const float *head_sink_of(int layer) const { return head_sinks ? head_sinks + static_cast<size_t>(layer) * cfg.head_num : nullptr; }
    // QK-norm (llmie_decoder_set_qk_norm): the caller's device arrays [num_layers, head_size] of fp16, or both null, and eps; read
    // where a call's attention launches are built, like the head sinks
    const half_t *q_gammas = nullptr, *k_gammas = nullptr;
    float qk_eps = 0.f;
    const half_t *q_gamma_of(int layer) const { return q_gammas ? q_gammas + static_cast<size_t>(layer) * cfg.head_size : nullptr; }
    const half_t *k_gamma_of(int layer) const { return k_gammas ? k_gammas + static_cast<size_t>(layer) * cfg.head_size : nullptr; }
    // draft tree (llmie_decoder_set_tree): the caller's device arrays [batch, tree_stride] as llmie_spec_tree_prepare leaves them, or
    // null / null / 0; read by every prefill launch that is built while they are set (the decode entries do not know them)
    const int32_t *tree_depth = nullptr;
    const uint64_t *tree_anc = nullptr;
    int tree_stride = 0;
    // profiling (eager only)
    bool profiling = false;
    std::vector<hipEvent_t> ev;      // pairs: start, stop
    std::vector<int> ev_op;          // op kind of pair i
    size_t ev_used = 0;
};

// brackets one engine op with events when profiling
struct OpTimer {
    llmie_decoder *d;
    hipStream_t st;
    bool on;
    size_t idx;
    OpTimer(llmie_decoder *dec, int op, llmie_stream s) : d(dec), st(as_stream(s)), on(false), idx(0) {
        if (d->profiling && d->ev_used + 1 <= d->ev_op.size()) {
            idx = d->ev_used++;
            d->ev_op[idx] = op;
            on = hipEventRecord(d->ev[2 * idx], st) == hipSuccess;
        }
    }
    ~OpTimer() {
        if (on) (void)hipEventRecord(d->ev[2 * idx + 1], st);
    }
};
#define TIMED(op, expr)                 \
    do {                                \
        OpTimer _t(dec, op, stream);    \
        rc = (expr);                    \
    } while (0);                        \
    if (rc) return rc

static size_t align_up(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

static bool config_ok(const llmie_decoder_config *c) {
    if (!c) return false;
    if (c->head_num <= 0 || c->kv_head_num <= 0 || c->head_size <= 0 || c->inter_size <= 0 ||
        c->num_layers <= 0 || c->max_seq_len <= 0 || c->max_batch <= 0)
        return false;
    if (c->head_num % c->kv_head_num) return false;
    if (c->rotary_dim <= 0 || c->rotary_dim % 2) return false;
    if (c->dtype != LLMIE_F32 && c->dtype != LLMIE_F16) return false;
    if (c->dtype == LLMIE_F32 && c->wfmt != LLMIE_W_F32) return false;
    if (c->dtype == LLMIE_F16 && c->wfmt == LLMIE_W_F32) return false;
    // MXFP4: blocks of 32 along K of every projection (K = hidden size or inter_size)
    if (c->wfmt == LLMIE_W_MXFP4 && ((c->head_num * c->head_size) % 32 || c->inter_size % 32)) return false;
    if (c->kv_fmt != LLMIE_KV_NATIVE && c->kv_fmt != LLMIE_KV_FP8) return false;
    if (c->flags & ~(LLMIE_DEC_NO_PACKED_COPY | LLMIE_DEC_PACKED_ONLY)) return false;
    if ((c->flags & LLMIE_DEC_NO_PACKED_COPY) && (c->flags & LLMIE_DEC_PACKED_ONLY)) return false;
    if (c->kv_fmt == LLMIE_KV_FP8) {  // e4m3 cache: fp16 engines on the fused attention kernels only
        const int rep = c->head_num / c->kv_head_num;
        if (c->dtype != LLMIE_F16 || (c->head_size != 128 && c->head_size != 64) || (rep != 1 && rep != 2 && rep != 4)) return false;
    }
    return true;
}

struct Carve {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off += align_up(bytes);
        return o;
    }
};

// Largest decode batch on the GEMV path.  Its dot products are VALU work that grows with the batch while a packed-weight
// (MFMA) step is nearly flat, so the switch sits at the measured crossover (MI355X, 7B, ctx 512, tokens/s GEMV vs packed,
// round 2): fp16 b3 924 / 905, b4 1140 / 1186; int8 b2 918 / 828, b3 1172 / 1211; fp8 b2 804 / 720, b3 1009 / 1044;
// int4 (ctx 2048) b1 460 / 442, b2 710 / 812.  Re-measured at the end of round 3 (the GEMV had gained ~10 % since: four rows per
// iteration, two rows per instruction for int4): fp16 b4 1302 / 1203, b5 1516 / 1452, b6 1710 / 1731; int8 b3 1240 / 1244, b4 1477 /
// 1637; fp8 b3 1036 / 1171; int4 (ctx 512) b2 1012 / 939.
static int gemv_max_batch(llmie_weight_format wfmt) {
    switch (wfmt) {
        case LLMIE_W_F16: return 5;
        case LLMIE_W_INT8: return 2;
        case LLMIE_W_FP8: return 2;
        case LLMIE_W_INT4: return 2;
        default: return 4;
    }
}

// The batches an engine with tile-packed images decodes on the packed kernels: above the GEMV crossover (a LLMIE_DEC_PACKED_ONLY
// engine: every batch), up to 32 rows, fp8 16.  fp8: the per-launch activation quantisation (amax + conversions of the whole register
// slice) costs ~5 us at 32 rows; measured (7B, ctx 512, tokens/s packed vs split-K batch path): b8 2705 / 2506, b16 5011 / 4450,
// b24 5656 / 5833, b32 7103 / 7120
static int packed_rows_max(const llmie_decoder_config &c) { return c.wfmt == LLMIE_W_FP8 ? 16 : 32; }
static bool packed_batch(const llmie_decoder_config &c, int batch) {
    return (batch > gemv_max_batch(c.wfmt) || (c.flags & LLMIE_DEC_PACKED_ONLY)) && batch <= packed_rows_max(c);
}

// weight format / shapes the packed batch path covers; max rows it will be asked for
static int packed_wf(const llmie_decoder_config *c) {
    if (c->dtype != LLMIE_F16) return 0;
    const int wf = c->wfmt == LLMIE_W_F16 ? PKF_F16
                   : (c->wfmt == LLMIE_W_INT8 ? PKF_I8 : (c->wfmt == LLMIE_W_FP8 ? PKF_FP8 : (c->wfmt == LLMIE_W_INT4 && c->int4_group == 128 ? PKF_I4 : 0)));
    const bool only = (c->flags & LLMIE_DEC_PACKED_ONLY) != 0;   // the images are all there is: built whatever the batch
    if (!wf || (c->flags & LLMIE_DEC_NO_PACKED_COPY)) return 0;
    // no second copy of the weights where no batch up to max_batch takes the packed path; a packed-only engine needs it to take all
    const int rows_max = packed_rows_max(*c);
    if (!packed_batch(*c, only || c->max_batch < rows_max ? c->max_batch : rows_max)) return 0;
    const int H = c->head_num * c->head_size, QKV = (c->head_num + 2 * c->kv_head_num) * c->head_size, I = c->inter_size;
    const int m = c->max_batch < 32 ? c->max_batch : 32;
    if (H % 32 || I % 32) return 0;
    if (!pk_eligible(wf, m, H, QKV, PKE_PLAIN) || !pk_eligible(wf, m, H, H, PKE_PLAIN) || !pk_eligible(wf, m, H, 2 * I, PKE_SWIGLU) ||
        !pk_eligible(wf, m, I, H, PKE_PLAIN))
        return 0;
    return wf;
}
// why a LLMIE_DEC_PACKED_ONLY config without a packed format is refused (create and the two plan queries)
static const char *packed_only_refusal(const llmie_decoder_config *c) {
    return c->wfmt == LLMIE_W_MXFP4 ? "decoder_create: LLMIE_DEC_PACKED_ONLY is not available for MXFP4 weights (no packed image is built)"
                                    : "decoder_create: LLMIE_DEC_PACKED_ONLY needs max_batch <= 32 (fp8: 16) and shapes / a format the packed kernels take";
}
struct PackedCarve {
    size_t per_layer[4], layer_bytes, hx, actx, mhax, slab, sync, total;
};
static PackedCarve packed_carve(const llmie_decoder_config *c, int wf) {
    PackedCarve p{};
    if (!wf) return p;
    const int H = c->head_num * c->head_size, QKV = (c->head_num + 2 * c->kv_head_num) * c->head_size, I = c->inter_size;
    // (each matrix: weight image, then -- int4 -- its group-scale image)
    p.per_layer[0] = align_up(pk_packed_bytes(wf, QKV, H, 0)) + align_up(pk_packed_scale_bytes(wf, QKV, H, 0));
    p.per_layer[1] = align_up(pk_packed_bytes(wf, H, H, 0)) + align_up(pk_packed_scale_bytes(wf, H, H, 0));
    p.per_layer[2] = align_up(pk_packed_bytes(wf, 2 * I, H, 1)) + align_up(pk_packed_scale_bytes(wf, 2 * I, H, 1));
    p.per_layer[3] = align_up(pk_packed_bytes(wf, H, I, 0)) + align_up(pk_packed_scale_bytes(wf, H, I, 0));
    p.layer_bytes = p.per_layer[0] + p.per_layer[1] + p.per_layer[2] + p.per_layer[3];
    p.hx = align_up(static_cast<size_t>(H) * 64);
    p.actx = align_up(static_cast<size_t>(I) * 64);
    p.mhax = p.hx;
    const int m = c->max_batch < 32 ? c->max_batch : 32;
    size_t sl = 0;
    for (int mm = 1; mm <= m; ++mm) {
        const size_t f = pk_slab_floats(wf, mm, I, H);
        sl = f > sl ? f : sl;
    }
    p.slab = align_up(sl * sizeof(float) + 16);
    p.sync = align_up(static_cast<size_t>(c->num_layers) * pk_chain_sync_bytes()) + 256;   // barrier counters per layer + the error word
    p.total = p.layer_bytes * c->num_layers + p.hx + p.actx + p.mhax + p.slab + p.sync;
    return p;
}
// fp32 floats of split-K slab scratch the engine's projections can need at up to `rows` activation rows (0: none)
static size_t engine_slab_floats(const llmie_decoder_config *c, int rows) {
    int wbits;
    switch (c->wfmt) {
        case LLMIE_W_F16: wbits = 16; break;
        case LLMIE_W_INT8: wbits = 8; break;
        case LLMIE_W_INT4: wbits = 4; break;
        case LLMIE_W_FP8: wbits = WF_FP8; break;
        case LLMIE_W_MXFP4: wbits = 0; break;   // no MXFP4 route takes slabs; the LM head (another format) below may
        default: return 0;
    }
    if (c->dtype != LLMIE_F16) return 0;
    const int H = c->head_num * c->head_size, QKV = (c->head_num + 2 * c->kv_head_num) * c->head_size, I = c->inter_size;
    const int shapes[5][2] = {{H, QKV}, {H, H}, {H, 2 * I}, {I, H}, {H, c->vocab_size}};   // (the LM head of llmie_lm_head_sample)
    size_t m = 0;
    // every row count up to `rows` (the plan -- kernel form, K slices -- changes with it); the LM head may come in a different
    // format than the layers (fp16 beside int8 / fp8 layers): all formats for that shape
    const int lm_bits[4] = {16, 8, 4, WF_FP8};
    for (int r = 1; r <= rows; ++r) {
        for (int i = 0; i < 4 && wbits; ++i) {
            const size_t f = linear_splitk_ws_floats(wbits, r, shapes[i][0], shapes[i][1]);
            m = f > m ? f : m;
        }
        for (int b : lm_bits) {
            const size_t f = linear_splitk_ws_floats(b, r, shapes[4][0], shapes[4][1]);
            m = f > m ? f : m;
        }
    }
    return m;
}

// the engine's workspace: offsets of its areas, in carve order
struct EngineCarve {
    size_t resid, qkv, mha, attn_out, act, gu, attn_ws, rope_table, tail_ticket, fp8_ws, packed, slabs, total;
};
static EngineCarve carve(const llmie_decoder_config *c) {
    const size_t e = c->dtype == LLMIE_F16 ? 2 : 4;
    const size_t B = c->max_batch, H = static_cast<size_t>(c->head_num) * c->head_size;
    const size_t QKV = static_cast<size_t>(c->head_num + 2 * c->kv_head_num) * c->head_size;
    const size_t I = c->inter_size;
    Carve k;
    EngineCarve o;
    o.resid = k.take(B * H * e);
    o.qkv = k.take(B * QKV * e);
    o.mha = k.take(B * H * e);
    o.attn_out = k.take(B * H * e);   // (no sequence uses it any more; kept: the workspace size is part of what callers allocate)
    o.act = k.take(B * I * e);
    o.gu = k.take(B * 2 * I * e);     // gate_up (unfused paths)
    o.attn_ws = k.take(llmie_decoder_mha_workspace_bytes(c->max_batch, c->head_num, c->head_size, c->max_seq_len));
    o.rope_table = k.take(static_cast<size_t>(c->max_seq_len) * (c->head_size / 2) * sizeof(float2));
    o.tail_ticket = k.take(256);      // arrival ticket word of the fused decode tail
    const int kmax = c->inter_size > static_cast<int>(H) ? c->inter_size : static_cast<int>(H);
    // fp8: three activation-quantisation units (normed input, attention output, SwiGLU output), see DecodeStep::splitk
    o.fp8_ws = k.take(c->wfmt == LLMIE_W_FP8 ? 3 * llmie_linear_fp8_workspace_bytes(c->max_batch, kmax, 0) : 256);
    o.packed = k.take(packed_carve(c, packed_wf(c)).total + 256);   // packed weight images + x32 activations + slabs
    o.slabs = k.take(engine_slab_floats(c, c->max_batch) * sizeof(float) + 256);   // split-K slabs of the row-major paths
    o.total = k.off;
    return o;
}

extern "C" size_t llmie_decoder_workspace_bytes(const llmie_decoder_config *cfg) {
    if (!config_ok(cfg)) return 0;
    return carve(cfg).total;
}

// (re)build the tile-packed images of every layer from row-major matrices (create; llmie_decoder_repack)
static int pack_layers(llmie_decoder *d, const llmie_layer_weights *layers, hipStream_t st) {
    const llmie_decoder_config *cfg = &d->cfg;
    const PackedCarve pc = packed_carve(cfg, d->pk_wf);
    unsigned char *pb = d->pk_base;
    const int H = d->H, QKV = d->QKV, I = d->I;
    d->packed.resize(cfg->num_layers);
    int prc = LLMIE_OK;
    for (int l = 0; l < cfg->num_layers && prc == LLMIE_OK; ++l) {
        unsigned char *q = pb + static_cast<size_t>(l) * pc.layer_bytes;
        unsigned char *po = q + pc.per_layer[0], *pg = po + pc.per_layer[1], *pd = pg + pc.per_layer[2];
        const llmie_layer_weights &w = layers[l];
        const bool i4 = d->pk_wf == PKF_I4;
        unsigned char *sq = q + align_up(pk_packed_bytes(d->pk_wf, QKV, H, 0)), *so = po + align_up(pk_packed_bytes(d->pk_wf, H, H, 0));
        unsigned char *sg = pg + align_up(pk_packed_bytes(d->pk_wf, 2 * I, H, 1)), *sd = pd + align_up(pk_packed_bytes(d->pk_wf, H, I, 0));
        prc = pk_pack(d->pk_wf, w.qkv.data, i4 ? w.qkv.scale : nullptr, q, i4 ? sq : nullptr, QKV, H, 0, st);
        if (!prc) prc = pk_pack(d->pk_wf, w.o.data, i4 ? w.o.scale : nullptr, po, i4 ? so : nullptr, H, H, 0, st);
        if (!prc) prc = pk_pack(d->pk_wf, w.gate_up.data, i4 ? w.gate_up.scale : nullptr, pg, i4 ? sg : nullptr, 2 * I, H, 1, st);
        if (!prc) prc = pk_pack(d->pk_wf, w.down.data, i4 ? w.down.scale : nullptr, pd, i4 ? sd : nullptr, H, I, 0, st);
        d->packed[l] = llmie_decoder::PackedLayer{q, po, pg, pd, {i4 ? sq : nullptr, i4 ? so : nullptr, i4 ? sg : nullptr, i4 ? sd : nullptr}};
    }
    return prc;
}

// Weights changed in place (or, for a LLMIE_DEC_PACKED_ONLY engine, new weights altogether): rebuild the tile-packed images from
// `layers` (row-major matrices in the engine's format; scale / bias / gamma pointers replace the ones given at create).  Enqueued
// on `stream`; engines without images just take the new pointers.
extern "C" int llmie_decoder_repack(llmie_decoder *dec, const llmie_layer_weights *layers, llmie_stream stream) {
    LLMIE_REQUIRE(dec && layers, "decoder_repack: NULL pointer");
    for (int l = 0; l < dec->cfg.num_layers; ++l) {
        const llmie_layer_weights &w = layers[l];
        LLMIE_REQUIRE(w.attn_norm_gamma && w.ffn_norm_gamma && w.qkv.data && w.o.data && w.gate_up.data && w.down.data,
                      "decoder_repack: layer %d has a NULL weight", l);
    }
    int rc = LLMIE_OK;
    if (dec->pk_wf) rc = pack_layers(dec, layers, as_stream(stream));
    if (rc) return rc;
    dec->layers.assign(layers, layers + dec->cfg.num_layers);
    if (dec->packed_only)
        for (llmie_layer_weights &w : dec->layers) w.qkv.data = w.o.data = w.gate_up.data = w.down.data = nullptr;
    return LLMIE_OK;
}

extern "C" size_t llmie_decoder_resident_weight_bytes(const llmie_decoder_config *cfg) {
    if (!config_ok(cfg)) return 0;
    const size_t H = static_cast<size_t>(cfg->head_num) * cfg->head_size, QKV = static_cast<size_t>(cfg->head_num + 2 * cfg->kv_head_num) * cfg->head_size;
    const size_t I = cfg->inter_size, elems = QKV * H + H * H + 3 * H * I, rows = QKV + H + 2 * I + H;
    size_t row_major = 0, scales = 0;
    switch (cfg->wfmt) {
        case LLMIE_W_F16: row_major = elems * 2; break;
        case LLMIE_W_F32: row_major = elems * 4; break;
        case LLMIE_W_INT8: row_major = elems; scales = rows * 2; break;
        case LLMIE_W_FP8: row_major = elems; scales = rows * 4; break;
        case LLMIE_W_INT4: row_major = elems / 2; scales = (elems / (cfg->int4_group > 0 ? cfg->int4_group : 128)) * 2; break;
        case LLMIE_W_MXFP4: row_major = elems / 2; scales = elems / 32; break;   // N K / 2 codes + N K / 32 e8m0 bytes per matrix
        default: return 0;
    }
    const int wf = packed_wf(cfg);
    const size_t images = wf ? packed_carve(cfg, wf).layer_bytes : 0;
    const size_t per_layer = ((cfg->flags & LLMIE_DEC_PACKED_ONLY) && wf ? 0 : row_major) + scales + images;
    return per_layer * cfg->num_layers;
}

// The one function that computes a (cos, sin) table (include/llmie.h): host only.  NONE / NULL is the fp32 formula the engine has always
// used, bit for bit; the scaled kinds are evaluated in double and rounded once.
extern "C" int llmie_rope_table_fill(float *cos_sin_out, int max_pos, int head_size, int rotary_dim, float rotary_base,
                                     const llmie_rope_scaling *sc) {
    LLMIE_REQUIRE(cos_sin_out, "rope_table_fill: NULL output");
    LLMIE_REQUIRE(max_pos >= 1 && head_size >= 2, "rope_table_fill: bad shape (max_pos %d, head_size %d)", max_pos, head_size);
    LLMIE_REQUIRE(rotary_dim >= 2 && rotary_dim % 2 == 0, "rope_table_fill: rotary_dim %d must be even and positive", rotary_dim);
    const int kind = sc ? static_cast<int>(sc->kind) : static_cast<int>(LLMIE_ROPE_NONE);
    LLMIE_REQUIRE(kind >= LLMIE_ROPE_NONE && kind <= LLMIE_ROPE_YARN, "rope_table_fill: unknown scaling kind %d", kind);
    // (NONE keeps what llmie_decoder_create has always accepted: a rotary_dim above the head size stops at head_size / 2 pairs)
    LLMIE_REQUIRE(kind == LLMIE_ROPE_NONE || (rotary_dim <= head_size && head_size % 2 == 0),
                  "rope_table_fill: a scaled table needs an even head_size and rotary_dim <= head_size (%d, %d)", head_size, rotary_dim);
    LLMIE_REQUIRE(kind == LLMIE_ROPE_NONE || rotary_base > 0.f, "rope_table_fill: rotary_base must be positive");
    const int half = head_size / 2, rot = rotary_dim / 2;
    if (kind == LLMIE_ROPE_NONE) {
        for (int pos = 0; pos < max_pos; ++pos)
            for (int j = 0; j < half; ++j) {
                float c = 1.f, s = 0.f;
                if (j < rot) {
                    const float ang = static_cast<float>(pos) / powf(rotary_base, static_cast<float>(2 * j) / static_cast<float>(rotary_dim));
                    c = cosf(ang), s = sinf(ang);
                }
                cos_sin_out[2 * (static_cast<size_t>(pos) * half + j)] = c;
                cos_sin_out[2 * (static_cast<size_t>(pos) * half + j) + 1] = s;
            }
        return LLMIE_OK;
    }
    const double factor = sc->factor, orig = sc->original_max_pos, base = rotary_base, two_pi = 6.283185307179586476925286766559;
    LLMIE_REQUIRE(std::isfinite(sc->factor) && sc->factor >= 1.f, "rope_table_fill: factor %g must be >= 1", factor);
    if (kind != LLMIE_ROPE_LINEAR) LLMIE_REQUIRE(sc->original_max_pos >= 1, "rope_table_fill: original_max_pos %d must be positive", sc->original_max_pos);
    double attn = 1.0, lo = 0.0, hi = 0.0;
    if (kind == LLMIE_ROPE_LLAMA3)
        LLMIE_REQUIRE(sc->low_freq_factor > 0.f && sc->high_freq_factor > sc->low_freq_factor,
                      "rope_table_fill: needs 0 < low_freq_factor < high_freq_factor (%g, %g)", (double)sc->low_freq_factor, (double)sc->high_freq_factor);
    if (kind == LLMIE_ROPE_YARN) {
        LLMIE_REQUIRE(sc->beta_fast >= 0.f && sc->beta_slow >= 0.f, "rope_table_fill: a beta must not be negative");
        const double bf = sc->beta_fast > 0.f ? sc->beta_fast : 32.0, bs = sc->beta_slow > 0.f ? sc->beta_slow : 1.0;
        auto corr = [&](double n) { return rotary_dim * std::log(orig / (two_pi * n)) / (2.0 * std::log(base)); };
        lo = corr(bf), hi = corr(bs);
        if (sc->truncate) lo = std::floor(lo), hi = std::ceil(hi);
        lo = std::max(lo, 0.0), hi = std::min(hi, static_cast<double>(rotary_dim - 1));
        if (lo == hi) hi += 0.001;
        attn = sc->attn_factor > 0.f ? static_cast<double>(sc->attn_factor) : 0.1 * std::log(factor) + 1.0;
    }
    std::vector<double> freq(rot);
    for (int j = 0; j < rot; ++j) {
        const double f = std::pow(base, -2.0 * j / rotary_dim);
        double g = f / factor;
        if (kind == LLMIE_ROPE_LLAMA3) {
            const double w = two_pi / f, lf = sc->low_freq_factor, hf = sc->high_freq_factor;
            if (w < orig / hf) g = f;
            else if (!(w > orig / lf)) {
                const double t = (orig / w - lf) / (hf - lf);
                g = (1.0 - t) * f / factor + t * f;
            }
        } else if (kind == LLMIE_ROPE_YARN) {
            const double ramp = std::min(1.0, std::max(0.0, (j - lo) / (hi - lo)));
            g = f / factor * ramp + f * (1.0 - ramp);
        }
        freq[j] = g;
    }
    for (int pos = 0; pos < max_pos; ++pos)
        for (int j = 0; j < half; ++j) {
            float c = 1.f, s = 0.f;
            if (j < rot) {
                const double ang = pos * freq[j];
                c = static_cast<float>(std::cos(ang) * attn), s = static_cast<float>(std::sin(ang) * attn);
            }
            cos_sin_out[2 * (static_cast<size_t>(pos) * half + j)] = c;
            cos_sin_out[2 * (static_cast<size_t>(pos) * half + j) + 1] = s;
        }
    return LLMIE_OK;
}
// fills the engine's table on the host and uploads it with one synchronous copy
static int rope_table_upload(llmie_decoder *d, const llmie_rope_scaling *sc, const char *who) {
    const llmie_decoder_config &c = d->cfg;
    std::vector<float> tab(static_cast<size_t>(c.max_seq_len) * (c.head_size / 2) * 2);
    const int rc = llmie_rope_table_fill(tab.data(), c.max_seq_len, c.head_size, c.rotary_dim, c.rotary_base, sc);
    if (rc != LLMIE_OK) return rc;
    if (hipMemcpy(d->rope_table, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("%s: RoPE table upload failed", who);
        return LLMIE_ERR_LAUNCH;
    }
    return LLMIE_OK;
}

extern "C" llmie_decoder *llmie_decoder_create(const llmie_decoder_config *cfg, const llmie_layer_weights *layers,
                                               void *workspace, size_t workspace_bytes) {
    if (!config_ok(cfg)) {
        set_error("decoder_create: invalid config");
        return nullptr;
    }
    if (!layers || !workspace) {
        set_error("decoder_create: NULL layers/workspace");
        return nullptr;
    }
    const EngineCarve offs = carve(cfg);
    const size_t need = offs.total;
    if (workspace_bytes < need) {
        set_error("decoder_create: workspace too small (%zu < %zu)", workspace_bytes, need);
        return nullptr;
    }
    if (reinterpret_cast<uintptr_t>(workspace) % 256) {
        set_error("decoder_create: workspace must be 256-byte aligned");
        return nullptr;
    }
    for (int l = 0; l < cfg->num_layers; ++l) {
        const llmie_layer_weights &w = layers[l];
        if (!w.attn_norm_gamma || !w.ffn_norm_gamma || !w.qkv.data || !w.o.data || !w.gate_up.data || !w.down.data) {
            set_error("decoder_create: layer %d has a NULL weight", l);
            return nullptr;
        }
        if (cfg->wfmt != LLMIE_W_F16 && cfg->wfmt != LLMIE_W_F32 &&
            (!w.qkv.scale || !w.o.scale || !w.gate_up.scale || !w.down.scale)) {
            set_error("decoder_create: layer %d lacks quantisation scales", l);
            return nullptr;
        }
    }
    llmie_decoder *d = new (std::nothrow) llmie_decoder();
    if (!d) return nullptr;
    d->cfg = *cfg;
    d->layers.assign(layers, layers + cfg->num_layers);
    d->H = cfg->head_num * cfg->head_size;
    d->QKV = (cfg->head_num + 2 * cfg->kv_head_num) * cfg->head_size;
    d->I = cfg->inter_size;
    d->esz = cfg->dtype == LLMIE_F16 ? 2 : 4;
    char *base = static_cast<char *>(workspace);
    d->resid = base + offs.resid;
    d->qkv = base + offs.qkv;
    d->mha = base + offs.mha;
    d->act = base + offs.act;
    d->gu = base + offs.gu;
    d->attn_ws = base + offs.attn_ws;
    d->attn_ws_bytes = llmie_decoder_mha_workspace_bytes(cfg->max_batch, cfg->head_num, cfg->head_size, cfg->max_seq_len);
    d->rope_table = reinterpret_cast<float2 *>(base + offs.rope_table);
    d->tail_ticket = reinterpret_cast<unsigned *>(base + offs.tail_ticket);
    if (hipMemset(d->tail_ticket, 0, 256) != hipSuccess) {
        set_error("decoder_create: clearing the workspace words failed");
        delete d;
        return nullptr;
    }
    d->fp8_ws = base + offs.fp8_ws;
    {
        const int kmax = cfg->inter_size > d->H ? cfg->inter_size : d->H;
        d->fp8_ws_bytes = cfg->wfmt == LLMIE_W_FP8 ? llmie_linear_fp8_workspace_bytes(cfg->max_batch, kmax, 0) : 0;
    }
    d->slab_ws = SlabWs{reinterpret_cast<float *>(base + offs.slabs), engine_slab_floats(cfg, cfg->max_batch)};
    if (!d->slab_ws.floats) d->slab_ws.p = nullptr;
    d->pk_wf = packed_wf(cfg);
    if ((cfg->flags & LLMIE_DEC_PACKED_ONLY) && !d->pk_wf) {
        set_error("%s", packed_only_refusal(cfg));
        delete d;
        return nullptr;
    }
    if (d->pk_wf) {
        // (uploads of the weights on other streams -- torch side streams are non-blocking -- must have landed before they are packed)
        if (hipDeviceSynchronize() != hipSuccess) {
            set_error("decoder_create: device synchronise failed");
            delete d;
            return nullptr;
        }
        // one-time re-tiling of every matrix into the stream-friendly image (null stream, synchronous: create is not on the
        // compute path); the row-major originals stay in use for batch <= gemv_max (GEMV) and for prefill
        const PackedCarve pc = packed_carve(cfg, d->pk_wf);
        unsigned char *pb = reinterpret_cast<unsigned char *>(base + offs.packed);
        d->pk_base = pb;
        const int prc = pack_layers(d, layers, nullptr);
        unsigned char *tail = pb + pc.layer_bytes * cfg->num_layers;
        d->hx = reinterpret_cast<half_t *>(tail);
        d->actx = reinterpret_cast<half_t *>(tail + pc.hx);
        d->mhax = reinterpret_cast<half_t *>(tail + pc.hx + pc.actx);
        d->pk_slab = reinterpret_cast<float *>(tail + pc.hx + pc.actx + pc.mhax);
        d->pk_slab_floats = (pc.slab - 16) / sizeof(float);
        d->pk_sync = reinterpret_cast<unsigned *>(tail + pc.hx + pc.actx + pc.mhax + pc.slab);
        d->pk_err = reinterpret_cast<unsigned *>(tail + pc.hx + pc.actx + pc.mhax + pc.slab + pc.sync - 256);
        if (prc != LLMIE_OK || hipMemset(tail, 0, pc.hx + pc.actx + pc.mhax) != hipSuccess || hipMemset(d->pk_sync, 0, pc.sync) != hipSuccess ||
            hipDeviceSynchronize() != hipSuccess) {
            set_error("decoder_create: packing the weights for the batch path failed");
            delete d;
            return nullptr;
        }
        if (cfg->flags & LLMIE_DEC_PACKED_ONLY) {   // the caller may free the row-major matrices now: forget them
            d->packed_only = true;
            for (llmie_layer_weights &w : d->layers) w.qkv.data = w.o.data = w.gate_up.data = w.down.data = nullptr;
        }
    }
    // cos/sin of angle = pos / base^(2j/rot_dim) (rope_utils.cuh:6-19), evaluated on the host in fp32 with libm -- one synchronous
    // upload at create time (llmie_decoder_set_rope_scaling is the only other host<->device copy the engine ever does)
    if (rope_table_upload(d, nullptr, "decoder_create") != LLMIE_OK) {
        delete d;
        return nullptr;
    }
    return d;
}

extern "C" void llmie_decoder_destroy(llmie_decoder *dec) {
    if (!dec) return;
    for (hipEvent_t e : dec->ev) (void)hipEventDestroy(e);
    delete dec;
}

extern "C" int llmie_decoder_profile_begin(llmie_decoder *dec, int max_events) {
    LLMIE_REQUIRE(dec && max_events > 0, "decoder_profile_begin: bad arguments");
    while (dec->ev.size() < 2 * static_cast<size_t>(max_events)) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) {
            set_error("decoder_profile_begin: hipEventCreate failed");
            return LLMIE_ERR_LAUNCH;
        }
        dec->ev.push_back(e);
    }
    dec->ev_op.assign(max_events, 0);
    dec->ev_used = 0;
    dec->profiling = true;
    return LLMIE_OK;
}

extern "C" int llmie_decoder_profile_end(llmie_decoder *dec, llmie_stream stream, double *ms_by_op, int *launches_by_op) {
    LLMIE_REQUIRE(dec && ms_by_op && launches_by_op, "decoder_profile_end: NULL pointer");
    dec->profiling = false;
    if (hipStreamSynchronize(as_stream(stream)) != hipSuccess) {
        set_error("decoder_profile_end: stream synchronise failed");
        return LLMIE_ERR_LAUNCH;
    }
    for (int i = 0; i < LLMIE_OP_COUNT; ++i) {
        ms_by_op[i] = 0.0;
        launches_by_op[i] = 0;
    }
    for (size_t i = 0; i < dec->ev_used; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, dec->ev[2 * i], dec->ev[2 * i + 1]) == hipSuccess) {
            ms_by_op[dec->ev_op[i]] += ms;
            launches_by_op[dec->ev_op[i]] += 1;
        }
    }
    dec->ev_used = 0;
    return LLMIE_OK;
}

extern "C" int llmie_decoder_status(llmie_decoder *dec, llmie_stream stream) {
    LLMIE_REQUIRE(dec, "decoder_status: NULL decoder");
    if (hipStreamSynchronize(as_stream(stream)) != hipSuccess) {
        set_error("decoder_status: stream synchronise failed: %s", hipGetErrorString(hipGetLastError()));
        return LLMIE_ERR_LAUNCH;
    }
    if (!dec->pk_err) return LLMIE_OK;
    unsigned word = 0;
    if (hipMemcpy(&word, dec->pk_err, sizeof(word), hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("decoder_status: reading the device error word failed");
        return LLMIE_ERR_LAUNCH;
    }
    if (word) {
        (void)hipMemset(dec->pk_err, 0, sizeof(word));
        (void)hipMemset(dec->pk_sync, 0, static_cast<size_t>(dec->cfg.num_layers) * pk_chain_sync_bytes());   // counters are mid-flight: start over
        set_error("decoder: a grid barrier of the persistent chain launch timed out (code 0x%08x, phase %u): not every workgroup was "
                  "resident; set LLMIE_NO_CHAIN=1 to use the launch sequence", word, word & 0xfu);
        return LLMIE_ERR_LAUNCH;
    }
    return LLMIE_OK;
}

// Diagnostic, not on the product path: the chain launches of this decoder write s_memrealtime (100 MHz) stamps of their phase
// edges for every workgroup into `stamps_dev` ([256][16] uint64, device memory; every layer overwrites it); null disarms.
extern "C" int llmie_decoder_debug_stamps(llmie_decoder *dec, void *stamps_dev) {
    LLMIE_REQUIRE(dec, "decoder_debug_stamps: NULL decoder");
    dec->pk_stamps = static_cast<unsigned long long *>(stamps_dev);
    return LLMIE_OK;
}

// ---- the engine's projections: ONE switch over the weight format.  A call on a layer matrix is a LinearOperands (proj_operands) and
// the scratch of the sequence that makes it (decode: decode_scratch; prefill: PrefillPass::scratch); engine_proj runs it. ----
static int wfmt_bits(llmie_weight_format fmt) {
    switch (fmt) {
        case LLMIE_W_F16: return 16;
        case LLMIE_W_INT8: return 8;
        case LLMIE_W_INT4: return 4;
        case LLMIE_W_FP8: return WF_FP8;
        case LLMIE_W_MXFP4: return WF_MXFP4;
        default: return 0;
    }
}
// y = [swiglu]( rmsnorm(x + pre_bias) * gamma . w^T ) (+ residual) on a matrix of the engine (the projections take no bias: the norm
// behind the O projection adds its bias, the attention launch the QKV one)
static LinearOperands proj_operands(const llmie_decoder_config &c, const void *x, const llmie_matrix &w, void *y, int M, int K, int N, int epi,
                                    const void *residual, const void *gamma = nullptr, const void *pre_bias = nullptr) {
    return LinearOperands{x, w.data, w.scale, y, M, K, N, epi, c.int4_group, nullptr, residual, gamma, pre_bias, c.rms_eps};
}
// decode: one slab area and the fp8 activation area; no room for an fp16 image (such row counts run their split-K or row-chunk routes)
static LinearScratch decode_scratch(const llmie_decoder *d) { return LinearScratch{d->slab_ws, nullptr, 0, d->fp8_ws, d->fp8_ws_bytes}; }
// gu: [M, N] scratch.  Formats without a fused SwiGLU form in linear_run (fp32, fp8 and MXFP4 weights) run it as projection +
// llmie_silu_and_mul
static int engine_proj(llmie_weight_format fmt, const LinearOperands &o, const LinearScratch &s, void *gu, llmie_stream stream) {
    const bool f32 = fmt == LLMIE_W_F32;
    if (o.epi == EPI_SWIGLU_ && (f32 || fmt == LLMIE_W_FP8 || fmt == LLMIE_W_MXFP4)) {
        LinearOperands p = o;
        p.y = gu, p.epi = EPI_NONE_, p.residual = nullptr;
        if (int rc = engine_proj(fmt, p, s, gu, stream)) return rc;
        return llmie_silu_and_mul(gu, o.y, o.M, o.N / 2, f32 ? LLMIE_F32 : LLMIE_F16, stream);
    }
    if (f32) return llmie_linear(o.x, o.w, o.y, o.M, o.K, o.N, 1, o.bias, o.residual, LLMIE_F32, nullptr, 0, stream);
    if (!wfmt_bits(fmt)) {
        set_error("engine: weight format %d not supported by this build", (int)fmt);
        return LLMIE_ERR_UNSUPPORTED;
    }
    return linear_run(wfmt_bits(fmt), o, s, as_stream(stream));
}
// a decode-side projection (the unfused and lora sequences, the LM head)
static int engine_linear(const llmie_decoder *d, llmie_weight_format fmt, const LinearOperands &o, llmie_stream stream) {
    return engine_proj(fmt, o, decode_scratch(d), d->gu, stream);
}

// ---- which launch sequence a call runs: decided once, by a pure host function per entry point (no device access, no getenv) ----
// The environment switches of the engine, read once per process.  (LLMIE_NO_NORM_QUANT belongs to norm.hip.)
struct EngineSwitches {
    bool no_fused_decode, no_fused_batch, no_packed_batch, chain, no_fused_short_prefill, no_qkv_rope_fusion;
};
static const EngineSwitches &engine_switches() {
    static const EngineSwitches s{getenv("LLMIE_NO_FUSED_DECODE") != nullptr,        getenv("LLMIE_NO_FUSED_BATCH") != nullptr,
                                  getenv("LLMIE_NO_PACKED_BATCH") != nullptr,        getenv("LLMIE_CHAIN") != nullptr,
                                  getenv("LLMIE_NO_FUSED_SHORT_PREFILL") != nullptr, getenv("LLMIE_NO_QKV_ROPE_FUSION") != nullptr};
    return s;
}
static EngineSwitches switches_of_mask(unsigned m) {
    return EngineSwitches{(m & LLMIE_SW_NO_FUSED_DECODE) != 0,        (m & LLMIE_SW_NO_FUSED_BATCH) != 0, (m & LLMIE_SW_NO_PACKED_BATCH) != 0,
                          (m & LLMIE_SW_CHAIN) != 0,                  (m & LLMIE_SW_NO_FUSED_SHORT_PREFILL) != 0,
                          (m & LLMIE_SW_NO_QKV_ROPE_FUSION) != 0};
}
// head sizes / head ratios of the attention kernels with RoPE, bias and the KV append fused in front
static bool fused_attention_geometry(const llmie_decoder_config &c) {
    const int rep = c.head_num / c.kv_head_num;
    return (c.head_size == 32 || c.head_size == 64 || c.head_size == 128 || c.head_size == 256) && (rep == 1 || rep == 2 || rep == 4 || rep == 8);
}

enum DecodePath : int { DP_REFUSED = 0, DP_GEMV, DP_PACKED, DP_PACKED_CHAIN, DP_SPLITK, DP_UNFUSED, DP_LORA, DP_MOE };
enum DecodeRefusal : int { DREF_NONE = 0, DREF_PACKED_ONLY, DREF_PAGED, DREF_KV_FP8, DREF_RAGGED, DREF_LORA, DREF_MX4_HIDDEN, DREF_MOE, DREF_MOE_LORA };
// One decode call as the planner sees it.  mis_hidden / mis_wqkv0: address % 16 of the hidden state and of layer 0's QKV matrix.
struct DecodeCall {
    llmie_decoder_config cfg;
    int batch;
    bool paged, ragged;
    unsigned mis_hidden, mis_wqkv0;
    EngineSwitches sw;
    bool lora;   // an adapter table is attached
    bool moe;    // experts are attached (llmie_decoder_moe_attach)
};
// what the adapter updates need of an engine: fp16 rows in front of every projection and a row-major route for the base (not fp8
// weights, not a packed-only engine), K % 32 == 0 and column blocks (q / k / v, gate / up) that are multiples of 16
static bool lora_engine_ok(const llmie_decoder_config &c) {
    const int H = c.head_num * c.head_size;
    return c.dtype == LLMIE_F16 && c.wfmt != LLMIE_W_FP8 && c.wfmt != LLMIE_W_F32 && c.wfmt != LLMIE_W_MXFP4 &&
           !(c.flags & LLMIE_DEC_PACKED_ONLY) && H % 32 == 0 &&
           c.inter_size % 32 == 0 && (c.kv_head_num * c.head_size) % 16 == 0;
}
// what a sliding window needs of an engine: the windowed instantiations of the decode split kernel (attention_decode.hip; the flash
// prefill kernel has them for every engine it runs on)
static bool window_engine_ok(const llmie_decoder_config &c) {
    const int rep = c.head_num / c.kv_head_num;
    return c.dtype == LLMIE_F16 && (c.head_size == 64 || c.head_size == 128) &&
           (rep == 1 || rep == 2 || rep == 4 || (rep == 8 && c.kv_fmt != LLMIE_KV_FP8));
}
// what the expert FFN needs of an engine: fp16 normalised rows in front of the FFN and a row-major route for the other projections
static bool moe_engine_ok(const llmie_decoder_config &c) {
    return c.dtype == LLMIE_F16 && (c.wfmt == LLMIE_W_F16 || c.wfmt == LLMIE_W_INT8 || c.wfmt == LLMIE_W_INT4) &&
           !(c.flags & LLMIE_DEC_PACKED_ONLY) && (c.head_num * c.head_size) % 64 == 0;
}
static const char *const kMoeRefusal =
    "experts need an fp16 engine with fp16 / int8 / int4 weights (not LLMIE_DEC_PACKED_ONLY) and a hidden size that is a multiple of 64";
static const char *const kMoeLoraRefusal = "an adapter table and experts cannot be attached to one engine at the same time";
static const char *const kWindowRefusal =
    "a sliding window needs an fp16 engine with head_size 64 / 128 and head_num / kv_head_num in {1,2,4,8} (e4m3 cache: {1,2,4})";
static const char *const kHeadSinkRefusal =
    "head sinks need an fp16 engine with head_size 64 / 128 and head_num / kv_head_num in {1,2,4,8} (e4m3 cache: {1,2,4})";
static const char *const kQkNormRefusal =
    "QK-norm needs an fp16 engine with head_size 64 / 128 and head_num / kv_head_num in {1,2,4,8} (e4m3 cache: {1,2,4}), no layer with a "
    "QKV bias, and neither a sliding window nor head sinks set";
static const char *const kLoraRefusal =
    "adapters need an fp16 engine with fp16 / int8 / int4 weights (an fp8-weight engine never materialises fp16 normalised rows, a "
    "LLMIE_DEC_PACKED_ONLY engine has no row-major route), hidden and inter sizes that are multiples of 32 and q / kv widths that are "
    "multiples of 16";
// The LLMIE_CHAIN probe (can every projection of a layer join a chain at this batch?) reads the engine's images and LDS plans, so it
// stays with the packed sequence: the plan answers DP_PACKED with chain_wanted, and the dispatch upgrades to DP_PACKED_CHAIN where
// the probe passes.
struct DecodePlan {
    int path, refusal;
    bool chain_wanted;
};
static DecodePlan plan_decode(const DecodeCall &d) {
    const llmie_decoder_config &c = d.cfg;
    const int batch = d.batch, H = c.head_num * c.head_size, I = c.inter_size;
    const bool attn_ok = fused_attention_geometry(c);
    const int wbits = c.wfmt == LLMIE_W_F16 ? 16 : (c.wfmt == LLMIE_W_INT8 ? 8 : (c.wfmt == LLMIE_W_INT4 ? 4 : 0));
    const bool fp8 = c.wfmt == LLMIE_W_FP8, packed_only = (c.flags & LLMIE_DEC_PACKED_ONLY) != 0;
    // GEMV form up to gemv_max rows (its dot products are VALU work that grows with the batch), MFMA split-K above
    // measured crossover on MI355X (7B, ctx 512, tokens/s GEMV vs split-K): fp16 b4 1157/1143, b6 1496/1592; int8 b4 1416/1404,
    // b6 1672/1962; fp8 b3 947/944, b4 1127/1213; int4 b2 796/745, b3 896/1074
    const int gemv_max = gemv_max_batch(c.wfmt);
    if (d.moe) {
        // the unfused sequence with route + expert FFN in place of the gate/up and down launches of every layer that has a router; the
        // same attention conditions as the lora sequence
        if (d.lora) return {DP_REFUSED, DREF_MOE_LORA, false};
        if (!moe_engine_ok(c)) return {DP_REFUSED, DREF_MOE, false};
        if (!attn_ok && d.paged) return {DP_REFUSED, DREF_PAGED, false};
        if (!attn_ok && c.kv_fmt == LLMIE_KV_FP8) return {DP_REFUSED, DREF_KV_FP8, false};
        if (!attn_ok && d.ragged) return {DP_REFUSED, DREF_RAGGED, false};
        return {DP_MOE, DREF_NONE, false};
    }
    if (d.lora) {
        // the unfused sequence with the four adapter updates behind its projections; its attention launch carries what the fused
        // paths need of it (paged / e4m3 caches, ragged lengths) where the geometry has the fused kernel
        if (!lora_engine_ok(c)) return {DP_REFUSED, DREF_LORA, false};
        if (!attn_ok && d.paged) return {DP_REFUSED, DREF_PAGED, false};
        if (!attn_ok && c.kv_fmt == LLMIE_KV_FP8) return {DP_REFUSED, DREF_KV_FP8, false};
        if (!attn_ok && d.ragged) return {DP_REFUSED, DREF_RAGGED, false};
        return {DP_LORA, DREF_NONE, false};
    }
    if (c.wfmt == LLMIE_W_MXFP4) {
        // every batch runs the unfused sequence (the fused-norm and SwiGLU forms of the GEMV are not built for the format); its
        // attention launch carries paged / e4m3 caches and ragged lengths where the geometry has the fused kernel, as the lora one's
        if (packed_only) return {DP_REFUSED, DREF_PACKED_ONLY, false};
        if (d.mis_hidden) return {DP_REFUSED, DREF_MX4_HIDDEN, false};
        if (!attn_ok && d.paged) return {DP_REFUSED, DREF_PAGED, false};
        if (!attn_ok && c.kv_fmt == LLMIE_KV_FP8) return {DP_REFUSED, DREF_KV_FP8, false};
        if (!attn_ok && d.ragged) return {DP_REFUSED, DREF_RAGGED, false};
        return {DP_UNFUSED, DREF_NONE, false};
    }
    const bool int4_ok = wbits == 4 && c.int4_group == 128 && batch <= 64;  // int4 MFMA form: group-128 scales, 64 rows per pass
    const bool batch_path_ok = !d.sw.no_fused_batch && c.dtype == LLMIE_F16 && (wbits == 16 || wbits == 8 || int4_ok || fp8) && attn_ok &&
                               batch <= 128 && H % 256 == 0 && I % 256 == 0 && H >= 512 && I >= 512 && splitk_rownorm_eligible(H);
    // (gemv_f16_eligible looks at the two addresses' alignment only)
    const bool gemv_ok = !packed_only && (batch <= gemv_max || !batch_path_ok) &&
                         (wbits == 16 ? gemv_f16_eligible(batch, H, reinterpret_cast<const void *>(static_cast<uintptr_t>(d.mis_hidden)),
                                                          reinterpret_cast<const void *>(static_cast<uintptr_t>(d.mis_wqkv0)))
                                      : ((wbits != 0 || fp8) && ksplit_eligible(batch, H, fp8 ? 8 : wbits)));
    // (fp8: gemv_ok holds ksplit_eligible(batch, H, 8), so every projection with a fused norm or SwiGLU -- K = H -- has its GEMV form)
    if (!d.sw.no_fused_decode && c.dtype == LLMIE_F16 && (wbits != 0 || fp8) && attn_ok && H % 8 == 0 && gemv_ok) return {DP_GEMV, DREF_NONE, false};
    const bool packed_on = !d.sw.no_packed_batch && !d.sw.no_fused_decode && attn_ok;
    if (packed_only && !(packed_on && packed_batch(c, batch))) return {DP_REFUSED, DREF_PACKED_ONLY, false};
    if (packed_on && packed_wf(&c) && packed_batch(c, batch)) return {DP_PACKED, DREF_NONE, d.sw.chain};
    if (batch_path_ok) return {DP_SPLITK, DREF_NONE, false};
    if (d.paged) return {DP_REFUSED, DREF_PAGED, false};
    if (c.kv_fmt == LLMIE_KV_FP8) return {DP_REFUSED, DREF_KV_FP8, false};
    if (d.ragged && !attn_ok) return {DP_REFUSED, DREF_RAGGED, false};
    return {DP_UNFUSED, DREF_NONE, false};
}
static int decode_refuse(const DecodeCall &d, const DecodePlan &p) {
    switch (p.refusal) {
        case DREF_PACKED_ONLY:
            set_error("decoder_forward: a LLMIE_DEC_PACKED_ONLY engine decodes on the packed kernels only (batch <= %d, no path switch)",
                      packed_rows_max(d.cfg));
            break;
        case DREF_LORA: set_error("decoder_forward: %s", kLoraRefusal); break;
        case DREF_MOE: set_error("decoder_forward: %s", kMoeRefusal); break;
        case DREF_MOE_LORA: set_error("decoder_forward: %s", kMoeLoraRefusal); break;
        case DREF_MX4_HIDDEN: set_error("decoder_forward: MXFP4 weights need a 16-byte aligned hidden_out"); break;
        case DREF_PAGED: set_error("decoder_forward_paged: the paged KV cache needs the fused decode paths (fp16 engines, batch <= 128)"); break;
        case DREF_KV_FP8:
            set_error("decoder_forward: the fp8 KV cache needs the fused decode paths (batch <= 128, fp16/int8/int4/fp8 weights with "
                      "H and I multiples of 256 at batch > 8)");
            break;
        default: set_error("decoder_forward_ragged: needs head_size in {32,64,128,256} and head_num/kv_head_num in {1,2,4,8}"); break;
    }
    return LLMIE_ERR_UNSUPPORTED;
}
static const char *decode_path_name(int path) {
    static const char *const names[] = {"refused", "gemv", "packed", "packed_chain", "splitk", "unfused", "lora", "moe"};
    return names[path];
}

enum PrefillPath : int { PP_REFUSED = 0, PP_PACKED_ONLY, PP_SHORT_SPLITK, PP_LEAN, PP_GENERAL, PP_LORA, PP_MOE };
enum PrefillRefusal : int { PREF_NONE = 0, PREF_FORMAT, PREF_PACKED_ONLY_FP8, PREF_LORA, PREF_MOE, PREF_MOE_LORA };
// One prefill call as the planner sees it.  The split-K kernels read the weights, the out-of-place norms hidden_out and the gammas
// in 16-byte vectors: weights handed over as views at other offsets (llmie_decoder_create takes any address) run the general sequences.
struct PrefillCall {
    llmie_decoder_config cfg;
    int T;
    bool weights_a16;         // every layer matrix 16-byte aligned
    bool int4_scales_a4;      // every int4 group-scale array 4-byte aligned
    bool hidden_gammas_a16;   // hidden_out and every gamma 16-byte aligned
    bool o_bias;              // some layer has an output-projection bias
    EngineSwitches sw;
    bool lora;                // an adapter table is attached
    bool moe;                 // experts are attached
    bool qk_norm;             // QK-norm is set: q and k are normalised in the RoPE + append launch, so no QKV form does RoPE itself
    bool tree = false;        // a draft tree is set: the RoPE + append launch rotates by depth, so no QKV form does RoPE itself
};
struct PrefillPlan {
    int path, refusal;
};
static PrefillPlan plan_prefill(const PrefillCall &p) {
    const llmie_decoder_config &c = p.cfg;
    const int T = p.T, H = c.head_num * c.head_size, I = c.inter_size;
    const bool fp8 = c.wfmt == LLMIE_W_FP8;
    const int wqbits = c.wfmt == LLMIE_W_INT8 ? 8 : (c.wfmt == LLMIE_W_INT4 ? 4 : 0);
    const bool mx4 = c.wfmt == LLMIE_W_MXFP4;
    if (c.dtype != LLMIE_F16 || (c.wfmt != LLMIE_W_F16 && !fp8 && !wqbits && !mx4) || c.head_size != 128) return {PP_REFUSED, PREF_FORMAT};
    if (p.moe) {
        if (p.lora) return {PP_REFUSED, PREF_MOE_LORA};
        return moe_engine_ok(c) ? PrefillPlan{PP_MOE, PREF_NONE} : PrefillPlan{PP_REFUSED, PREF_MOE};
    }
    if (p.lora) return lora_engine_ok(c) ? PrefillPlan{PP_LORA, PREF_NONE} : PrefillPlan{PP_REFUSED, PREF_LORA};
    // MXFP4: the general sequence at every row count (llmie_linear_mxfp4 picks the projection's route by the rows; no packed image)
    // (a LLMIE_DEC_PACKED_ONLY config never gets here: creating the engine refuses it)
    if (mx4) return {PP_GENERAL, PREF_NONE};
    if (c.flags & LLMIE_DEC_PACKED_ONLY) return fp8 ? PrefillPlan{PP_REFUSED, PREF_PACKED_ONLY_FP8} : PrefillPlan{PP_PACKED_ONLY, PREF_NONE};
    const bool short_fmt_ok = !fp8 && (wqbits != 4 || (c.int4_group == 128 && T <= 64));   // int4 split-K form: 64 rows, group 128
    if (!p.sw.no_fused_short_prefill && short_fmt_ok && p.weights_a16 && (wqbits != 4 || p.int4_scales_a4) && T <= 128 && H % 256 == 0 &&
        I % 256 == 0 && H >= 512 && I >= 512 && splitk_rownorm_eligible(H))
        return {PP_SHORT_SPLITK, PREF_NONE};
    if (!fp8 && p.hidden_gammas_a16 && rmsnorm_oop_eligible(H) && !p.o_bias) return {PP_LEAN, PREF_NONE};
    return {PP_GENERAL, PREF_NONE};
}
static int prefill_refuse(const PrefillPlan &p) {
    if (p.refusal == PREF_FORMAT)
        LLMIE_UNSUPPORTED("decoder_prefill: fp16 activations + fp16 / int8 / int4 / fp8 weights + head_size 128 only (use the per-kernel path)");
    if (p.refusal == PREF_LORA) LLMIE_UNSUPPORTED("decoder_prefill: %s", kLoraRefusal);
    if (p.refusal == PREF_MOE) LLMIE_UNSUPPORTED("decoder_prefill: %s", kMoeRefusal);
    if (p.refusal == PREF_MOE_LORA) LLMIE_UNSUPPORTED("decoder_prefill: %s", kMoeLoraRefusal);
    LLMIE_UNSUPPORTED("decoder_prefill: LLMIE_DEC_PACKED_ONLY engines prefill fp16 / int8 / int4 weights only");
}
static const char *prefill_path_name(int path) {
    static const char *const names[] = {"refused", "packed_only", "short_splitk", "lean", "general", "lora", "moe"};
    return names[path];
}

// ---- what one LAYER of a prefill pass launches: decided per layer, by a pure host function as well ----
enum PrefillNorm : int { PN_NONE = 0, PN_INPLACE, PN_OOP, PN_QUANT, PN_ROWNORM };
enum PrefillQkv : int {
    PQ_PLAIN = 0, PQ_ROPE_F16, PQ_ROPE_W8, PQ_ROPE_IMAGE, PQ_PLAIN_E4M3, PQ_ROPE_E4M3, PQ_UNPACK_PLAIN, PQ_ROPE_UNPACKED, PQ_SPLITK, PQ_SPLITK_ROPE
};
enum PrefillGateUp : int { PG_FUSED = 0, PG_TWO_LAUNCH, PG_E4M3_SWIGLU, PG_FP8_SWIGLU, PG_UNPACK_FUSED, PG_UNPACK_TWO_LAUNCH, PG_SPLITK };
// What the form choices read of one layer's operands: address % 16 of the QKV matrix, scales and bias, of the gate/up matrix and scales
// and of the hidden state; whether the FFN gamma is there; the split-K slab and de-quantisation areas of the pass's workspace.
struct PrefillLayerCall {
    unsigned mis_qkv_w, mis_qkv_scale, mis_qkv_bias, mis_gu_w, mis_gu_scale, mis_hidden;
    bool ffn_gamma;
    size_t slab_floats, deq_bytes;
};
// attn_norm / ffn_norm: PrefillNorm (PN_INPLACE: llmie_rmsnorm / llmie_fused_add_bias_residual_rmsnorm; PN_QUANT: rmsnorm_quant_f16, the
// FFN one with the O bias; PN_NONE / PN_ROWNORM: the split-K sequence, whose row kernels normalise for the next projection).  qkv:
// PrefillQkv (ROPE forms: RoPE + the cache append in the projection's epilogue, hence rope_done; IMAGE: dequantize_weights_f16 first;
// UNPACK: pk_unpack_f16 first).  launches: per LLMIE_OP_* kind, one per TIMED launch -- derived from the forms.
struct PrefillLayerPlan {
    int attn_norm, qkv, ffn_norm, gate_up;
    bool rope_done;
    PrefillAttnPlan attn;
    int launches[LLMIE_OP_COUNT];
};
// Round 3: RoPE + KV-cache append as the EPILOGUE of the QKV projection (context_attention.cpp:158-205 in one launch sequence;
// gemm8p.cuh ROPE forms): q is rotated on its way into the packed QKV buffer, k / v go straight to their cache slots and never
// travel through the buffer; bit-identical to projection + prefill_rope_append_kernel (same arithmetic on the fp16-rounded
// accumulator).  Prefill-sized T on the eight-phase kernels only; everything else keeps the two launches.  (Pass level: a pass where
// this holds writes the epilogue's token table once, whatever its layers end up choosing.)
static bool prefill_rope_fusable(const PrefillCall &p) {
    return !p.lora && !p.moe && !p.qk_norm && !p.tree && p.cfg.wfmt != LLMIE_W_MXFP4 && !p.sw.no_qkv_rope_fusion && p.T >= kWqPrefillRows && gemm256_fills(p.T, (p.cfg.head_num + 2 * p.cfg.kv_head_num) * p.cfg.head_size);
}
static PrefillLayerPlan plan_prefill_layer(const PrefillCall &p, int path, int batch, int max_q_len, const PrefillLayerCall &lc) {
    const llmie_decoder_config &c = p.cfg;
    const int T = p.T, H = c.head_num * c.head_size, QKV = (c.head_num + 2 * c.kv_head_num) * c.head_size, I = c.inter_size;
    const bool fp8 = c.wfmt == LLMIE_W_FP8, lean = path == PP_LEAN;
    const int wqbits = c.wfmt == LLMIE_W_INT8 ? 8 : (c.wfmt == LLMIE_W_INT4 ? 4 : 0);
    // stand-in addresses with the residues the eligibility functions look at (never dereferenced); ws: any workspace area -- they are
    // carved at 256-byte multiples
    auto at = [](unsigned mis) { return reinterpret_cast<void *>(static_cast<uintptr_t>(256 + mis)); };
    void *const ws = at(0);
    const SlabWs slabs{static_cast<float *>(ws), lc.slab_floats};
    // the projections' input: the lean sequence's norms write it into the workspace, the others normalise the hidden state in place
    const void *x = lean ? ws : at(lc.mis_hidden);
    const void *qw = at(lc.mis_qkv_w), *qsc = at(lc.mis_qkv_scale), *gw = at(lc.mis_gu_w), *gsc = at(lc.mis_gu_scale);
    const bool rope_ok = prefill_rope_fusable(p) && lc.mis_qkv_bias % 8 == 0;
    PrefillLayerPlan o{};
    if (path == PP_SHORT_SPLITK) {
        // (the slab consumer of the QKV projection does RoPE + the cache append as well: one launch less per layer)
        const SplitKSlabs sk{slabs.p, 1, T, QKV};
        o.qkv = !p.sw.no_qkv_rope_fusion && !p.qk_norm && !p.tree && splitk_finalize_qkv_rope_eligible(sk, c.head_size, ws, at(lc.mis_qkv_bias)) ? PQ_SPLITK_ROPE : PQ_SPLITK;
        o.attn_norm = PN_NONE, o.ffn_norm = PN_ROWNORM, o.gate_up = PG_SPLITK;
    } else if (path == PP_LORA || path == PP_MOE || c.wfmt == LLMIE_W_MXFP4) {
        // the general sequence with the forms the adapter updates need: normalised rows in place, the QKV buffer un-rotated (the update
        // lands before RoPE: the RoPE + append launch runs in front of the flash kernel), gate/up un-activated.  MXFP4 weights run the
        // same forms: their projections have the plain epilogue only
        o.attn_norm = o.ffn_norm = PN_INPLACE, o.qkv = PQ_PLAIN, o.gate_up = PG_TWO_LAUNCH;
    } else if (path == PP_PACKED_ONLY) {
        // every projection runs the fp16 GEMM on the unpacked image of its matrix: the fp16 forms, on the de-quantisation area
        o.qkv = rope_ok && lc.deq_bytes >= static_cast<size_t>(QKV) * H * sizeof(half_t) && gemm256_qkv_rope_eligible(G256_F16, T, QKV, H, x, ws, nullptr, ws)
                    ? PQ_ROPE_UNPACKED : PQ_UNPACK_PLAIN;
        const LinearCall gc = linear_call(16, LinearOperands{x, ws, nullptr, ws, T, H, 2 * I, EPI_SWIGLU_}, LinearScratch{slabs});
        o.gate_up = plan_linear_f16(gc).route != LR_REFUSED ? PG_UNPACK_FUSED : PG_UNPACK_TWO_LAUNCH;
        o.attn_norm = o.ffn_norm = PN_INPLACE;
    } else {
        // fp8, prefill-sized: the two RMSNorms emit the e4m3 activations of the projection behind them (norm.hip
        // rmsnorm_quant_kernel; bit-identical to norm + quantize_rows) and the tiled fp8 GEMM takes them as they are.
        // (The conditions here are the sequence's own, not plan_linear_fp8's route: a quantising norm needs a 256-row grid that FILLS
        // -- the time model's partly filled grids quantise inside linear_fp8 -- and the fused gate/up is llmie_linear_fp8_swiglu's rule.)
        const bool nq = fp8 && T > 8 && H % 128 == 0 && rmsnorm_quant_eligible(H);
        o.attn_norm = o.ffn_norm = lean ? PN_OOP : PN_INPLACE;
        o.qkv = PQ_PLAIN;
        if (nq && gemm256_fills(T, QKV) && QKV % 4 == 0 && (lc.mis_qkv_w | lc.mis_qkv_scale) == 0) {
            o.attn_norm = PN_QUANT;
            o.qkv = rope_ok && gemm256_qkv_rope_eligible(G256_E4M3, T, QKV, H, ws, qw, qsc, ws) ? PQ_ROPE_E4M3 : PQ_PLAIN_E4M3;
        } else if (rope_ok && !fp8 && !wqbits) {
            if (gemm256_qkv_rope_eligible(G256_F16, T, QKV, H, x, qw, nullptr, ws)) o.qkv = PQ_ROPE_F16;
        } else if (rope_ok && !fp8) {
            // int8 / int4: the route the plain projection would take -- the eight-phase int8 form, or (int4, and int8 shapes without the
            // in-kernel form) the fp16 image of the matrix -- with the epilogue on the same kernels
            const int route = plan_linear_wq(linear_call(wqbits, LinearOperands{x, qw, qsc, ws, T, H, QKV, EPI_NONE_, c.int4_group},
                                                         LinearScratch{slabs, ws, lc.deq_bytes})).route;
            if (route == LR_W8_G8P && gemm256_qkv_rope_eligible(G256_W8, T, QKV, H, x, qw, qsc, ws)) o.qkv = PQ_ROPE_W8;
            if (route == LR_WQ_IMAGE_PREFILL && gemm256_qkv_rope_eligible(G256_F16, T, QKV, H, x, ws, nullptr, ws)) o.qkv = PQ_ROPE_IMAGE;
        }
        // act = swiglu(x . Wgu^T) (ffn.cpp:105-122): fused into the projection's epilogue where the route plan has a form, else
        // projection + llmie_silu_and_mul (e.g. fp16 H < 512 at 65-192 rows, int8 H % 256 != 0 at 9-191 rows, weights at offsets the
        // vector kernels do not take).  Quantised weights at prefill-sized T fuse only where the 256-row SwiGLU grid fills the chip:
        // the split-K and row-chunk forms the plan has left there cost more than the two launches.
        const bool gu_fused8 = fp8 && gemm256_swiglu_fills(T, 2 * I) && H % 128 == 0 && lc.mis_gu_w == 0;
        const LinearCall gc = linear_call(wqbits ? wqbits : 16, LinearOperands{x, gw, gsc, ws, T, H, 2 * I, EPI_SWIGLU_, c.int4_group},
                                          LinearScratch{slabs, wqbits ? ws : nullptr, lc.deq_bytes});
        if (nq && gu_fused8 && lc.ffn_gamma && lc.mis_gu_scale == 0) o.ffn_norm = PN_QUANT, o.gate_up = PG_E4M3_SWIGLU;
        else if (fp8) o.gate_up = gu_fused8 ? PG_FP8_SWIGLU : PG_TWO_LAUNCH;
        else if (wqbits) o.gate_up = (T < kWqPrefillRows || gemm256_swiglu_fills(T, 2 * I)) && plan_linear_wq(gc).route != LR_REFUSED ? PG_FUSED : PG_TWO_LAUNCH;
        else o.gate_up = plan_linear_f16(gc).route != LR_REFUSED ? PG_FUSED : PG_TWO_LAUNCH;
    }
    o.rope_done = o.qkv == PQ_ROPE_F16 || o.qkv == PQ_ROPE_W8 || o.qkv == PQ_ROPE_IMAGE || o.qkv == PQ_ROPE_E4M3 || o.qkv == PQ_ROPE_UNPACKED ||
                  o.qkv == PQ_SPLITK_ROPE;
    o.attn = plan_prefill_attn(batch, max_q_len, c.head_num, c.kv_fmt == LLMIE_KV_FP8, o.rope_done, 0, 0, p.tree);
    // (the split-K sequence's ATTN_NORM launch is the row kernel behind the down projection)
    for (int op : {LLMIE_OP_ATTN_NORM, LLMIE_OP_QKV_GEMM, LLMIE_OP_MHA, LLMIE_OP_O_GEMM, LLMIE_OP_FFN_NORM, LLMIE_OP_GATE_UP_SWIGLU, LLMIE_OP_DOWN_GEMM})
        o.launches[op] = 1;
    if (o.qkv == PQ_ROPE_UNPACKED || o.qkv == PQ_SPLITK || o.qkv == PQ_SPLITK_ROPE) o.launches[LLMIE_OP_QKV_GEMM] = 2;
    if (o.gate_up == PG_TWO_LAUNCH || o.gate_up == PG_UNPACK_TWO_LAUNCH || o.gate_up == PG_SPLITK) o.launches[LLMIE_OP_GATE_UP_SWIGLU] = 2;
    if (path == PP_LORA)   // shrink + expand behind each of the four projections
        for (int op : {LLMIE_OP_QKV_GEMM, LLMIE_OP_O_GEMM, LLMIE_OP_GATE_UP_SWIGLU, LLMIE_OP_DOWN_GEMM}) o.launches[op] += 2;
    return o;
}
// the PrefillCall llmie_decoder_plan_name / llmie_decoder_prefill_layer_plan describe with their call flags
static PrefillCall prefill_call_of_flags(const llmie_decoder_config &cfg, int tokens, unsigned call_flags, const EngineSwitches &sw) {
    return PrefillCall{cfg, tokens, !(call_flags & LLMIE_PLAN_WEIGHTS_MISALIGNED), !(call_flags & LLMIE_PLAN_SCALES_MISALIGNED),
                       !(call_flags & (LLMIE_PLAN_HIDDEN_MISALIGNED | LLMIE_PLAN_GAMMAS_MISALIGNED)), (call_flags & LLMIE_PLAN_O_BIAS) != 0, sw,
                       (call_flags & LLMIE_PLAN_LORA) != 0, false, (call_flags & LLMIE_PLAN_QK_NORM) != 0, (call_flags & LLMIE_PLAN_TREE) != 0};
}
// a draft tree and a sliding window / head sinks exclude each other (named follow-ups)
static const char *const kTreeRefusal =
    "a draft tree needs an engine with a prefill path (fp16 activations, head_size 128) and neither a sliding window nor head sinks set";
// what QK-norm needs of an engine's config (beside the geometry): nothing a config says rules it out but the geometry; the layers'
// QKV biases and the window / head-sink state are the engine's (llmie_decoder_set_qk_norm)
static bool qk_norm_engine_ok(const llmie_decoder_config &c) { return window_engine_ok(c); }

// Host-only: the launch sequence llmie_decoder_forward (prefill = 0, rows = batch) or llmie_decoder_prefill (prefill = 1, rows =
// tokens) plans for an engine of this config; NULL with llmie_last_error() set where the call -- or creating the engine -- is refused.
extern "C" const char *llmie_decoder_plan_name(const llmie_decoder_config *cfg, int prefill, int rows, unsigned call_flags,
                                               unsigned switch_mask) {
    if (!config_ok(cfg)) {
        set_error("decoder_plan_name: invalid config");
        return nullptr;
    }
    if ((cfg->flags & LLMIE_DEC_PACKED_ONLY) && !packed_wf(cfg)) {
        set_error("%s", packed_only_refusal(cfg));
        return nullptr;
    }
    const EngineSwitches sw = switches_of_mask(switch_mask);
    if ((call_flags & LLMIE_PLAN_WINDOW) && !window_engine_ok(*cfg)) {
        set_error("decoder_plan_name: %s", kWindowRefusal);
        return nullptr;
    }
    if ((call_flags & LLMIE_PLAN_HEAD_SINK) && !window_engine_ok(*cfg)) {
        set_error("decoder_plan_name: %s", kHeadSinkRefusal);
        return nullptr;
    }
    if ((call_flags & LLMIE_PLAN_QK_NORM) && (!qk_norm_engine_ok(*cfg) || (call_flags & (LLMIE_PLAN_WINDOW | LLMIE_PLAN_HEAD_SINK)))) {
        set_error("decoder_plan_name: %s", kQkNormRefusal);
        return nullptr;
    }
    if ((call_flags & LLMIE_PLAN_TREE) && (call_flags & (LLMIE_PLAN_WINDOW | LLMIE_PLAN_HEAD_SINK))) {
        set_error("decoder_plan_name: %s", kTreeRefusal);
        return nullptr;
    }
    if (prefill) {
        if (rows < 1) {
            set_error("decoder_plan_name: %d tokens", rows);
            return nullptr;
        }
        const PrefillPlan p = plan_prefill(prefill_call_of_flags(*cfg, rows, call_flags, sw));
        if (p.path == PP_REFUSED) return (void)prefill_refuse(p), nullptr;
        return prefill_path_name(p.path);
    }
    if (rows < 1 || rows > cfg->max_batch) {
        set_error("decoder_forward: batch %d outside [1,%d]", rows, cfg->max_batch);
        return nullptr;
    }
    const DecodeCall dc{*cfg, rows, (call_flags & LLMIE_PLAN_PAGED) != 0, (call_flags & LLMIE_PLAN_RAGGED) != 0,
                        (call_flags & LLMIE_PLAN_HIDDEN_MISALIGNED) ? 8u : 0u, (call_flags & LLMIE_PLAN_WEIGHTS_MISALIGNED) ? 8u : 0u, sw,
                        (call_flags & LLMIE_PLAN_LORA) != 0};
    const DecodePlan p = plan_decode(dc);
    if (p.path == DP_REFUSED) return (void)decode_refuse(dc, p), nullptr;
    return decode_path_name(p.path);
}

// the KV cache of an engine call (block_table null: dense caches)
static KvView kv_view(const llmie_decoder_config &c, void *k, void *v, const int32_t *block_table, int max_pages, int num_pages) {
    const bool fp8 = c.kv_fmt == LLMIE_KV_FP8;
    return KvView{k, v, block_table, max_pages, num_pages, fp8 ? 1 : 0, (fp8 && c.k_scale > 0.f) ? c.k_scale : 1.f,
                  (fp8 && c.v_scale > 0.f) ? c.v_scale : 1.f};
}

// One decode step: the call as every launch sequence reads it.  The sequences are members, so their bodies name the call's parts
// like locals.
struct DecodeStep {
    llmie_decoder *dec;
    const llmie_decoder_config &c;
    void *h;  // running hidden state, updated in place like decoder_output in the reference
    int batch;
    KvView kv;
    DecodePos pos;
    llmie_stream stream;
    hipStream_t st;
    int H, QKV, I, wbits;
    bool fp8;
    llmie_dtype dt;

    // attention with bias, the KV append and RoPE (rope = false: already applied) fused in front; out_x32: `out` is the x32 image of
    // the packed sequences
    int attention(const void *qkv, const void *qkv_bias, void *out, int layer, const SplitKSlabs *qkv_slabs = nullptr,
                  const SlabScale *qkv_scale = nullptr, int out_x32 = 0, bool rope = true) const {
        return decoder_mha_rope(DecodeAttnShape{batch, c.head_num, c.kv_head_num, c.head_size, c.max_seq_len, dt},
                                DecodeAttnIo{qkv, qkv_bias, out, dec->attn_ws, dec->attn_ws_bytes, rope ? dec->rope_table : nullptr,
                                             rope ? c.rotary_dim : 0, nullptr, qkv_slabs, qkv_scale, out_x32, dec->window_of(layer), dec->sinks,
                                             dec->head_sink_of(layer), dec->q_gamma_of(layer), dec->k_gamma_of(layer), dec->qk_eps},
                                kv, pos, layer, st);
    }

    // ---- fused fp16 decode path (batch <= 8): 5 launches per layer ----
    //   qkv  = rmsnorm(h)*g1 . Wqkv^T                      (norm fused into the GEMV prologue)
    //   mha  = attention(rope(q), rope(k) -> cache, v)     (RoPE + bias + KV append fused into the attention)
    //   h   += mha . Wo^T                                   (residual epilogue; h is the residual stream)
    //   act  = swiglu(rmsnorm(h + o.bias)*g2 . Wgu^T)      (norm prologue + SwiGLU epilogue)
    //   h   += act . Wd^T
    // Same math as self_decoder.cpp:69-119 (residual updated before the o.bias add, as the reference).
    int gemv() const {
        int rc;
        // (the in-launch merge of the attention partials -- the tickets argument of llmie_decoder_mha_rope -- measured SLOWER than the
        // separate 4.8 us merge kernel on MI355X, 2.97 vs 2.81 ms per token: every workgroup pays the release fence; the engine
        // always uses the merge kernel)
        // y = [swiglu]( rmsnorm(x + pre_bias)*gamma . W^T ) + residual on the streaming GEMV of the weight format
        const LinearScratch scratch = decode_scratch(dec);
        auto lin = [&](const void *x, const llmie_matrix &w, void *y, int K, int N, int epi, const void *residual,
                       const void *gamma, const void *pre_bias) -> int {
            const LinearOperands o = proj_operands(c, x, w, y, batch, K, N, epi, residual, gamma, pre_bias);
            // fp8 (e4m3 weights x per-token e4m3 activations): this sequence takes the GEMV wherever K fits its register budget, AHEAD of
            // plan_linear_fp8's shape rules (which ask K % 256 == 0 of every call: an inter_size of 1376 decodes on the GEMV); longer
            // rows (down projection at batch > 2) take what linear_fp8 plans.  (plan_decode: a projection with a fused norm or
            // SwiGLU has K = H, which the plan found GEMV-eligible)
            if (fp8 && ksplit_eligible(batch, K, 8)) return linear_fp8_gemv(o, st);
            return engine_proj(c.wfmt, o, scratch, dec->gu, stream);
        };
        for (int l = 0; l < c.num_layers; ++l) {
            const llmie_layer_weights &w = dec->layers[l];
            TIMED(LLMIE_OP_QKV_GEMM, lin(h, w.qkv, dec->qkv, H, QKV, EPI_NONE_, nullptr, w.attn_norm_gamma, nullptr));
            TIMED(LLMIE_OP_MHA, attention(dec->qkv, w.qkv.bias, dec->mha, l));
            TIMED(LLMIE_OP_O_GEMM, lin(dec->mha, w.o, h, H, H, EPI_NONE_, h, nullptr, nullptr));
            TIMED(LLMIE_OP_GATE_UP_SWIGLU, lin(h, w.gate_up, dec->act, H, 2 * I, EPI_SWIGLU_, nullptr, w.ffn_norm_gamma, w.o.bias));
            TIMED(LLMIE_OP_DOWN_GEMM, lin(dec->act, w.down, h, I, H, EPI_NONE_, h, nullptr, nullptr));
        }
        return LLMIE_OK;
    }

    // ---- packed-weight batch path (gemv_max < batch <= 32; fp16 / int8 weights, fp8 up to 16 rows): 6 launches per layer, no
    // fp32 slab round trip except the down projection's K split --
    //   qkv  = rmsnorm(h) * g1 . Wqkv^T            norm in the kernel's prologue (per-token factor in its epilogue), fp16 qkv rows
    //   mha  = attention(rope(q), rope(k) -> cache, v)
    //   hx   = h + mha . Wo^T                       residual epilogue, x32 image of the residual stream
    //   actx = swiglu(rmsnorm(hx + o.bias) * g2 . Wgu^T)
    //   hx  += actx . Wd^T                          K split over workgroups (K = inter_size) + one reduce launch
    // Same math as self_decoder.cpp:69-119.  Weights come from the tile-packed images built at create time.
    // The four projections of layer l on its packed images.  first: the layer reads the caller's row-major hidden state (from its O
    // projection on, the residual stream lives in the x32 image hx); last: its down projection writes the hidden state back row-major
    struct PackedLayerOps {
        PkOperands qkv, o, gate_up, down;
    };
    PackedLayerOps pk_layer(int l, bool first, bool last) const {
        const llmie_layer_weights &w = dec->layers[l];
        const llmie_decoder::PackedLayer &pw = dec->packed[l];
        half_t *hh = static_cast<half_t *>(h), *qkvb = reinterpret_cast<half_t *>(dec->qkv);
        // (int4: the packed group-scale image; else the caller's row scales)
        auto sc = [&](int i, const llmie_matrix &m) -> const void * { return pw.sc[i] ? pw.sc[i] : m.scale; };
        auto f16 = [](const void *p) { return static_cast<const half_t *>(p); };
        return PackedLayerOps{
            {first ? hh : dec->hx, pw.qkv, sc(0, w.qkv), qkvb, H, QKV, PKE_PLAIN, first ? 0 : PKX_X, nullptr, f16(w.attn_norm_gamma), nullptr, c.rms_eps,
             nullptr, 0},
            {dec->mhax, pw.o, sc(1, w.o), dec->hx, H, H, PKE_PLAIN, PKX_X | PKX_Y | (first ? 0 : PKX_RES), first ? hh : dec->hx, nullptr, nullptr, 0.f,
             nullptr, 0},
            {dec->hx, pw.gate_up, sc(2, w.gate_up), dec->actx, H, 2 * I, PKE_SWIGLU, PKX_X | PKX_Y, nullptr, f16(w.ffn_norm_gamma), f16(w.o.bias),
             c.rms_eps, nullptr, 0},
            {dec->actx, pw.down, sc(3, w.down), last ? hh : dec->hx, I, H, PKE_PLAIN, PKX_X | PKX_RES | (last ? 0 : PKX_Y), dec->hx, nullptr, nullptr,
             0.f, dec->pk_slab, dec->pk_slab_floats}};
    }
    int packed() const {
        int rc;
        const int wf = dec->pk_wf;
        for (int l = 0; l < c.num_layers; ++l) {
            const PackedLayerOps p = pk_layer(l, l == 0, l + 1 == c.num_layers);
            TIMED(LLMIE_OP_QKV_GEMM, pk_linear(wf, batch, p.qkv, st));
            TIMED(LLMIE_OP_MHA, attention(dec->qkv, dec->layers[l].qkv.bias, dec->mhax, l, nullptr, nullptr, 1));
            TIMED(LLMIE_OP_O_GEMM, pk_linear(wf, batch, p.o, st));
            TIMED(LLMIE_OP_GATE_UP_SWIGLU, pk_linear(wf, batch, p.gate_up, st));
            TIMED(LLMIE_OP_DOWN_GEMM, pk_linear(wf, batch, p.down, st));
        }
        return LLMIE_OK;
    }
    // Round 3, OPT-IN (LLMIE_CHAIN=1): ONE persistent launch per layer for the chain O -> gate/up -> down (-> slab reduce) -> next
    // layer's QKV (pk_gemm.cuh, pk_chain_kernel: grid barriers between the phases, the next phase's weight ring prefetched across
    // each): 2 launches per layer (attention + chain) instead of 6, the launches' own code per phase (bit-identical outputs).
    // Measured SLOWER than the launch sequence (int8, batch 32, MI355X: 94 us per chain against 78 us for the five launches it
    // replaces; phase-edge timestamps, DESIGN.md section 9: a phase inside the chain takes what its launch takes -- the ~8 us of
    // fixed cost per projection is the kernel's own prologue (activation slice, norm) and epilogue, not the launch -- and a grid
    // barrier costs 5.5-7 us against ~2.5 us for a launch boundary), so the launch sequence stays the default.
    // probe: can every projection of a layer join a chain at this batch?  (pk_chain_add validates shapes / plans / LDS)
    bool chain_joins() const {
        if (!dec->pk_sync) return false;
        const PackedLayerOps p = pk_layer(0, false, false);   // a middle layer's operands
        PkChain ch;
        pk_chain_begin(&ch, dec->pk_wf, batch);
        return ch.ok && !pk_chain_add(&ch, 0, p.o) && !pk_chain_add(&ch, 1, p.gate_up) && !pk_chain_add(&ch, 2, p.down) &&
               (c.num_layers == 1 || !pk_chain_add(&ch, 4, p.qkv));
    }
    int packed_chain() const {
        int rc;
        const int wf = dec->pk_wf;
        for (int l = 0; l < c.num_layers; ++l) {
            const bool first = l == 0, last = l + 1 == c.num_layers;
            const PackedLayerOps p = pk_layer(l, first, last);
            if (first) TIMED(LLMIE_OP_QKV_GEMM, pk_linear(wf, batch, p.qkv, st));
            TIMED(LLMIE_OP_MHA, attention(dec->qkv, dec->layers[l].qkv.bias, dec->mhax, l, nullptr, nullptr, 1));
            PkChain ch;
            pk_chain_begin(&ch, wf, batch);
            rc = pk_chain_add(&ch, 0, p.o);
            if (!rc) rc = pk_chain_add(&ch, 1, p.gate_up);
            if (!rc) rc = pk_chain_add(&ch, 2, p.down);
            if (!rc && !last) rc = pk_chain_add(&ch, 4, pk_layer(l + 1, false, false).qkv);
            if (rc) return rc;
            ch.stamps = dec->pk_stamps;   // (diagnostic; null unless llmie_decoder_debug_stamps armed it)
            TIMED(LLMIE_OP_CHAIN, pk_chain_launch(&ch, dec->pk_sync + static_cast<size_t>(l) * (pk_chain_sync_bytes() / sizeof(unsigned)), dec->pk_err, st));
        }
        return LLMIE_OK;
    }

    // ---- fused batch decode path (8 < batch <= 128; fp16, int8, int4 (<= 64) or fp8 weights): 8 launches per layer (+ the attention
    // merge when the context spans several chunks) instead of 11-12.  Every projection is a split-K MFMA launch that
    // leaves fp32 partial slabs; the consumer of each slab does the reduction:
    //   qkv slabs            -> read directly by the attention launch (q rows, new k/v rows; + scale, bias, RoPE, append)
    //   o / down slabs       -> splitk_rownorm: reduction + residual stream update + the NEXT RMSNorm in one launch
    //   gate_up slabs        -> finalize with the SwiGLU epilogue
    // (each small dependent launch costs ~4.5 us on MI355X, a third of a batch-32 int8 layer before this fusion)
    // fp8: activations enter every projection as per-token e4m3; the row kernel emits them directly for the qkv and
    // gate_up inputs, the attention and SwiGLU outputs take a quantize_rows launch each (10 launches per layer).
    int splitk() const {
        int rc;
        half_t *hh = static_cast<half_t *>(h), *resid = reinterpret_cast<half_t *>(dec->resid);
        half_t *mha = reinterpret_cast<half_t *>(dec->mha), *act = reinterpret_cast<half_t *>(dec->act);
        const int fmt = fp8 ? WF_FP8 : wbits;
        const size_t unit = dec->fp8_ws_bytes, kmax = static_cast<size_t>(I > H ? I : H);
        auto xq_of = [&](int u) { return fp8 ? reinterpret_cast<uint8_t *>(dec->fp8_ws) + u * unit : nullptr; };
        auto xs_of = [&](int u) {
            return fp8 ? reinterpret_cast<float *>(xq_of(u) + ((static_cast<size_t>(c.max_batch) * kmax + 255) & ~size_t(255))) : nullptr;
        };
        uint8_t *xqA = xq_of(0), *xqB = xq_of(1), *xqC = xq_of(2);
        float *xsA = xs_of(0), *xsB = xs_of(1), *xsC = xs_of(2);
        auto scale_of = [&](const llmie_matrix &m, const float *xs) {
            if (fp8) return SlabScale{nullptr, static_cast<const float *>(m.scale), xs};
            return SlabScale{wbits == 8 ? static_cast<const half_t *>(m.scale) : nullptr, nullptr, nullptr};
        };
        // int4: the group scales are applied inside the split-K kernel (the slabs hold scaled values)
        auto gs_of = [&](const llmie_matrix &m) { return wbits == 4 ? static_cast<const half_t *>(m.scale) : nullptr; };
        // self_decoder.cpp:77 (first layer only: later ones get it from the previous layer's down-projection epilogue)
        TIMED(LLMIE_OP_ATTN_NORM, llmie_rmsnorm(h, dec->resid, dec->layers[0].attn_norm_gamma, c.rms_eps, batch, H, dt, stream));
        if (fp8) TIMED(LLMIE_OP_ATTN_NORM, quantize_rows_fp8(hh, xqA, xsA, batch, H, st));
        for (int l = 0; l < c.num_layers; ++l) {
            const llmie_layer_weights &w = dec->layers[l];
            const bool last = l + 1 == c.num_layers;
            const void *xin = fp8 ? static_cast<const void *>(xqA) : hh;
            SplitKSlabs sk;
            TIMED(LLMIE_OP_QKV_GEMM, linear_splitk_partial(fmt, xin, w.qkv.data, batch, H, QKV, st, &sk, dec->slab_ws, gs_of(w.qkv)));
            const SlabScale qsc = scale_of(w.qkv, xsA);
            TIMED(LLMIE_OP_MHA, attention(nullptr, w.qkv.bias, dec->mha, l, &sk, &qsc));
            if (fp8) TIMED(LLMIE_OP_O_GEMM, quantize_rows_fp8(mha, xqB, xsB, batch, H, st));
            TIMED(LLMIE_OP_O_GEMM, linear_splitk_partial(fmt, fp8 ? static_cast<const void *>(xqB) : mha, w.o.data, batch, H, H, st, &sk, dec->slab_ws, gs_of(w.o)));
            // self_decoder.cpp:92  h += resid; resid = h; h += o.bias; h = rmsnorm(h, ffn_gamma)
            TIMED(LLMIE_OP_FFN_NORM, splitk_rownorm(sk, scale_of(w.o, xsB), static_cast<const half_t *>(w.o.bias), resid,
                                                    static_cast<const half_t *>(w.ffn_norm_gamma), c.rms_eps,
                                                    fp8 ? nullptr : hh, xqA, xsA, st));
            // ffn.cpp:105-122  act = silu(h.Wg^T) * (h.Wu^T)
            TIMED(LLMIE_OP_GATE_UP_SWIGLU, linear_splitk_partial(fmt, xin, w.gate_up.data, batch, H, 2 * I, st, &sk, dec->slab_ws, gs_of(w.gate_up)));
            TIMED(LLMIE_OP_GATE_UP_SWIGLU, splitk_finalize(sk, scale_of(w.gate_up, xsA), act, EPI_SWIGLU_, nullptr, nullptr, st));
            if (fp8) TIMED(LLMIE_OP_DOWN_GEMM, quantize_rows_fp8(act, xqC, xsC, batch, I, st));
            TIMED(LLMIE_OP_DOWN_GEMM, linear_splitk_partial(fmt, fp8 ? static_cast<const void *>(xqC) : act, w.down.data, batch, I, H, st, &sk, dec->slab_ws, gs_of(w.down)));
            // ffn.cpp:132 + self_decoder.cpp:111 h = act.Wd^T + resid, then the next layer's resid = h; h = rmsnorm(h)
            const void *next_gamma = last ? nullptr : dec->layers[l + 1].attn_norm_gamma;
            TIMED(LLMIE_OP_ATTN_NORM, splitk_rownorm(sk, scale_of(w.down, xsC), nullptr, resid, static_cast<const half_t *>(next_gamma),
                                                     c.rms_eps, (fp8 && !last) ? nullptr : hh, last ? nullptr : xqA, xsA, st));
        }
        return LLMIE_OK;
    }
    int unfused() const;
    int lora() const;
    int moe(const MoePlan &moe_plan) const;
};

// ---- the reference's launch sequence (self_decoder.cpp:69-119), one kernel per step; RoPE inside the attention launch where its
// geometry allows ----
int DecodeStep::unfused() const {
    int rc;
    const bool fused_rope = fused_attention_geometry(c);
    for (int l = 0; l < c.num_layers; ++l) {
        const llmie_layer_weights &w = dec->layers[l];
        // self_decoder.cpp:77  resid = h ; h = rmsnorm(h)
        TIMED(LLMIE_OP_ATTN_NORM, llmie_rmsnorm(h, dec->resid, w.attn_norm_gamma, c.rms_eps, batch, H, dt, stream));
        // self_attention.cpp:79  qkv = h . Wqkv^T   (bias is applied inside the MHA kernel, as the reference)
        TIMED(LLMIE_OP_QKV_GEMM, engine_linear(dec, c.wfmt, proj_operands(c, h, w.qkv, dec->qkv, batch, H, QKV, EPI_NONE_, nullptr), stream));
        if (fused_rope) {
            // :100-:108 RoPE at position step-1 + fused masked MHA with KV append, one launch (+ merge)
            TIMED(LLMIE_OP_MHA, attention(dec->qkv, w.qkv.bias, dec->mha, l));
        } else {
            // :100 RoPE at position step-1
            TIMED(LLMIE_OP_ROPE, llmie_rope_decode(dec->qkv, batch, c.head_num, c.kv_head_num, c.head_size, pos.step, pos.step_dev,
                                                   c.rotary_dim, c.rotary_base, dt, stream));
            // :108 fused masked MHA with KV append
            TIMED(LLMIE_OP_MHA, attention(dec->qkv, w.qkv.bias, dec->mha, l, nullptr, nullptr, 0, false));
        }
        // :131 output projection (no bias here: the fused norm below adds o.bias, self_decoder.cpp:92-98)
        TIMED(LLMIE_OP_O_GEMM, engine_linear(dec, c.wfmt, proj_operands(c, dec->mha, w.o, h, batch, H, H, EPI_NONE_, nullptr), stream));
        // self_decoder.cpp:92  h += resid; resid = h; h += o.bias; h = rmsnorm(h, ffn_gamma)
        TIMED(LLMIE_OP_FFN_NORM, llmie_fused_add_bias_residual_rmsnorm(dec->resid, h, w.o.bias, w.ffn_norm_gamma,
                                                                       c.rms_eps, batch, H, dt, stream));
        // ffn.cpp:105-122  act = silu(h.Wg^T) * (h.Wu^T)
        TIMED(LLMIE_OP_GATE_UP_SWIGLU, engine_linear(dec, c.wfmt, proj_operands(c, h, w.gate_up, dec->act, batch, H, 2 * I, EPI_SWIGLU_, nullptr), stream));
        // ffn.cpp:132 + self_decoder.cpp:111  h = act . Wd^T + resid
        TIMED(LLMIE_OP_DOWN_GEMM, engine_linear(dec, c.wfmt, proj_operands(c, dec->act, w.down, h, batch, I, H, EPI_NONE_, dec->resid), stream));
    }
    return LLMIE_OK;
}

// the attach call's scratch must cover this call's rows: checked before anything is enqueued
static int lora_rows_fit(const llmie_decoder *d, int rows, const char *who) {
    const size_t need = llmie_lora_workspace_bytes(rows, d->lora.slots, 192);
    if (d->lora.ws_bytes < need) {
        set_error("%s: the adapter workspace given to llmie_decoder_lora_attach does not cover %d rows (%zu < %zu)", who, rows, d->lora.ws_bytes, need);
        return LLMIE_ERR_WORKSPACE;
    }
    return LLMIE_OK;
}

// one adapter update of the lora sequences: y += scale . B . (A . x) per row, shrink + expand on the plan this call's plan launch left
static int engine_lora(const llmie_decoder *d, const void *x, void *y, int rows, int K, int N, int blocks, const int *widths, int layer,
                       int module, llmie_stream stream) {
    return llmie_lora_apply(x, y, rows, K, N, blocks, widths, d->lora.table, d->lora.slots, d->cfg.num_layers, layer, module, d->lora.ws,
                            d->lora.ws_bytes, LLMIE_F16, stream);
}

// ---- per-request adapters: the unfused sequence, every projection followed by its adapter update where the update's input is
// materialised (the QKV one before RoPE: the attention launch rotates); gate/up as projection + update + llmie_silu_and_mul ----
int DecodeStep::lora() const {
    int rc;
    const int qkv_w[3] = {c.head_num * c.head_size, c.kv_head_num * c.head_size, c.kv_head_num * c.head_size}, gu_w[2] = {I, I};
    if ((rc = llmie_lora_plan(dec->lora.seq_slot, nullptr, batch, batch, dec->lora.table, dec->lora.slots, dec->lora.ws, dec->lora.ws_bytes, stream)))
        return rc;
    for (int l = 0; l < c.num_layers; ++l) {
        const llmie_layer_weights &w = dec->layers[l];
        TIMED(LLMIE_OP_ATTN_NORM, llmie_rmsnorm(h, dec->resid, w.attn_norm_gamma, c.rms_eps, batch, H, dt, stream));
        TIMED(LLMIE_OP_QKV_GEMM, engine_linear(dec, c.wfmt, proj_operands(c, h, w.qkv, dec->qkv, batch, H, QKV, EPI_NONE_, nullptr), stream));
        TIMED(LLMIE_OP_QKV_GEMM, engine_lora(dec, h, dec->qkv, batch, H, QKV, 3, qkv_w, l, LLMIE_LORA_QKV, stream));
        if (fused_attention_geometry(c)) {
            TIMED(LLMIE_OP_MHA, attention(dec->qkv, w.qkv.bias, dec->mha, l));
        } else {
            TIMED(LLMIE_OP_ROPE, llmie_rope_decode(dec->qkv, batch, c.head_num, c.kv_head_num, c.head_size, pos.step, pos.step_dev,
                                                   c.rotary_dim, c.rotary_base, dt, stream));
            TIMED(LLMIE_OP_MHA, attention(dec->qkv, w.qkv.bias, dec->mha, l, nullptr, nullptr, 0, false));
        }
        TIMED(LLMIE_OP_O_GEMM, engine_linear(dec, c.wfmt, proj_operands(c, dec->mha, w.o, h, batch, H, H, EPI_NONE_, nullptr), stream));
        TIMED(LLMIE_OP_O_GEMM, engine_lora(dec, dec->mha, h, batch, H, H, 1, &H, l, LLMIE_LORA_O, stream));
        TIMED(LLMIE_OP_FFN_NORM, llmie_fused_add_bias_residual_rmsnorm(dec->resid, h, w.o.bias, w.ffn_norm_gamma, c.rms_eps, batch, H, dt, stream));
        TIMED(LLMIE_OP_GATE_UP_SWIGLU, engine_linear(dec, c.wfmt, proj_operands(c, h, w.gate_up, dec->gu, batch, H, 2 * I, EPI_NONE_, nullptr), stream));
        TIMED(LLMIE_OP_GATE_UP_SWIGLU, engine_lora(dec, h, dec->gu, batch, H, 2 * I, 2, gu_w, l, LLMIE_LORA_GATE_UP, stream));
        TIMED(LLMIE_OP_GATE_UP_SWIGLU, llmie_silu_and_mul(dec->gu, dec->act, batch, I, dt, stream));
        TIMED(LLMIE_OP_DOWN_GEMM, engine_linear(dec, c.wfmt, proj_operands(c, dec->act, w.down, h, batch, I, H, EPI_NONE_, dec->resid), stream));
        TIMED(LLMIE_OP_DOWN_GEMM, engine_lora(dec, dec->act, h, batch, I, H, 1, &H, l, LLMIE_LORA_DOWN, stream));
    }
    return LLMIE_OK;
}

// the attach call's scratch must cover this call's rows: checked before anything is enqueued.  The call's one plan is made here
static int moe_rows_fit(const llmie_decoder *d, int rows, const char *who, MoePlan *plan) {
    MoeCall c = d->moe.call;
    c.rows = rows;
    const size_t need = llmie_moe_workspace_bytes(rows, c.H, c.Ie, c.E, c.k);
    if (d->moe.ws_bytes < need) {
        set_error("%s: the workspace given to llmie_decoder_moe_attach does not cover %d rows (%zu < %zu)", who, rows, d->moe.ws_bytes, need);
        return LLMIE_ERR_WORKSPACE;
    }
    // and the attach flags must hold at this row count (LLMIE_MOE_FORCE_GEMV has a row limit)
    return moe_call_check(who, c, plan);
}
// the FFN of a layer with a router, h = moe_ffn(h) + resid, under the call's plan: prepared once, its stages under the op kinds of a
// dense layer's FFN launches
static int engine_moe_ffn(llmie_decoder *dec, const MoePlan &plan, int layer, void *h, const void *resid, llmie_stream stream) {
    int rc;
    MoePrepared m;
    const MoeOperands o{h, resid, h, &dec->moe.layers[layer], dec->moe.ws, dec->moe.ws_bytes, LLMIE_F16};
    if ((rc = moe_prepare("moe_ffn", plan.call, o, &plan, &m))) return rc;
    TIMED(LLMIE_OP_FFN_NORM, moe_launch(m, MOE_STAGE_ROUTE, as_stream(stream)));
    TIMED(LLMIE_OP_GATE_UP_SWIGLU, moe_launch(m, MOE_STAGE_GATE_UP, as_stream(stream)));
    TIMED(LLMIE_OP_DOWN_GEMM, moe_launch(m, MOE_STAGE_DOWN, as_stream(stream)));
    return LLMIE_OK;
}

// ---- experts attached: the unfused sequence; a layer with a router runs route + expert FFN (the down projection's residual through
// `resid`) where a dense layer runs its gate/up and down launches ----
int DecodeStep::moe(const MoePlan &moe_plan) const {
    int rc;
    for (int l = 0; l < c.num_layers; ++l) {
        const llmie_layer_weights &w = dec->layers[l];
        TIMED(LLMIE_OP_ATTN_NORM, llmie_rmsnorm(h, dec->resid, w.attn_norm_gamma, c.rms_eps, batch, H, dt, stream));
        TIMED(LLMIE_OP_QKV_GEMM, engine_linear(dec, c.wfmt, proj_operands(c, h, w.qkv, dec->qkv, batch, H, QKV, EPI_NONE_, nullptr), stream));
        if (fused_attention_geometry(c)) {
            TIMED(LLMIE_OP_MHA, attention(dec->qkv, w.qkv.bias, dec->mha, l));
        } else {
            TIMED(LLMIE_OP_ROPE, llmie_rope_decode(dec->qkv, batch, c.head_num, c.kv_head_num, c.head_size, pos.step, pos.step_dev,
                                                   c.rotary_dim, c.rotary_base, dt, stream));
            TIMED(LLMIE_OP_MHA, attention(dec->qkv, w.qkv.bias, dec->mha, l, nullptr, nullptr, 0, false));
        }
        TIMED(LLMIE_OP_O_GEMM, engine_linear(dec, c.wfmt, proj_operands(c, dec->mha, w.o, h, batch, H, H, EPI_NONE_, nullptr), stream));
        TIMED(LLMIE_OP_FFN_NORM, llmie_fused_add_bias_residual_rmsnorm(dec->resid, h, w.o.bias, w.ffn_norm_gamma, c.rms_eps, batch, H, dt, stream));
        if (dec->moe.layers[l].router) {
            if ((rc = engine_moe_ffn(dec, moe_plan, l, h, dec->resid, stream))) return rc;
        } else {
            TIMED(LLMIE_OP_GATE_UP_SWIGLU, engine_linear(dec, c.wfmt, proj_operands(c, h, w.gate_up, dec->act, batch, H, 2 * I, EPI_SWIGLU_, nullptr), stream));
            TIMED(LLMIE_OP_DOWN_GEMM, engine_linear(dec, c.wfmt, proj_operands(c, dec->act, w.down, h, batch, I, H, EPI_NONE_, dec->resid), stream));
        }
    }
    return LLMIE_OK;
}

// every decode entry point: validate, copy hidden_in, plan, refuse or dispatch
static int decoder_forward(llmie_decoder *dec, const void *hidden_in, void *hidden_out, void *k_cache, void *v_cache,
                           const int32_t *block_table, int max_pages, int num_pages, int batch, const DecodePos &pos, llmie_stream stream) {
    LLMIE_REQUIRE(dec && hidden_in && hidden_out && k_cache && v_cache, "decoder_forward: NULL pointer");
    const llmie_decoder_config &c = dec->cfg;
    LLMIE_REQUIRE(batch >= 1 && batch <= c.max_batch, "decoder_forward: batch %d outside [1,%d]", batch, c.max_batch);
    LLMIE_REQUIRE(pos.step_dev || (pos.step >= 1 && pos.step <= c.max_seq_len), "decoder_forward: step %d outside [1,%d]", pos.step,
                  c.max_seq_len);
    if (dec->lora.table)
        if (int rc = lora_rows_fit(dec, batch, "decoder_forward")) return rc;
    MoePlan moe_plan{};
    if (dec->moe.on() && !dec->lora.table)
        if (int rc = moe_rows_fit(dec, batch, "decoder_forward", &moe_plan)) return rc;
    if (hidden_out != hidden_in) {
        hipError_t e = hipMemcpyAsync(hidden_out, hidden_in, static_cast<size_t>(batch) * dec->H * dec->esz,
                                      hipMemcpyDeviceToDevice, as_stream(stream));
        if (e != hipSuccess) {
            set_error("decoder_forward: copy failed: %s", hipGetErrorString(e));
            return LLMIE_ERR_LAUNCH;
        }
    }
    const DecodeCall call{c, batch, block_table != nullptr, pos.ragged != 0, mis16(hidden_out), mis16(dec->layers[0].qkv.data), engine_switches(),
                          dec->lora.table != nullptr, dec->moe.on()};
    const DecodePlan plan = plan_decode(call);
    const DecodeStep s{dec, c, hidden_out, batch, kv_view(c, k_cache, v_cache, block_table, max_pages, num_pages), pos, stream, as_stream(stream),
                       dec->H, dec->QKV, dec->I, c.wfmt == LLMIE_W_F16 ? 16 : (c.wfmt == LLMIE_W_INT8 ? 8 : (c.wfmt == LLMIE_W_INT4 ? 4 : 0)),
                       c.wfmt == LLMIE_W_FP8, c.dtype};
    switch (plan.path) {
        case DP_GEMV: return s.gemv();
        case DP_PACKED: return plan.chain_wanted && s.chain_joins() ? s.packed_chain() : s.packed();
        case DP_SPLITK: return s.splitk();
        case DP_UNFUSED: return s.unfused();
        case DP_LORA: return s.lora();
        case DP_MOE: return s.moe(moe_plan);
        default: return decode_refuse(call, plan);
    }
}

extern "C" int llmie_decoder_forward(llmie_decoder *dec, const void *hidden_in, void *hidden_out, void *k_cache,
                                     void *v_cache, int batch, int step, const int32_t *step_dev,
                                     llmie_stream stream) {
    return decoder_forward(dec, hidden_in, hidden_out, k_cache, v_cache, nullptr, 0, 0, batch, DecodePos{step, step_dev, 0}, stream);
}

// Ragged batch (continuous batching): ctx_len_dev[b] = context length of sequence b including this step's token.  Every
// projection is row-wise, so only the attention launch sees the difference (RoPE position, append slot, span per sequence).
extern "C" int llmie_decoder_forward_ragged(llmie_decoder *dec, const void *hidden_in, void *hidden_out, void *k_cache,
                                            void *v_cache, int batch, const int32_t *ctx_len_dev, llmie_stream stream) {
    LLMIE_REQUIRE(dec && ctx_len_dev, "decoder_forward_ragged: NULL pointer");
    return decoder_forward(dec, hidden_in, hidden_out, k_cache, v_cache, nullptr, 0, 0, batch, DecodePos{-1, ctx_len_dev, 1}, stream);
}

static int paged_args_ok(const llmie_decoder *dec, const int32_t *block_table, int max_pages, int num_pages, const char *who) {
    LLMIE_REQUIRE(dec && block_table, "%s: NULL pointer", who);
    LLMIE_REQUIRE(max_pages > 0 && num_pages > 0 &&
                      static_cast<long long>(max_pages) * LLMIE_KV_PAGE_TOKENS >= dec->cfg.max_seq_len,
                  "%s: max_pages * %d must cover max_seq_len %d", who, LLMIE_KV_PAGE_TOKENS, dec->cfg.max_seq_len);
    return LLMIE_OK;
}

extern "C" int llmie_decoder_forward_paged_ragged(llmie_decoder *dec, const void *hidden_in, void *hidden_out, void *k_pool,
                                                  void *v_pool, const int32_t *block_table, int max_pages, int num_pages, int batch,
                                                  const int32_t *ctx_len_dev, llmie_stream stream) {
    LLMIE_REQUIRE(dec && ctx_len_dev, "decoder_forward_paged_ragged: NULL pointer");
    if (int rc = paged_args_ok(dec, block_table, max_pages, num_pages, "decoder_forward_paged")) return rc;
    return decoder_forward(dec, hidden_in, hidden_out, k_pool, v_pool, block_table, max_pages, num_pages, batch, DecodePos{-1, ctx_len_dev, 1},
                           stream);
}

extern "C" int llmie_decoder_forward_paged(llmie_decoder *dec, const void *hidden_in, void *hidden_out, void *k_pool, void *v_pool,
                                           const int32_t *block_table, int max_pages, int num_pages, int batch, int step,
                                           const int32_t *step_dev, llmie_stream stream) {
    if (int rc = paged_args_ok(dec, block_table, max_pages, num_pages, "decoder_forward_paged")) return rc;
    return decoder_forward(dec, hidden_in, hidden_out, k_pool, v_pool, block_table, max_pages, num_pages, batch, DecodePos{step, step_dev, 0},
                           stream);
}

// slabs of a prefill pass: the engine format's plans up to 192 rows, and -- beyond, where fp16 engines and the fp16 weight images of
// int4 / packed-only engines may run a projection as 128-row split-K passes -- what the fp16 projections reserve at T rows
static size_t prefill_slab_floats(const llmie_decoder_config *c, int T) {
    size_t m = engine_slab_floats(c, T < 192 ? T : 192);
    if (T > 192 && c->wfmt != LLMIE_W_FP8) {
        const int H = c->head_num * c->head_size, QKV = (c->head_num + 2 * c->kv_head_num) * c->head_size, I = c->inter_size;
        const int shapes[4][2] = {{H, QKV}, {H, H}, {H, 2 * I}, {I, H}};
        for (const auto &sh : shapes) {
            const size_t f = linear_f16_reserve_slab_floats(T, sh[0], sh[1]);
            m = f > m ? f : m;
        }
    }
    return m;
}
// the prefill workspace: offsets of its areas, in carve order
struct PrefillCarve {
    size_t resid, qkv, attn, gu, act, pad, cum, fp8_ws, slabs, deq, tokens, total;
};
static PrefillCarve prefill_carve(const llmie_decoder_config *c, int T, int B) {
    const size_t e = 2, H = static_cast<size_t>(c->head_num) * c->head_size;
    const size_t QKV = static_cast<size_t>(c->head_num + 2 * c->kv_head_num) * c->head_size, I = c->inter_size;
    Carve k;
    PrefillCarve o;
    o.resid = k.take(static_cast<size_t>(T) * H * e);
    o.qkv = k.take(static_cast<size_t>(T) * QKV * e);      // packed qkv
    o.attn = k.take(static_cast<size_t>(T) * H * e);       // attention output
    o.gu = k.take(static_cast<size_t>(T) * 2 * I * e);
    o.act = k.take(static_cast<size_t>(T) * I * e);
    o.pad = k.take(static_cast<size_t>(T) * sizeof(int32_t));        // padding offsets (by-product of the prefix kernel)
    o.cum = k.take(static_cast<size_t>(B + 1) * sizeof(int32_t));    // cum_seqlens
    // fp8 engines: per-token e4m3 image + scales of the activation matrix entering each projection
    o.fp8_ws = k.take(c->wfmt == LLMIE_W_FP8 ? llmie_linear_fp8_workspace_bytes(T, static_cast<int>(I > H ? I : H), 0) : 256);
    o.slabs = k.take(prefill_slab_floats(c, T) * sizeof(float) + 256);   // split-K slabs (short prefills; fp8 passes; mid-size fp16 passes)
    // int8 / int4 / packed-only engines: room for the fp16 image of the largest matrix, at every T -- at least the image_bytes of any
    // plan (plan_linear_wq's image routes; packed-only engines unpack every matrix), and more where the plan needs none: kept
    size_t dq = 0;
    if (c->wfmt == LLMIE_W_INT8 || c->wfmt == LLMIE_W_INT4 || c->wfmt == LLMIE_W_MXFP4 || (c->flags & LLMIE_DEC_PACKED_ONLY)) {
        const size_t shapes[4][2] = {{H, QKV}, {H, H}, {H, 2 * I}, {I, H}};
        for (const auto &sh : shapes) {
            const size_t b = sh[0] * sh[1] * sizeof(half_t);
            dq = b > dq ? b : dq;
        }
    }
    o.deq = k.take(dq + 256);
    o.tokens = k.take(static_cast<size_t>(T) * 2 * sizeof(int32_t) + 256);   // QkvRopeArgs, then (sequence, cache position) of every packed token
    o.total = k.off;
    return o;
}

extern "C" size_t llmie_decoder_prefill_workspace_bytes(const llmie_decoder_config *cfg, int max_tokens, int max_batch) {
    if (!config_ok(cfg) || max_tokens <= 0 || max_batch <= 0) return 0;
    return prefill_carve(cfg, max_tokens, max_batch).total;
}

// One prefill pass: the call, its workspace areas and the projections every launch sequence shares.  The sequences are members, so
// their bodies name the call's parts like locals.  Which form each launch of a layer takes is plan_prefill_layer's answer for that
// layer's operands; the sequences run it.
struct PrefillPass {
    llmie_decoder *dec;
    const llmie_decoder_config &c;
    const PrefillCall &call;
    int path;
    llmie_stream stream;
    hipStream_t st;
    KvView kv;
    const int32_t *cum, *history_lengths;
    int batch, T, max_q_len, H, QKV, I;
    bool fp8;
    int wqbits;   // weight-only int8 / int4: the same layer sequence on the quantised matrices -- the projections de-quantise inside
                  // the GEMM (int8: gemm8p.cuh WQ form) or through an fp16 image of one matrix at a time (int4; quant_linear.hip)
    half_t *h, *resid, *qkv, *attn, *gu, *act;
    void *f8ws;
    size_t f8ws_bytes;
    SlabWs slabs;
    void *deq;
    size_t deq_bytes;
    QkvRopeArgs *rope_args;   // (device copy of the fused QKV epilogue's operands)

    PrefillLayerPlan layer_plan(const llmie_layer_weights &w) const {
        return plan_prefill_layer(call, path, batch, max_q_len,
                                  PrefillLayerCall{mis16(w.qkv.data), mis16(w.qkv.scale), mis16(w.qkv.bias), mis16(w.gate_up.data),
                                                   mis16(w.gate_up.scale), mis16(h), w.ffn_norm_gamma != nullptr, slabs.floats, deq_bytes});
    }
    // a form this sequence has no launch for: the planner and the sequence disagree
    int bad_form(const char *what, int form) const {
        set_error("decoder_prefill: the %s sequence cannot run %s form %d", prefill_path_name(path), what, form);
        return LLMIE_ERR_UNSUPPORTED;
    }
    // e4m3 rows + token scales the quantising norms leave for the projection behind them
    uint8_t *xqn() const { return static_cast<uint8_t *>(f8ws); }
    float *xsn() const { return reinterpret_cast<float *>(xqn() + ((static_cast<size_t>(T) * H + 255) & ~static_cast<size_t>(255))); }
    // the pass's scratch: the split-K slabs, the area of the fp16 image of quantised (int8 / int4 / MXFP4) weights, the fp8 activations
    LinearScratch scratch() const { return LinearScratch{slabs, deq, deq_bytes, f8ws, f8ws_bytes}; }
    // y = [swiglu]( x . W^T ) (+ residual) in the engine's weight format (fp8: per-token e4m3 activations, fp8 MFMA)
    int proj(const half_t *x, const llmie_matrix &w, half_t *y, int K, int N, const half_t *residual, int epi = EPI_NONE_) const {
        return engine_proj(c.wfmt, proj_operands(c, x, w, y, T, K, N, epi, residual), scratch(), gu, stream);
    }
    // the two norms of the lean (out of place: h stays the residual stream) and general sequences
    int norm_form(int form) const { return (path == PP_LEAN) == (form == PN_OOP) ? form : -1; }
    int attn_norm(int form, const llmie_layer_weights &w) const {
        const half_t *g = (const half_t *)w.attn_norm_gamma;
        switch (norm_form(form)) {
            case PN_INPLACE: return llmie_rmsnorm(h, resid, g, c.rms_eps, T, H, LLMIE_F16, stream);
            case PN_OOP: return rmsnorm_oop_f16(h, resid, g, c.rms_eps, T, H, st);
            case PN_QUANT: return rmsnorm_quant_f16(h, resid, nullptr, g, c.rms_eps, T, H, false, xqn(), xsn(), st);
            default: return bad_form("attention norm", form);
        }
    }
    int ffn_norm(int form, const llmie_layer_weights &w) const {
        const half_t *g = (const half_t *)w.ffn_norm_gamma;
        switch (norm_form(form)) {
            case PN_INPLACE: return llmie_fused_add_bias_residual_rmsnorm(resid, h, w.o.bias, g, c.rms_eps, T, H, LLMIE_F16, stream);
            case PN_OOP: return rmsnorm_oop_f16(h, resid, g, c.rms_eps, T, H, st);
            case PN_QUANT: return rmsnorm_quant_f16(h, resid, (const half_t *)w.o.bias, g, c.rms_eps, T, H, true, xqn(), xsn(), st);
            default: return bad_form("FFN norm", form);
        }
    }
    // xs: token scales of e4m3 operands
    int qkv_rope(int l, const llmie_matrix &w, G256Operands ops, const void *x, const float *xs, const void *Wd, const void *wsc) const {
        gemm256_qkv_rope_launch(ops, x, Wd, qkv, T, QKV, H, xs, static_cast<const float *>(wsc), static_cast<const half_t *>(w.bias), rope_args, l, st);
        return launch_status("decoder_prefill(qkv + rope + append)");
    }
    // the QKV projection of the lean and general sequences, on the normalised rows x (the e4m3 forms: on the quantising norm's)
    int qkv_proj(int l, const llmie_matrix &w, const half_t *x, int form) const {
        switch (form) {
            case PQ_PLAIN: return proj(x, w, qkv, H, QKV, nullptr);
            case PQ_ROPE_F16: return qkv_rope(l, w, G256_F16, x, nullptr, w.data, nullptr);
            case PQ_ROPE_W8: return qkv_rope(l, w, G256_W8, x, nullptr, w.data, w.scale);
            case PQ_ROPE_IMAGE:
                if (int rc = dequantize_weights_f16(wqbits, w.data, static_cast<const half_t *>(w.scale), static_cast<half_t *>(deq), QKV, H, c.int4_group, st)) return rc;
                return qkv_rope(l, w, G256_F16, x, nullptr, deq, nullptr);
            case PQ_ROPE_E4M3: return qkv_rope(l, w, G256_E4M3, xqn(), xsn(), w.data, w.scale);
            case PQ_PLAIN_E4M3:
                gemm256_launch(G256_E4M3, xqn(), w.data, qkv, T, QKV, H, nullptr, nullptr, xsn(), (const float *)w.scale, st);
                return launch_status("decoder_prefill(qkv fp8)");
            default: return bad_form("QKV", form);
        }
    }
    int attention(int l, const llmie_matrix &wqkv, const PrefillLayerPlan &lp) const {
        PrefillAttnPlan ap = lp.attn;   // (the layer plan is per pass; the window is per layer)
        ap.window = dec->window_of(l), ap.sinks = ap.window > 0 ? dec->sinks : 0;
        ap.head_sink = dec->head_sinks != nullptr;
        return prefill_attention_f16(ap, kv, qkv, (const half_t *)wqkv.bias, attn, cum, history_lengths, dec->rope_table, l, T, c.kv_head_num,
                                     c.max_seq_len, c.rotary_dim, st, dec->head_sink_of(l),
                                     PrefillQkNorm{dec->q_gamma_of(l), dec->k_gamma_of(l), dec->qk_eps},
                                     PrefillTree{dec->tree_depth, dec->tree_anc, dec->tree_stride});
    }
    // act = swiglu(x . Wgu^T) of the lean and general sequences (ffn.cpp:105-122)
    int gate_up(const half_t *x, const llmie_matrix &w, int form) const {
        int rc;
        switch (form) {
            case PG_FUSED:
                TIMED(LLMIE_OP_GATE_UP_SWIGLU, proj(x, w, act, H, 2 * I, nullptr, EPI_SWIGLU_));
                return LLMIE_OK;
            case PG_E4M3_SWIGLU:
                TIMED(LLMIE_OP_GATE_UP_SWIGLU, (gemm256_swiglu_launch(G256_E4M3, xqn(), w.data, act, T, 2 * I, H, xsn(), (const float *)w.scale, st),
                                                launch_status("decoder_prefill(gate_up fp8)")));
                return LLMIE_OK;
            case PG_FP8_SWIGLU:
                TIMED(LLMIE_OP_GATE_UP_SWIGLU, llmie_linear_fp8_swiglu(x, (const uint8_t *)w.data, (const float *)w.scale, act, T, H, 2 * I, f8ws, f8ws_bytes, stream));
                return LLMIE_OK;
            case PG_TWO_LAUNCH:
                TIMED(LLMIE_OP_GATE_UP_SWIGLU, proj(x, w, gu, H, 2 * I, nullptr));
                TIMED(LLMIE_OP_GATE_UP_SWIGLU, llmie_silu_and_mul(gu, act, T, I, LLMIE_F16, stream));
                return LLMIE_OK;
            default: return bad_form("gate/up", form);
        }
    }
    int packed_only() const {
        int rc;
        // LLMIE_DEC_PACKED_ONLY: the row-major matrices are gone -- every projection unpacks its tile-packed image (scales applied,
        // one fp16 rounding per weight: the numerics of the int4 prefill) into the workspace and runs the fp16 GEMM on it
        auto pproj = [&](const void *img, const void *scale, int swiglu_img, const half_t *x, half_t *y, int K, int N, int epi,
                         const half_t *residual) -> int {
            if (deq_bytes < static_cast<size_t>(N) * K * sizeof(half_t)) {
                set_error("decoder_prefill: workspace holds no room for the fp16 image of a %d x %d matrix", N, K);
                return LLMIE_ERR_WORKSPACE;
            }
            int rc2 = pk_unpack_f16(dec->pk_wf, img, static_cast<const half_t *>(scale), static_cast<half_t *>(deq), N, K, swiglu_img, st);
            if (rc2) return rc2;
            return linear_f16_nk(LinearOperands{x, deq, nullptr, y, T, K, N, epi, 0, nullptr, residual}, LinearScratch{slabs}, st);
        };
        for (int l = 0; l < c.num_layers; ++l) {
            const llmie_layer_weights &w = dec->layers[l];
            const llmie_decoder::PackedLayer &pw = dec->packed[l];
            const PrefillLayerPlan lp = layer_plan(w);
            TIMED(LLMIE_OP_ATTN_NORM, llmie_rmsnorm(h, resid, w.attn_norm_gamma, c.rms_eps, T, H, LLMIE_F16, stream));
            switch (lp.qkv) {
                case PQ_ROPE_UNPACKED:   // (the unpacked fp16 image as the operand of the QKV projection with the RoPE + append epilogue)
                    TIMED(LLMIE_OP_QKV_GEMM, pk_unpack_f16(dec->pk_wf, pw.qkv, static_cast<const half_t *>(w.qkv.scale), static_cast<half_t *>(deq), QKV, H, 0, st));
                    TIMED(LLMIE_OP_QKV_GEMM, qkv_rope(l, w.qkv, G256_F16, h, nullptr, deq, nullptr));
                    break;
                case PQ_UNPACK_PLAIN: TIMED(LLMIE_OP_QKV_GEMM, pproj(pw.qkv, w.qkv.scale, 0, h, qkv, H, QKV, EPI_NONE_, nullptr)); break;
                default: return bad_form("QKV", lp.qkv);
            }
            TIMED(LLMIE_OP_MHA, attention(l, w.qkv, lp));
            TIMED(LLMIE_OP_O_GEMM, pproj(pw.o, w.o.scale, 0, attn, h, H, H, EPI_NONE_, nullptr));
            TIMED(LLMIE_OP_FFN_NORM, llmie_fused_add_bias_residual_rmsnorm(resid, h, w.o.bias, w.ffn_norm_gamma, c.rms_eps, T, H, LLMIE_F16, stream));
            switch (lp.gate_up) {
                case PG_UNPACK_FUSED: TIMED(LLMIE_OP_GATE_UP_SWIGLU, pproj(pw.gate_up, w.gate_up.scale, 1, h, act, H, 2 * I, EPI_SWIGLU_, nullptr)); break;
                case PG_UNPACK_TWO_LAUNCH:
                    TIMED(LLMIE_OP_GATE_UP_SWIGLU, pproj(pw.gate_up, w.gate_up.scale, 1, h, gu, H, 2 * I, EPI_NONE_, nullptr));
                    TIMED(LLMIE_OP_GATE_UP_SWIGLU, llmie_silu_and_mul(gu, act, T, I, LLMIE_F16, stream));
                    break;
                default: return bad_form("gate/up", lp.gate_up);
            }
            TIMED(LLMIE_OP_DOWN_GEMM, pproj(pw.down, w.down.scale, 0, act, h, I, H, EPI_NONE_, resid));
        }
        return LLMIE_OK;
    }
    // Short prefills (<= 128 tokens, fp16 weights) are weight-stream bound like a decode batch: same launch fusion as the batch
    // decode path -- every projection leaves split-K slabs, the O and down slabs are consumed by the row kernel (reduction +
    // residual stream + the next RMSNorm), the gate/up slabs by the SwiGLU finalize: 9 launches per layer instead of 13.
    int short_splitk() const {
        int rc;
        const int sbits = wqbits ? wqbits : 16;   // split-K kernels' weight-format code
        // int8: row scales applied by the slab consumers; int4: group scales applied inside the split-K kernel
        auto sc_of = [&](const llmie_matrix &m) { return SlabScale{wqbits == 8 ? static_cast<const half_t *>(m.scale) : nullptr, nullptr, nullptr}; };
        auto gs_of = [&](const llmie_matrix &m) { return wqbits == 4 ? static_cast<const half_t *>(m.scale) : nullptr; };
        TIMED(LLMIE_OP_ATTN_NORM, llmie_rmsnorm(h, resid, dec->layers[0].attn_norm_gamma, c.rms_eps, T, H, LLMIE_F16, stream));
        for (int l = 0; l < c.num_layers; ++l) {
            const llmie_layer_weights &w = dec->layers[l];
            const PrefillLayerPlan lp = layer_plan(w);
            const bool last = l + 1 == c.num_layers;
            SplitKSlabs sk;
            TIMED(LLMIE_OP_QKV_GEMM, linear_splitk_partial(sbits, h, w.qkv.data, T, H, QKV, st, &sk, slabs, gs_of(w.qkv)));
            switch (lp.qkv) {
                case PQ_SPLITK_ROPE:
                    TIMED(LLMIE_OP_QKV_GEMM, splitk_finalize_qkv_rope(sk, sc_of(w.qkv), qkv, (const half_t *)w.qkv.bias, kv, cum, history_lengths,
                                                                      dec->rope_table, l, batch, c.head_num, c.kv_head_num, c.max_seq_len, c.rotary_dim, st));
                    break;
                case PQ_SPLITK: TIMED(LLMIE_OP_QKV_GEMM, splitk_finalize(sk, sc_of(w.qkv), qkv, EPI_NONE_, nullptr, nullptr, st)); break;
                default: return bad_form("QKV", lp.qkv);
            }
            TIMED(LLMIE_OP_MHA, attention(l, w.qkv, lp));
            TIMED(LLMIE_OP_O_GEMM, linear_splitk_partial(sbits, attn, w.o.data, T, H, H, st, &sk, slabs, gs_of(w.o)));
            // context_decoder.cpp: h += resid; resid = h; h += o.bias; h = rmsnorm(h, ffn_gamma)
            TIMED(LLMIE_OP_FFN_NORM, splitk_rownorm(sk, sc_of(w.o), static_cast<const half_t *>(w.o.bias), resid,
                                                    static_cast<const half_t *>(w.ffn_norm_gamma), c.rms_eps, h, nullptr, nullptr, st));
            TIMED(LLMIE_OP_GATE_UP_SWIGLU, linear_splitk_partial(sbits, h, w.gate_up.data, T, H, 2 * I, st, &sk, slabs, gs_of(w.gate_up)));
            TIMED(LLMIE_OP_GATE_UP_SWIGLU, splitk_finalize(sk, sc_of(w.gate_up), act, EPI_SWIGLU_, nullptr, nullptr, st));
            TIMED(LLMIE_OP_DOWN_GEMM, linear_splitk_partial(sbits, act, w.down.data, T, I, H, st, &sk, slabs, gs_of(w.down)));
            // h = act.Wd^T + resid, then the next layer's resid = h; h = rmsnorm(h) (last layer: h stays un-normalised)
            const void *next_gamma = last ? nullptr : dec->layers[l + 1].attn_norm_gamma;
            TIMED(LLMIE_OP_ATTN_NORM, splitk_rownorm(sk, sc_of(w.down), nullptr, resid, static_cast<const half_t *>(next_gamma), c.rms_eps, h,
                                                     nullptr, nullptr, st));
        }
        return LLMIE_OK;
    }
    // Round 3, fp16 / int8 / int4 weights without an output-projection bias (Llama): the residual stream S lives un-normalised in
    // `h` for the whole pass -- the O and down projections add into it in their epilogues (y = S, residual = S: every element is read
    // and written by the same lane) and the two norms are out-of-place reads of S into `resid` (used as the projections' input N):
    //   N = norm(S) g1 -> qkv -> attention -> S += attn . Wo^T -> N = norm(S) g2 -> act = swiglu(N . Wgu^T) -> S += act . Wd^T
    // Same values as the general sequence up to where fp16 roundings fall (o + resid is rounded once instead of twice); each norm
    // moves 2 x |S| bytes instead of 3-4 x (context_decoder.cpp:70-199 order).
    // (interleaved A/B on one box, fp16: 1 x 2048 78.15k -> 78.55k tok/s, 8 x 512 89.56k -> 89.87k: the norms drop 13.5 + 15.0 ->
    // 9.7 + 9.7 us per layer, the O projection's residual epilogue costs 6.3 us of that back)
    int lean() const {
        int rc;
        half_t *S = h, *Nn = resid;
        for (int l = 0; l < c.num_layers; ++l) {
            const llmie_layer_weights &w = dec->layers[l];
            const PrefillLayerPlan lp = layer_plan(w);
            TIMED(LLMIE_OP_ATTN_NORM, attn_norm(lp.attn_norm, w));
            TIMED(LLMIE_OP_QKV_GEMM, qkv_proj(l, w.qkv, Nn, lp.qkv));
            TIMED(LLMIE_OP_MHA, attention(l, w.qkv, lp));
            TIMED(LLMIE_OP_O_GEMM, proj(attn, w.o, S, H, H, S));
            TIMED(LLMIE_OP_FFN_NORM, ffn_norm(lp.ffn_norm, w));
            if ((rc = gate_up(Nn, w.gate_up, lp.gate_up))) return rc;
            TIMED(LLMIE_OP_DOWN_GEMM, proj(act, w.down, S, I, H, S));
        }
        return LLMIE_OK;
    }
    // per-request adapters: the general sequence in the forms plan_prefill_layer forces, every projection followed by its adapter update
    int lora() const {
        int rc;
        const int qkv_w[3] = {c.head_num * c.head_size, c.kv_head_num * c.head_size, c.kv_head_num * c.head_size}, gu_w[2] = {I, I};
        for (int l = 0; l < c.num_layers; ++l) {
            const llmie_layer_weights &w = dec->layers[l];
            const PrefillLayerPlan lp = layer_plan(w);
            TIMED(LLMIE_OP_ATTN_NORM, attn_norm(lp.attn_norm, w));
            TIMED(LLMIE_OP_QKV_GEMM, qkv_proj(l, w.qkv, h, lp.qkv));
            TIMED(LLMIE_OP_QKV_GEMM, engine_lora(dec, h, qkv, T, H, QKV, 3, qkv_w, l, LLMIE_LORA_QKV, stream));
            TIMED(LLMIE_OP_MHA, attention(l, w.qkv, lp));
            TIMED(LLMIE_OP_O_GEMM, proj(attn, w.o, h, H, H, nullptr));
            TIMED(LLMIE_OP_O_GEMM, engine_lora(dec, attn, h, T, H, H, 1, &H, l, LLMIE_LORA_O, stream));
            TIMED(LLMIE_OP_FFN_NORM, ffn_norm(lp.ffn_norm, w));
            if (lp.gate_up != PG_TWO_LAUNCH) return bad_form("gate/up", lp.gate_up);
            TIMED(LLMIE_OP_GATE_UP_SWIGLU, proj(h, w.gate_up, gu, H, 2 * I, nullptr));
            TIMED(LLMIE_OP_GATE_UP_SWIGLU, engine_lora(dec, h, gu, T, H, 2 * I, 2, gu_w, l, LLMIE_LORA_GATE_UP, stream));
            TIMED(LLMIE_OP_GATE_UP_SWIGLU, llmie_silu_and_mul(gu, act, T, I, LLMIE_F16, stream));
            TIMED(LLMIE_OP_DOWN_GEMM, proj(act, w.down, h, I, H, resid));
            TIMED(LLMIE_OP_DOWN_GEMM, engine_lora(dec, act, h, T, I, H, 1, &H, l, LLMIE_LORA_DOWN, stream));
        }
        return LLMIE_OK;
    }
    // experts attached: the general sequence in the forms plan_prefill_layer forces (normalised fp16 rows in place); a layer with a
    // router runs route + expert FFN where a dense layer runs its gate/up and down launches
    int moe(const MoePlan &moe_plan) const {
        int rc;
        for (int l = 0; l < c.num_layers; ++l) {
            const llmie_layer_weights &w = dec->layers[l];
            const PrefillLayerPlan lp = layer_plan(w);
            TIMED(LLMIE_OP_ATTN_NORM, attn_norm(lp.attn_norm, w));
            TIMED(LLMIE_OP_QKV_GEMM, qkv_proj(l, w.qkv, h, lp.qkv));
            TIMED(LLMIE_OP_MHA, attention(l, w.qkv, lp));
            TIMED(LLMIE_OP_O_GEMM, proj(attn, w.o, h, H, H, nullptr));
            TIMED(LLMIE_OP_FFN_NORM, ffn_norm(lp.ffn_norm, w));
            if (dec->moe.layers[l].router) {
                if ((rc = engine_moe_ffn(dec, moe_plan, l, h, resid, stream))) return rc;
            } else {
                if ((rc = gate_up(h, w.gate_up, lp.gate_up))) return rc;
                TIMED(LLMIE_OP_DOWN_GEMM, proj(act, w.down, h, I, H, resid));
            }
        }
        return LLMIE_OK;
    }
    // the general sequence (context_decoder.cpp:70-199): every format, any alignment, an output-projection bias
    int general() const {
        int rc;
        for (int l = 0; l < c.num_layers; ++l) {
            const llmie_layer_weights &w = dec->layers[l];
            const PrefillLayerPlan lp = layer_plan(w);
            TIMED(LLMIE_OP_ATTN_NORM, attn_norm(lp.attn_norm, w));
            TIMED(LLMIE_OP_QKV_GEMM, qkv_proj(l, w.qkv, h, lp.qkv));
            TIMED(LLMIE_OP_MHA, attention(l, w.qkv, lp));
            TIMED(LLMIE_OP_O_GEMM, proj(attn, w.o, h, H, H, nullptr));
            TIMED(LLMIE_OP_FFN_NORM, ffn_norm(lp.ffn_norm, w));
            if ((rc = gate_up(h, w.gate_up, lp.gate_up))) return rc;
            TIMED(LLMIE_OP_DOWN_GEMM, proj(act, w.down, h, I, H, resid));
        }
        return LLMIE_OK;
    }
};

static int prefill_shape_ok(const llmie_decoder_config &c, int batch, int num_tokens, int max_q_len) {
    LLMIE_REQUIRE(batch >= 1 && num_tokens >= 1 && max_q_len >= 1 && max_q_len <= num_tokens && max_q_len <= c.max_seq_len,
                  "decoder_prefill: bad shape batch=%d tokens=%d max_q_len=%d", batch, num_tokens, max_q_len);
    LLMIE_REQUIRE(num_tokens <= static_cast<long long>(batch) * max_q_len, "decoder_prefill: num_tokens > batch*max_q_len");
    return LLMIE_OK;
}
// both prefill entry points: validate, plan, refuse or: carve the workspace, copy hidden_in, set up what the sequences share, dispatch
static int decoder_prefill(llmie_decoder *dec, const void *hidden_in, void *hidden_out, void *k_cache, void *v_cache,
                           const int32_t *block_table, int max_pages, int num_pages, const int32_t *input_lengths,
                           const int32_t *history_lengths, int batch, int num_tokens, int max_q_len, void *workspace,
                           size_t workspace_bytes, llmie_stream stream) {
    LLMIE_REQUIRE(dec && hidden_in && hidden_out && k_cache && v_cache && input_lengths && history_lengths && workspace,
                  "decoder_prefill: NULL pointer");
    const llmie_decoder_config &c = dec->cfg;
    if (int rc = prefill_shape_ok(c, batch, num_tokens, max_q_len)) return rc;
    const int H = dec->H, QKV = dec->QKV, I = dec->I, T = num_tokens;
    const EngineSwitches &sw = engine_switches();
    PrefillCall call{c, T, true, true, mis16(hidden_out) == 0, false, sw, dec->lora.table != nullptr, dec->moe.on(), dec->q_gammas != nullptr,
                     dec->tree_anc != nullptr};
    if (call.tree) LLMIE_REQUIRE(max_q_len <= dec->tree_stride, "decoder_prefill: max_q_len %d above the stride %d of the tree that is set", max_q_len, dec->tree_stride);
    for (const llmie_layer_weights &w : dec->layers) {
        call.weights_a16 = call.weights_a16 && (mis16(w.qkv.data) | mis16(w.o.data) | mis16(w.gate_up.data) | mis16(w.down.data)) == 0;
        call.int4_scales_a4 = call.int4_scales_a4 && (reinterpret_cast<uintptr_t>(w.qkv.scale) | reinterpret_cast<uintptr_t>(w.o.scale) |
                                                      reinterpret_cast<uintptr_t>(w.gate_up.scale) | reinterpret_cast<uintptr_t>(w.down.scale)) % 4 == 0;
        call.hidden_gammas_a16 = call.hidden_gammas_a16 && (mis16(w.attn_norm_gamma) | mis16(w.ffn_norm_gamma)) == 0;
        call.o_bias = call.o_bias || w.o.bias != nullptr;
    }
    const PrefillPlan plan = plan_prefill(call);
    if (plan.path == PP_REFUSED) return prefill_refuse(plan);
    if (plan.path == PP_LORA)
        if (int rc = lora_rows_fit(dec, T, "decoder_prefill")) return rc;
    MoePlan moe_plan{};
    if (plan.path == PP_MOE)
        if (int rc = moe_rows_fit(dec, T, "decoder_prefill", &moe_plan)) return rc;
    const PrefillCarve o = prefill_carve(&c, T, batch);
    if (workspace_bytes < o.total || reinterpret_cast<uintptr_t>(workspace) % 256) {
        set_error("decoder_prefill: workspace too small or unaligned (%zu < %zu)", workspace_bytes, o.total);
        return LLMIE_ERR_WORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    if (hidden_out != hidden_in) {
        if (hipMemcpyAsync(hidden_out, hidden_in, static_cast<size_t>(T) * H * 2, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            set_error("decoder_prefill: copy failed");
            return LLMIE_ERR_LAUNCH;
        }
    }
    char *base = static_cast<char *>(workspace);
    const bool fp8 = c.wfmt == LLMIE_W_FP8;
    int32_t *pad = (int32_t *)(base + o.pad), *cum = (int32_t *)(base + o.cum);
    int32_t *tok_b = (int32_t *)(base + o.tokens + 256), *tok_tpos = tok_b + T;
    PrefillPass p{dec, c, call, plan.path, stream, st, kv_view(c, k_cache, v_cache, block_table, max_pages, num_pages), cum, history_lengths, batch, T, max_q_len,
                  H, QKV, I, fp8, c.wfmt == LLMIE_W_INT8 ? 8 : (c.wfmt == LLMIE_W_INT4 ? 4 : 0),
                  (half_t *)hidden_out, (half_t *)(base + o.resid), (half_t *)(base + o.qkv), (half_t *)(base + o.attn), (half_t *)(base + o.gu),
                  (half_t *)(base + o.act), base + o.fp8_ws, fp8 ? llmie_linear_fp8_workspace_bytes(T, I > H ? I : H, 0) : 0,
                  SlabWs{reinterpret_cast<float *>(base + o.slabs), prefill_slab_floats(&c, T)}, base + o.deq, o.tokens - o.deq,
                  (QkvRopeArgs *)(base + o.tokens)};
    int rc;
    // context_decoder.cpp:70: exclusive prefix of the lengths (padding offsets are a by-product nobody needs here);
    // the prefix kernel takes [batch, max_q_len] with max_q_len = ceil(T / batch) rows worth of scratch -> use 1 row of T
    if ((rc = llmie_cal_padding_offset(pad, cum, input_lengths, batch, (T + batch - 1) / batch, stream))) return rc;
    if (prefill_rope_fusable(call)) {   // the token table of the QKV projection's RoPE + append epilogue
        QkvRopeArgs ra{};
        ra.k_cache = p.kv.k;
        ra.v_cache = p.kv.v;
        ra.rope = dec->rope_table;
        ra.table = p.kv.block_table;
        ra.layer_stride = p.kv.block_table ? static_cast<size_t>(p.kv.num_pages) * c.kv_head_num * 128 * c.head_size
                                           : static_cast<size_t>(batch) * c.kv_head_num * c.max_seq_len * c.head_size;
        ra.head_num = c.head_num;
        ra.kv_head_num = c.kv_head_num;
        ra.max_seq_len = c.max_seq_len;
        ra.rotary_dim = c.rotary_dim;
        ra.max_pages = p.kv.max_pages;
        ra.kv8 = p.kv.fp8;
        ra.k_inv_scale = 1.0f / p.kv.k_scale;
        ra.v_inv_scale = 1.0f / p.kv.v_scale;
        if ((rc = prefill_token_table(cum, history_lengths, batch, T, tok_b, tok_tpos, ra, p.rope_args, st))) return rc;
    }
    if (plan.path == PP_LORA &&   // the slot of every token: its sequence's, expanded over the lengths on the device
        (rc = llmie_lora_plan(dec->lora.seq_slot, input_lengths, batch, T, dec->lora.table, dec->lora.slots, dec->lora.ws, dec->lora.ws_bytes, stream)))
        return rc;
    switch (plan.path) {
        case PP_LORA: return p.lora();
        case PP_MOE: return p.moe(moe_plan);
        case PP_PACKED_ONLY: return p.packed_only();
        case PP_SHORT_SPLITK: return p.short_splitk();
        case PP_LEAN: return p.lean();
        default: return p.general();
    }
}

extern "C" int llmie_decoder_prefill(llmie_decoder *dec, const void *hidden_in, void *hidden_out, void *k_cache,
                                     void *v_cache, const int32_t *input_lengths, const int32_t *history_lengths,
                                     int batch, int num_tokens, int max_q_len, void *workspace, size_t workspace_bytes,
                                     llmie_stream stream) {
    return decoder_prefill(dec, hidden_in, hidden_out, k_cache, v_cache, nullptr, 0, 0, input_lengths, history_lengths, batch, num_tokens,
                           max_q_len, workspace, workspace_bytes, stream);
}

extern "C" int llmie_decoder_prefill_paged(llmie_decoder *dec, const void *hidden_in, void *hidden_out, void *k_pool, void *v_pool,
                                           const int32_t *block_table, int max_pages, int num_pages, const int32_t *input_lengths,
                                           const int32_t *history_lengths, int batch, int num_tokens, int max_q_len,
                                           void *workspace, size_t workspace_bytes, llmie_stream stream) {
    if (int rc = paged_args_ok(dec, block_table, max_pages, num_pages, "decoder_prefill_paged")) return rc;
    return decoder_prefill(dec, hidden_in, hidden_out, k_pool, v_pool, block_table, max_pages, num_pages, input_lengths, history_lengths, batch,
                           num_tokens, max_q_len, workspace, workspace_bytes, stream);
}

extern "C" size_t llmie_decoder_lora_workspace_bytes(const llmie_decoder_config *cfg, int max_tokens, int slots) {
    if (!config_ok(cfg) || max_tokens <= 0) return 0;
    return llmie_lora_workspace_bytes(max_tokens > cfg->max_batch ? max_tokens : cfg->max_batch, slots, 192);
}

extern "C" int llmie_decoder_lora_attach(llmie_decoder *dec, const void *table_dev, int slots, const int32_t *seq_slot_dev, void *workspace,
                                         size_t workspace_bytes) {
    LLMIE_REQUIRE(dec && table_dev && seq_slot_dev && workspace, "decoder_lora_attach: NULL pointer");
    LLMIE_REQUIRE(slots > 0, "decoder_lora_attach: %d slots", slots);
    if (slots > LLMIE_LORA_MAX_SLOTS) LLMIE_UNSUPPORTED("decoder_lora_attach: %d slots above LLMIE_LORA_MAX_SLOTS (%d)", slots, LLMIE_LORA_MAX_SLOTS);
    if (!lora_engine_ok(dec->cfg)) LLMIE_UNSUPPORTED("decoder_lora_attach: %s", kLoraRefusal);
    if (dec->moe.on()) LLMIE_UNSUPPORTED("decoder_lora_attach: %s", kMoeLoraRefusal);
    const size_t need = llmie_lora_workspace_bytes(dec->cfg.max_batch, slots, 192);
    if (workspace_bytes < need || reinterpret_cast<uintptr_t>(workspace) % 256) {
        set_error("decoder_lora_attach: workspace too small or not 256-byte aligned (%zu < %zu)", workspace_bytes, need);
        return LLMIE_ERR_WORKSPACE;
    }
    dec->lora.table = table_dev, dec->lora.slots = slots, dec->lora.seq_slot = seq_slot_dev, dec->lora.ws = workspace, dec->lora.ws_bytes = workspace_bytes;
    return LLMIE_OK;
}

extern "C" size_t llmie_decoder_moe_workspace_bytes(const llmie_decoder_config *cfg, int max_tokens, int inter, int experts, int top_k) {
    if (!config_ok(cfg) || max_tokens <= 0) return 0;
    return llmie_moe_workspace_bytes(max_tokens > cfg->max_batch ? max_tokens : cfg->max_batch, cfg->head_num * cfg->head_size, inter, experts, top_k);
}

// both attach entries: the descriptors of every layer are already checked pointer by pointer
static int moe_attach_common(llmie_decoder *dec, const char *who, std::vector<llmie_moe_experts> &&layers, const MoeCall &call, void *workspace,
                             size_t workspace_bytes) {
    const size_t need = llmie_moe_workspace_bytes(dec->cfg.max_batch, call.H, call.Ie, call.E, call.k);
    if (workspace_bytes < need || reinterpret_cast<uintptr_t>(workspace) % 256) {
        set_error("%s: workspace too small or not 256-byte aligned (%zu < %zu)", who, workspace_bytes, need);
        return LLMIE_ERR_WORKSPACE;
    }
    dec->moe.layers = std::move(layers);
    dec->moe.call = call;
    dec->moe.ws = workspace, dec->moe.ws_bytes = workspace_bytes;
    return LLMIE_OK;
}

extern "C" int llmie_decoder_moe_attach(llmie_decoder *dec, const llmie_moe_layer *layers, int inter, int experts, int top_k, unsigned flags,
                                        void *workspace, size_t workspace_bytes) {
    LLMIE_REQUIRE(dec && layers && workspace, "decoder_moe_attach: NULL pointer");
    LLMIE_REQUIRE(inter > 0 && experts > 0 && top_k > 0, "decoder_moe_attach: non-positive size inter=%d experts=%d top_k=%d", inter, experts, top_k);
    if (!moe_engine_ok(dec->cfg)) LLMIE_UNSUPPORTED("decoder_moe_attach: %s", kMoeRefusal);
    if (dec->lora.table) LLMIE_UNSUPPORTED("decoder_moe_attach: %s", kMoeLoraRefusal);
    // the operator's own checks of the expert geometry and flags, at one row (a flag with a row limit is checked per call)
    const MoeCall call{1, dec->H, inter, experts, top_k, flags, LLMIE_W_F16, false};
    if (int rc = moe_call_check("decoder_moe_attach", call)) return rc;
    bool any = false;
    std::vector<llmie_moe_experts> ex(dec->cfg.num_layers, llmie_moe_experts{});
    for (int l = 0; l < dec->cfg.num_layers; ++l) {
        const llmie_moe_layer &m = layers[l];
        LLMIE_REQUIRE(!m.router || (m.gate_up && m.down), "decoder_moe_attach: layer %d has a router without its expert matrices", l);
        if (mis16(m.router) || mis16(m.gate_up) || mis16(m.down)) LLMIE_UNSUPPORTED("decoder_moe_attach: layer %d: router / gate_up / down not 16-byte aligned", l);
        any |= m.router != nullptr;
        ex[l].format = LLMIE_W_F16, ex[l].router = m.router, ex[l].gate_up = m.gate_up, ex[l].down = m.down, ex[l].act = LLMIE_MOE_ACT_SWIGLU;
    }
    LLMIE_REQUIRE(any, "decoder_moe_attach: no layer has a router");
    return moe_attach_common(dec, "decoder_moe_attach", std::move(ex), call, workspace, workspace_bytes);
}

extern "C" int llmie_decoder_moe_attach_ex(llmie_decoder *dec, const llmie_moe_experts *layers, int inter, int experts, int top_k, unsigned flags,
                                           void *workspace, size_t workspace_bytes) {
    LLMIE_REQUIRE(dec && layers && workspace, "decoder_moe_attach_ex: NULL pointer");
    LLMIE_REQUIRE(inter > 0 && experts > 0 && top_k > 0, "decoder_moe_attach_ex: non-positive size inter=%d experts=%d top_k=%d", inter, experts, top_k);
    if (!moe_engine_ok(dec->cfg)) LLMIE_UNSUPPORTED("decoder_moe_attach_ex: %s", kMoeRefusal);
    if (dec->lora.table) LLMIE_UNSUPPORTED("decoder_moe_attach_ex: %s", kMoeLoraRefusal);
    const llmie_moe_experts *first = nullptr;
    for (int l = 0; l < dec->cfg.num_layers; ++l) {
        const llmie_moe_experts &m = layers[l];
        if (!m.router) continue;   // the layer keeps its dense FFN
        if (int rc = moe_experts_ok("decoder_moe_attach_ex", &m)) return rc;
        if (!first) first = &m;
        if (m.format != first->format || m.act != first->act)
            LLMIE_UNSUPPORTED("decoder_moe_attach_ex: layer %d differs from the first sparse layer in expert format or act", l);
    }
    LLMIE_REQUIRE(first, "decoder_moe_attach_ex: no layer has a router");
    const MoeCall call{1, dec->H, inter, experts, top_k, flags, first->format, moe_epilogue_live(*first)};
    if (int rc = moe_call_check("decoder_moe_attach_ex", call)) return rc;
    return moe_attach_common(dec, "decoder_moe_attach_ex", std::vector<llmie_moe_experts>(layers, layers + dec->cfg.num_layers), call, workspace,
                             workspace_bytes);
}

extern "C" int llmie_decoder_moe_detach(llmie_decoder *dec) {
    LLMIE_REQUIRE(dec, "decoder_moe_detach: NULL decoder");
    dec->moe = llmie_decoder::Moe{};
    return LLMIE_OK;
}

// Sliding-window attention: state on the engine, read where a call's attention launches are planned (the lora_attach pattern)
extern "C" int llmie_decoder_set_window(llmie_decoder *dec, const int32_t *layer_window, int sinks) {
    LLMIE_REQUIRE(dec, "decoder_set_window: NULL decoder");
    if (!layer_window) {   // back to full attention on every layer
        LLMIE_REQUIRE(sinks == 0, "decoder_set_window: %d sink tokens without a window", sinks);
        dec->layer_window.clear(), dec->sinks = 0;
        return LLMIE_OK;
    }
    LLMIE_REQUIRE(sinks >= 0, "decoder_set_window: sinks %d must not be negative", sinks);
    bool any = false;
    for (int l = 0; l < dec->cfg.num_layers; ++l) {
        LLMIE_REQUIRE(layer_window[l] >= 0, "decoder_set_window: window %d of layer %d must not be negative", layer_window[l], l);
        any |= layer_window[l] > 0;
    }
    LLMIE_REQUIRE(any || sinks == 0, "decoder_set_window: %d sink tokens without a window on any layer", sinks);
    if (any && !window_engine_ok(dec->cfg)) LLMIE_UNSUPPORTED("decoder_set_window: %s", kWindowRefusal);
    if (any && dec->q_gammas) LLMIE_UNSUPPORTED("decoder_set_window: %s", kQkNormRefusal);
    if (any && dec->tree_anc) LLMIE_UNSUPPORTED("decoder_set_window: %s", kTreeRefusal);
    if (any) dec->layer_window.assign(layer_window, layer_window + dec->cfg.num_layers), dec->sinks = sinks;
    else dec->layer_window.clear(), dec->sinks = 0;
    return LLMIE_OK;
}

// Learned per-head sink logits: the caller's device array, kept on the engine and read where a call's attention launches are planned
extern "C" int llmie_decoder_set_head_sinks(llmie_decoder *dec, const float *head_sink_dev) {
    LLMIE_REQUIRE(dec, "decoder_set_head_sinks: NULL decoder");
    if (head_sink_dev && !window_engine_ok(dec->cfg)) LLMIE_UNSUPPORTED("decoder_set_head_sinks: %s", kHeadSinkRefusal);
    if (head_sink_dev && dec->q_gammas) LLMIE_UNSUPPORTED("decoder_set_head_sinks: %s", kQkNormRefusal);
    if (head_sink_dev && dec->tree_anc) LLMIE_UNSUPPORTED("decoder_set_head_sinks: %s", kTreeRefusal);
    LLMIE_REQUIRE(reinterpret_cast<uintptr_t>(head_sink_dev) % sizeof(float) == 0, "decoder_set_head_sinks: the array must be 4-byte aligned");
    dec->head_sinks = head_sink_dev;
    return LLMIE_OK;
}

// QK-norm: the caller's device arrays and eps, kept on the engine and read where a call's attention launches are built
extern "C" int llmie_decoder_set_qk_norm(llmie_decoder *dec, const void *q_gamma_dev, const void *k_gamma_dev, float eps) {
    LLMIE_REQUIRE(dec, "decoder_set_qk_norm: NULL decoder");
    LLMIE_REQUIRE((q_gamma_dev != nullptr) == (k_gamma_dev != nullptr), "decoder_set_qk_norm: q_gamma and k_gamma go together (one is NULL)");
    if (!q_gamma_dev) {   // back to un-normalised q and k
        dec->q_gammas = dec->k_gammas = nullptr, dec->qk_eps = 0.f;
        return LLMIE_OK;
    }
    LLMIE_REQUIRE((mis16(q_gamma_dev) | mis16(k_gamma_dev)) == 0, "decoder_set_qk_norm: the gamma arrays must be 16-byte aligned");
    LLMIE_REQUIRE(eps >= 0.f, "decoder_set_qk_norm: eps must be a number >= 0");
    bool bias = false;
    for (const llmie_layer_weights &w : dec->layers) bias |= w.qkv.bias != nullptr;
    if (!qk_norm_engine_ok(dec->cfg) || bias || !dec->layer_window.empty() || dec->head_sinks)
        LLMIE_UNSUPPORTED("decoder_set_qk_norm: %s", kQkNormRefusal);
    dec->q_gammas = static_cast<const half_t *>(q_gamma_dev), dec->k_gammas = static_cast<const half_t *>(k_gamma_dev), dec->qk_eps = eps;
    return LLMIE_OK;
}

// Draft tree: the caller's device arrays, kept on the engine and read by every prefill launch built while they are set
extern "C" int llmie_decoder_set_tree(llmie_decoder *dec, const int32_t *depth_dev, const uint64_t *anc_dev, int stride) {
    LLMIE_REQUIRE(dec, "decoder_set_tree: NULL decoder");
    LLMIE_REQUIRE((depth_dev != nullptr) == (anc_dev != nullptr), "decoder_set_tree: depth and anc go together (one is NULL)");
    if (!depth_dev) {   // back to a causal chunk
        LLMIE_REQUIRE(stride == 0, "decoder_set_tree: stride %d without a tree", stride);
        dec->tree_depth = nullptr, dec->tree_anc = nullptr, dec->tree_stride = 0;
        return LLMIE_OK;
    }
    LLMIE_REQUIRE(stride >= 1 && stride <= LLMIE_SPEC_TREE_MAX_NODES, "decoder_set_tree: stride %d outside [1,%d]", stride, LLMIE_SPEC_TREE_MAX_NODES);
    LLMIE_REQUIRE(reinterpret_cast<uintptr_t>(depth_dev) % 4 == 0 && reinterpret_cast<uintptr_t>(anc_dev) % 8 == 0,
                  "decoder_set_tree: depth must be 4-byte and anc 8-byte aligned");
    const PrefillCall probe{dec->cfg, 1, true, true, true, false, engine_switches(), false, false, false, true};
    if (plan_prefill(probe).path == PP_REFUSED || !dec->layer_window.empty() || dec->head_sinks) LLMIE_UNSUPPORTED("decoder_set_tree: %s", kTreeRefusal);
    dec->tree_depth = depth_dev, dec->tree_anc = anc_dev, dec->tree_stride = stride;
    return LLMIE_OK;
}

// RoPE frequency scaling: refill the table on the host, one synchronous upload (not inside a capture)
extern "C" int llmie_decoder_set_rope_scaling(llmie_decoder *dec, const llmie_rope_scaling *scaling) {
    LLMIE_REQUIRE(dec, "decoder_set_rope_scaling: NULL decoder");
    if (!fused_attention_geometry(dec->cfg))
        LLMIE_UNSUPPORTED("decoder_set_rope_scaling: this engine's decode attention rotates by rotary_base, not by the table (needs head_size in "
                          "{32,64,128,256} and head_num/kv_head_num in {1,2,4,8})");
    return rope_table_upload(dec, scaling, "decoder_set_rope_scaling");
}

extern "C" int llmie_decoder_lora_detach(llmie_decoder *dec) {
    LLMIE_REQUIRE(dec, "decoder_lora_detach: NULL decoder");
    dec->lora = llmie_decoder::Lora{};
    return LLMIE_OK;
}

// Host-only: what one layer of llmie_decoder_prefill launches (include/llmie.h) -- the pass's plan_prefill, plan_prefill_layer for a
// layer whose operands follow the call flags, and its plan_prefill_attn, as text
extern "C" const char *llmie_decoder_prefill_layer_plan(const llmie_decoder_config *cfg, int tokens, int batch, int max_q_len, unsigned call_flags,
                                                        unsigned switch_mask, int *status) {
    static thread_local char text[384];
    const int rc = [&]() -> int {
        LLMIE_REQUIRE(config_ok(cfg), "decoder_prefill_layer_plan: invalid config");
        if ((cfg->flags & LLMIE_DEC_PACKED_ONLY) && !packed_wf(cfg))
            LLMIE_UNSUPPORTED("%s", packed_only_refusal(cfg));
        if (int bad = prefill_shape_ok(*cfg, batch, tokens, max_q_len)) return bad;
        if ((call_flags & LLMIE_PLAN_WINDOW) && !window_engine_ok(*cfg)) LLMIE_UNSUPPORTED("decoder_prefill_layer_plan: %s", kWindowRefusal);
        if ((call_flags & LLMIE_PLAN_HEAD_SINK) && !window_engine_ok(*cfg)) LLMIE_UNSUPPORTED("decoder_prefill_layer_plan: %s", kHeadSinkRefusal);
        if ((call_flags & LLMIE_PLAN_QK_NORM) && (!qk_norm_engine_ok(*cfg) || (call_flags & (LLMIE_PLAN_WINDOW | LLMIE_PLAN_HEAD_SINK))))
            LLMIE_UNSUPPORTED("decoder_prefill_layer_plan: %s", kQkNormRefusal);
        if ((call_flags & LLMIE_PLAN_TREE) && (call_flags & (LLMIE_PLAN_WINDOW | LLMIE_PLAN_HEAD_SINK)))
            LLMIE_UNSUPPORTED("decoder_prefill_layer_plan: %s", kTreeRefusal);
        if (call_flags & LLMIE_PLAN_TREE)
            LLMIE_REQUIRE(max_q_len <= LLMIE_SPEC_TREE_MAX_NODES, "decoder_prefill_layer_plan: max_q_len %d above the %d nodes of a tree", max_q_len, LLMIE_SPEC_TREE_MAX_NODES);
        const PrefillCall call = prefill_call_of_flags(*cfg, tokens, call_flags, switches_of_mask(switch_mask));
        const PrefillPlan plan = plan_prefill(call);
        if (plan.path == PP_REFUSED) return prefill_refuse(plan);
        const PrefillCarve o = prefill_carve(cfg, tokens, batch);
        const bool scales = cfg->wfmt != LLMIE_W_F16;   // (fp16 engines have none: a null pointer)
        const unsigned mis_w = (call_flags & LLMIE_PLAN_WEIGHTS_MISALIGNED) ? 8u : 0u, mis_s = scales && (call_flags & LLMIE_PLAN_SCALES_MISALIGNED) ? 2u : 0u;
        const PrefillLayerPlan lp = plan_prefill_layer(
            call, plan.path, batch, max_q_len,
            PrefillLayerCall{mis_w, mis_s, (call_flags & LLMIE_PLAN_QKV_BIAS_MISALIGNED) ? 4u : 0u, mis_w,
                             mis_s + (scales && (call_flags & LLMIE_PLAN_GATE_UP_SCALES_MISALIGNED) ? 8u : 0u),
                             (call_flags & LLMIE_PLAN_HIDDEN_MISALIGNED) ? 8u : 0u, !(call_flags & LLMIE_PLAN_NO_FFN_GAMMA), prefill_slab_floats(cfg, tokens),
                             o.tokens - o.deq});
        static const char *const norms[] = {"none", "inplace", "oop", "quant", "rownorm"};
        static const char *const qkvs[] = {"plain", "rope_f16", "rope_w8", "rope_image", "plain_e4m3", "rope_e4m3", "unpack_plain", "rope_unpacked", "splitk", "splitk_rope"};
        static const char *const gus[] = {"fused", "two_launch", "e4m3_swiglu", "fp8_swiglu", "unpack_fused", "unpack_two_launch", "splitk"};
        static const char *const ops[] = {"attn_norm", "qkv_gemm", "rope", "mha", "o_gemm", "ffn_norm", "gate_up_swiglu", "down_gemm"};
        const char *pre = lp.qkv == PQ_ROPE_IMAGE ? "dequant" : (lp.qkv == PQ_UNPACK_PLAIN || lp.qkv == PQ_ROPE_UNPACKED ? "unpack" : "none");
        const PrefillAttnPlan &a = lp.attn;
        int n = snprintf(text, sizeof(text), "%s token_table=%d attn_norm=%s qkv=%s pre=%s rope_done=%d attn=q%dw%dt%d kv=%s grid=%dx%dx%d rope_append=%d "
                         "ffn_norm=%s gate_up=%s launches", prefill_path_name(plan.path), prefill_rope_fusable(call) ? 1 : 0, norms[lp.attn_norm], qkvs[lp.qkv],
                         pre, lp.rope_done ? 1 : 0, a.q_rows, a.waves, a.row_tiles, a.kv_e4m3 ? "e4m3" : "f16", a.grid[0], a.grid[1], a.grid[2],
                         a.rope_append ? 1 : 0, norms[lp.ffn_norm], gus[lp.gate_up]);
        for (int op = 0; op <= LLMIE_OP_DOWN_GEMM; ++op)
            if (lp.launches[op]) n += snprintf(text + n, sizeof(text) - n, " %s=%d", ops[op], lp.launches[op]);
        // (a windowed layer runs the windowed instantiation of the same flash form on the same grid)
        if (call_flags & LLMIE_PLAN_WINDOW) n += snprintf(text + n, sizeof(text) - n, " attn_window=1");
        // (... and head sinks the SINK instantiation of that form)
        if (call_flags & LLMIE_PLAN_HEAD_SINK) n += snprintf(text + n, sizeof(text) - n, " attn_head_sink=1");
        // (QK-norm: the QKN instantiation of the RoPE + append launch; the QKV forms above are already the ones without the epilogue)
        if (call_flags & LLMIE_PLAN_QK_NORM) n += snprintf(text + n, sizeof(text) - n, " qk_norm=1");
        // (a draft tree: the TREE instantiations of the RoPE + append launch and of the 64-row flash form)
        if (lp.attn.tree) snprintf(text + n, sizeof(text) - n, " tree");
        return LLMIE_OK;
    }();
    if (status) *status = rc;
    return rc == LLMIE_OK ? text : nullptr;
}

// One LM-head call: what every entry brings.  Final RMSNorm and the LM-head projection into `logits` are common (lm_head_logits);
// behind them each entry runs its own tail on the logits, with the operands only that tail uses: top-k + sampling (the reference's
// two launches), top-k round 1 + the fused decode tail, or the per-request sampler (+ its extension).
struct LmHeadCall {
    llmie_decoder *dec;
    void *hidden;
    const void *gamma;
    const llmie_matrix *head;
    llmie_weight_format fmt;
    void *logits;
    int batch;
    SamplePos pos;
    int end_id;
    llmie_stream stream;
    SampleState state;   // (the top-k tails move seq_len and finished alone)
    SampleOut out;
    const void *embed;   // the optional tail: next_hidden[b] = embed[out_id[b]], *step_dev += 1
    void *next_hidden;
    int advance;
};

// the checks every entry shares, then the logits.  tail_operands: the entry's own tail has what it needs
static int lm_head_logits(const LmHeadCall &call, bool tail_operands) {
    llmie_decoder *dec = call.dec;
    llmie_stream stream = call.stream;
    LLMIE_REQUIRE(dec && call.hidden && call.gamma && call.head && call.head->data && call.logits && tail_operands && call.state.seq_len &&
                      call.state.finished && call.out.out_id, "lm_head_sample: NULL pointer");
    const llmie_decoder_config &c = dec->cfg;
    const int batch = call.batch;
    LLMIE_REQUIRE(batch >= 1 && batch <= c.max_batch, "lm_head_sample: batch %d outside [1,%d]", batch, c.max_batch);
    LLMIE_REQUIRE(c.vocab_size > 0, "lm_head_sample: vocab_size not set in the decoder config");
    if (call.fmt == LLMIE_W_MXFP4) LLMIE_UNSUPPORTED("lm_head_sample: an MXFP4 LM head is not supported (fp16 / int8 / int4 / fp8 heads; a follow-up)");
    int rc;
    if (call.fmt == LLMIE_W_F16 && c.dtype == LLMIE_F16 && gemv_f16_eligible(batch, dec->H, call.hidden, call.head->data) &&
        !engine_switches().no_fused_decode) {
        // final RMSNorm fused into the LM-head GEMV prologue (hidden itself is left un-normalised)
        LinearOperands o = proj_operands(c, call.hidden, *call.head, call.logits, batch, dec->H, c.vocab_size, EPI_NONE_, nullptr, call.gamma);
        o.bias = call.head->bias;
        TIMED(LLMIE_OP_LM_HEAD, linear_f16_nk(o, LinearScratch{}, as_stream(stream)));
    } else {
        // llama.cpp:247  final RMSNorm (the residual copy is unused there: pass NULL)
        TIMED(LLMIE_OP_FINAL_NORM, llmie_rmsnorm(call.hidden, nullptr, call.gamma, c.rms_eps, batch, dec->H, c.dtype, stream));
        // llama.cpp:282  logits = hidden . lm_head^T
        TIMED(LLMIE_OP_LM_HEAD, engine_linear(dec, call.fmt, proj_operands(c, call.hidden, *call.head, call.logits, batch, dec->H, c.vocab_size,
                                                                           EPI_NONE_, nullptr), stream));
    }
    return LLMIE_OK;
}
// the sampler family's view of the call behind lm_head_logits (the decoder is there)
static SampleRows lm_head_rows(const LmHeadCall &call, const llmie_sampling_params *params) {
    return SampleRows{call.logits, call.batch, call.dec->cfg.vocab_size, call.dec->cfg.dtype, params, call.end_id};
}
static SampleTail lm_head_tail(const LmHeadCall &call) {
    return SampleTail{call.embed, call.next_hidden, call.dec->H, call.advance, call.dec->tail_ticket};
}

extern "C" int llmie_lm_head_sample(llmie_decoder *dec, void *hidden, const void *final_norm_gamma,
                                    const llmie_matrix *lm_head, llmie_weight_format lm_fmt, void *logits,
                                    int32_t *tmp_ids, void *tmp_vals, int32_t *topk_ids, void *topk_vals, int K,
                                    int blocks_per_row, int32_t *seq_len, uint8_t *finished, int32_t *out_ids,
                                    int batch, int step, const int32_t *step_dev, int end_id, llmie_stream stream) {
    LmHeadCall call{dec, hidden, final_norm_gamma, lm_head, lm_fmt, logits, batch, SamplePos{step, step_dev}, end_id, stream};
    call.state.seq_len = seq_len, call.state.finished = finished, call.out.out_id = out_ids;
    int rc = lm_head_logits(call, topk_ids && topk_vals);
    if (rc != LLMIE_OK) return rc;
    const int V = dec->cfg.vocab_size;
    // llama.cpp:293,304
    TIMED(LLMIE_OP_TOPK, llmie_topk(logits, tmp_ids, tmp_vals, topk_ids, topk_vals, batch, V, K, blocks_per_row, dec->cfg.dtype, stream));
    TIMED(LLMIE_OP_SAMPLING, llmie_sampling(topk_ids, topk_vals, seq_len, finished, out_ids, batch, K, step, step_dev, end_id, V, dec->cfg.dtype,
                                            stream));
    return LLMIE_OK;
}

extern "C" int llmie_lm_head_sample_next(llmie_decoder *dec, void *hidden, const void *final_norm_gamma, const llmie_matrix *lm_head,
                                         llmie_weight_format lm_fmt, void *logits, int32_t *tmp_ids, void *tmp_vals, int32_t *topk_ids,
                                         void *topk_vals, int K, int blocks_per_row, int32_t *seq_len, uint8_t *finished, int32_t *out_ids,
                                         int batch, int step, int32_t *step_dev, int end_id, const void *embed_table, void *next_hidden,
                                         int advance_step, llmie_stream stream) {
    LLMIE_REQUIRE(!next_hidden || embed_table, "lm_head_sample_next: next_hidden without an embedding table");
    LLMIE_REQUIRE(!advance_step || step_dev, "lm_head_sample_next: advance_step needs the device-resident step");
    LLMIE_REQUIRE(tmp_ids && tmp_vals, "lm_head_sample_next: tmp buffers required");
    LmHeadCall call{dec, hidden, final_norm_gamma, lm_head, lm_fmt, logits, batch, SamplePos{step, step_dev}, end_id, stream};
    call.state.seq_len = seq_len, call.state.finished = finished, call.out.out_id = out_ids;
    call.embed = embed_table, call.next_hidden = next_hidden, call.advance = advance_step;
    int rc = lm_head_logits(call, topk_ids && topk_vals);
    if (rc != LLMIE_OK) return rc;
    // llama.cpp:293-318 (+ :219 of the next token): round 1 of the top-k, then ONE launch for round 2, the sampling, the next
    // step's input embedding and the step counter
    LLMIE_REQUIRE(K >= 1 && K <= 32 && K <= dec->cfg.vocab_size && blocks_per_row >= 1 && blocks_per_row <= 64,
                  "lm_head_sample_next: K=%d / blocks_per_row=%d outside [1, 32] / [1, 64], or tmp buffers missing", K, blocks_per_row);
    const TopkOperands tk{tmp_ids, tmp_vals, topk_ids, topk_vals, K, blocks_per_row};
    TIMED(LLMIE_OP_TOPK, topk_round1_only(logits, tk, batch, dec->cfg.vocab_size, dec->cfg.dtype, as_stream(stream)));
    TIMED(LLMIE_OP_SAMPLING, decode_tail(tk, lm_head_rows(call, nullptr), call.state, call.pos, out_ids, lm_head_tail(call), as_stream(stream)));
    return LLMIE_OK;
}

extern "C" int llmie_lm_head_sample_ext(llmie_decoder *dec, void *hidden, const void *final_norm_gamma, const llmie_matrix *lm_head,
                                        llmie_weight_format lm_fmt, void *logits, const llmie_sampling_params *params_dev,
                                        int32_t *history, int history_stride, int32_t *history_len, int history_append, int32_t *seq_len,
                                        uint8_t *finished, int32_t *out_ids, float *out_logprob, int batch, int step, int32_t *step_dev,
                                        int end_id, const void *embed_table, void *next_hidden, int advance_step, void *workspace,
                                        size_t workspace_bytes, llmie_stream stream, const llmie_sampling_ext *ext) {
    LLMIE_REQUIRE(dec, "lm_head_sample_params: NULL decoder");
    LLMIE_REQUIRE(!next_hidden || embed_table, "lm_head_sample_params: next_hidden without an embedding table");
    LLMIE_REQUIRE(!advance_step || step_dev, "lm_head_sample_params: advance_step needs the device-resident step");
    LLMIE_REQUIRE(batch >= 1 && batch <= dec->cfg.max_batch, "lm_head_sample_params: batch %d outside [1,%d]", batch, dec->cfg.max_batch);
    LLMIE_REQUIRE(dec->cfg.vocab_size > 0, "lm_head_sample_params: vocab_size not set in the decoder config");
    LmHeadCall call{dec, hidden, final_norm_gamma, lm_head, lm_fmt, logits, batch, SamplePos{step, step_dev}, end_id, stream};
    call.state = SampleState{history, history_stride, history_len, history_append, seq_len, finished};
    call.out = SampleOut{out_ids, out_logprob};
    call.embed = embed_table, call.next_hidden = next_hidden, call.advance = advance_step;
    const SampleRows rows = lm_head_rows(call, params_dev);
    const SampleWs ws{workspace, workspace_bytes};
    int rc = sample_logits_check("sample_logits", rows, call.state, out_ids);
    if (rc != LLMIE_OK) return rc;
    if ((rc = sample_workspace_check("sample_logits", ws, llmie_sample_logits_workspace_bytes(batch, rows.vocab), nullptr)) != LLMIE_OK) return rc;
    bool active;
    if ((rc = sample_ext_check(batch, rows.vocab, ext, &active)) != LLMIE_OK) return rc;
    if ((rc = lm_head_logits(call, true)) != LLMIE_OK) return rc;
    // per-request controls: ONE launch (sampling_params.hip), with the next step's embedding and counter in it
    TIMED(LLMIE_OP_SAMPLING, sample_logits_launch(rows, call.state, call.pos, call.out, lm_head_tail(call), ws, active ? ext : nullptr,
                                                  as_stream(stream)));
    return LLMIE_OK;
}

// (no extension: nothing for sample_ext_check to refuse, and the kernel without it)
extern "C" int llmie_lm_head_sample_params(llmie_decoder *dec, void *hidden, const void *final_norm_gamma, const llmie_matrix *lm_head,
                                           llmie_weight_format lm_fmt, void *logits, const llmie_sampling_params *params_dev,
                                           int32_t *history, int history_stride, int32_t *history_len, int history_append,
                                           int32_t *seq_len, uint8_t *finished, int32_t *out_ids, float *out_logprob, int batch, int step,
                                           int32_t *step_dev, int end_id, const void *embed_table, void *next_hidden, int advance_step,
                                           void *workspace, size_t workspace_bytes, llmie_stream stream) {
    return llmie_lm_head_sample_ext(dec, hidden, final_norm_gamma, lm_head, lm_fmt, logits, params_dev, history, history_stride, history_len,
                                    history_append, seq_len, finished, out_ids, out_logprob, batch, step, step_dev, end_id, embed_table,
                                    next_hidden, advance_step, workspace, workspace_bytes, stream, nullptr);
}
