// llmie_score_tokens: log-probability of a given token at every row -- RMSNorm, LM head and log-softmax with the logits kept in the
// fp32 MFMA accumulators and reduced where they are.  A [rows, vocab] logits matrix is never written (131 MB of fp16 at 2048 x 32000)
// and never rounded to fp16, which is what costs the composed rmsnorm + linear + log_softmax route 1e-4 .. 7e-4 of each log-probability.
//
//   score_tile_kernel   one workgroup per (row tile of 128, span of column tiles): the 128 x 128 x 64 MFMA tile loop of
//                       tiled_mfma_f16_kernel (gemm_kernels.cuh); instead of storing a tile, every lane folds its 16 logits of each of its
//                       4 rows into running (max, sum of exp(z - max), target logit, best value, best id).  At the end of the span the 8
//                       lane states of a row (2 column waves x 4 lane groups) are merged in a fixed order into one partial per (row, span).
//   score_merge_kernel  one thread per row: the spans' partials in span order -> logprob, lse, argmax, argmax logprob.
//
// Determinism and row independence: which columns a lane state, a span and a merge step cover depends on the vocabulary size alone
// (score_spans below never looks at `rows`), every merge runs in a fixed order without atomics, and an MFMA output element depends on
// its own row and column only -- so a row's bits are the same whatever the row count and wherever the row sits.
#include "device_utils.cuh"
#include "llmie_internal.h"

#include <cfloat>
#include <climits>

namespace llmie {

namespace {

constexpr int kScoreBM = 128, kScoreBN = 128, kScoreBK = 64;
constexpr int kScoreMaxSpans = 32;
constexpr int kScorePartFloats = 8;   // (max, sum, target logit, best value, best id, pad x 3): 32 bytes, written as two 16-byte stores

// column tiles per span and number of spans for a vocabulary: at most kScoreMaxSpans spans, never more than there are column tiles.
// 2048 rows x 32000: 16 row tiles x 32 spans of 8 tiles = 512 workgroups, two per CU (what 240 VGPRs per lane let be resident).
struct ScoreSpans {
    int col_tiles, tiles_per_span, spans;
};
ScoreSpans score_spans(int vocab) {
    ScoreSpans s;
    s.col_tiles = (vocab + kScoreBN - 1) / kScoreBN;
    s.tiles_per_span = (s.col_tiles + kScoreMaxSpans - 1) / kScoreMaxSpans;
    s.spans = (s.col_tiles + s.tiles_per_span - 1) / s.tiles_per_span;
    return s;
}
size_t score_x_bytes(int rows, int hidden) { return static_cast<size_t>(rows) * hidden * sizeof(half_t); }   // H % 64 == 0: a multiple of 128

// (value, id) order of llmie_topk: larger value first, equal values -> lower id
__device__ __forceinline__ bool score_better(float v, int id, float bv, int bid) { return v > bv || (v == bv && id < bid); }

__global__ __launch_bounds__(256) void score_tile_kernel(const half_t *__restrict__ X, const half_t *__restrict__ W,
                                                         const half_t *__restrict__ bias, const int32_t *__restrict__ targets,
                                                         float *__restrict__ part, int rows, int V, int K, int tiles_per_span, int spans) {
    constexpr int BM = kScoreBM, BN = kScoreBN, BK = kScoreBK;
    // A and B k-tiles (2 x 16 KiB); after the span's last tile the same bytes hold the lane states (128 rows x 8 slots x 5 words = 20 KiB)
    __shared__ __attribute__((aligned(16))) half_t smem[(BM + BN) * BK];
    half_t *As = smem, *Bs = smem + BM * BK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;   // 2 x 2 waves, 64 x 64 each
    const int r = lane & 15, q = lane >> 4;
    const int span = blockIdx.x, m0 = blockIdx.y * BM;
    const int col_tiles = (V + BN - 1) / BN;
    const int ct_begin = span * tiles_per_span, ct_end = min(ct_begin + tiles_per_span, col_tiles);

    // running state of the lane's own columns of its 4 rows (m = m0 + wm*64 + i*16 + r)
    float run_max[4], run_sum[4], tgt_z[4], best_v[4];
    int best_id[4], tgt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        run_max[i] = -FLT_MAX;   // finite: exp(run_max - new_max) is 0, never exp(-inf + inf)
        run_sum[i] = 0.f;
        tgt_z[i] = 0.f;
        best_v[i] = -INFINITY;
        best_id[i] = INT_MAX;
        const int m = m0 + wm * 64 + i * 16 + r;
        tgt[i] = m < rows ? targets[m] : -1;
    }

    for (int ct = ct_begin; ct < ct_end; ++ct) {
        const int n0 = ct * BN;
        half8_t ra[4], rb[4];
        auto gload = [&](int k0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int id = tid + 256 * i, row = id >> 3, ch = id & 7;
                const int am = min(m0 + row, rows - 1), bn = min(n0 + row, V - 1);   // clamped: edge rows / columns never counted
                ra[i] = *reinterpret_cast<const half8_t *>(X + static_cast<size_t>(am) * K + k0 + ch * 8);
                rb[i] = *reinterpret_cast<const half8_t *>(W + static_cast<size_t>(bn) * K + k0 + ch * 8);
            }
        };
        auto lstore = [&]() {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int id = tid + 256 * i, row = id >> 3, ch = id & 7;
                const int off = row * BK + ((ch ^ (row & 7)) << 3);
                *reinterpret_cast<half8_t *>(As + off) = ra[i];
                *reinterpret_cast<half8_t *>(Bs + off) = rb[i];
            }
        };
        floatx4 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

        gload(0);
        for (int k0 = 0; k0 < K; k0 += BK) {
            __syncthreads();   // previous k-tile fully consumed
            lstore();
            __syncthreads();
            if (k0 + BK < K) gload(k0 + BK);   // in flight under the MFMAs below
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                half8_t af[4], bf[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = wm * 64 + i * 16 + r;
                    af[i] = *reinterpret_cast<const half8_t *>(As + row * BK + (((ks * 4 + q) ^ (row & 7)) << 3));
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int row = wn * 64 + j * 16 + r;
                    bf[j] = *reinterpret_cast<const half8_t *>(Bs + row * BK + (((ks * 4 + q) ^ (row & 7)) << 3));
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[j], af[i], acc[i][j], 0, 0, 0);
            }
        }
        // acc[i][j][e] = z[m0 + wm*64 + i*16 + r][n0 + wn*64 + j*16 + 4q + e]: fold the tile into the running state, columns >= V left out
        float bv[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int n = n0 + wn * 64 + j * 16 + 4 * q + e;
                bv[j][e] = (bias && n < V) ? to_f32(bias[n]) : 0.f;
            }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float tmax = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int n = n0 + wn * 64 + j * 16 + 4 * q + e;
                    const float z = n < V ? acc[i][j][e] + bv[j][e] : -INFINITY;
                    acc[i][j][e] = z;
                    tmax = fmaxf(tmax, z);
                    if (z > best_v[i]) {   // ascending n: the first of equal values stays
                        best_v[i] = z;
                        best_id[i] = n;
                    }
                    if (n == tgt[i]) tgt_z[i] = z;
                }
            const float nmax = fmaxf(run_max[i], tmax);
            float s = run_sum[i] * expf(run_max[i] - nmax);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) s += expf(acc[i][j][e] - nmax);   // masked columns: exp(-inf) = 0
            run_sum[i] = s;
            run_max[i] = nmax;
        }
    }

    // the 8 lane states of each row (slot = wn * 4 + q) through LDS, merged by one thread per row in slot order
    __syncthreads();   // every wave is done with the k-tiles
    float *st = reinterpret_cast<float *>(smem);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float *p = st + ((wm * 64 + i * 16 + r) * 8 + wn * 4 + q) * 5;
        p[0] = run_max[i];
        p[1] = run_sum[i];
        p[2] = tgt_z[i];
        p[3] = best_v[i];
        p[4] = __builtin_bit_cast(float, best_id[i]);
    }
    __syncthreads();
    if (tid < BM && m0 + tid < rows) {
        const float *p = st + tid * 8 * 5;
        float mx = p[0];
#pragma unroll
        for (int s = 1; s < 8; ++s) mx = fmaxf(mx, p[s * 5]);
        float sum = 0.f, tz = 0.f, bval = -INFINITY;
        int bid = INT_MAX;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            sum += p[s * 5 + 1] * expf(p[s * 5] - mx);
            tz += p[s * 5 + 2];   // at most one slot holds the target: the others add 0
            const float v = p[s * 5 + 3];
            const int id = __builtin_bit_cast(int, p[s * 5 + 4]);
            if (score_better(v, id, bval, bid)) {
                bval = v;
                bid = id;
            }
        }
        float *dst = part + (static_cast<size_t>(m0 + tid) * spans + span) * kScorePartFloats;
        *reinterpret_cast<floatx4 *>(dst) = floatx4{mx, sum, tz, bval};
        *reinterpret_cast<floatx4 *>(dst + 4) = floatx4{__builtin_bit_cast(float, bid), 0.f, 0.f, 0.f};
    }
}

__global__ __launch_bounds__(256) void score_merge_kernel(const float *__restrict__ part, const int32_t *__restrict__ targets,
                                                          float *__restrict__ out_logprob, float *__restrict__ out_lse,
                                                          int32_t *__restrict__ out_argmax, float *__restrict__ out_argmax_logprob,
                                                          int rows, int V, int spans, int span_cols) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= rows) return;
    const float *p = part + static_cast<size_t>(t) * spans * kScorePartFloats;
    float mx = p[0];
    for (int s = 1; s < spans; ++s) mx = fmaxf(mx, p[s * kScorePartFloats]);
    float sum = 0.f, bval = -INFINITY;
    int bid = INT_MAX;
    for (int s = 0; s < spans; ++s) {   // span order
        const float *ps = p + s * kScorePartFloats;
        sum += ps[1] * expf(ps[0] - mx);
        const int id = __builtin_bit_cast(int, ps[4]);
        if (score_better(ps[3], id, bval, bid)) {
            bval = ps[3];
            bid = id;
        }
    }
    // z - lse as (z - max) - log(sum): the difference of two logits is formed before the small term joins it, so logits of
    // magnitude 200 (fp32 spacing 1.5e-5) cost a log-probability no more than their own rounding
    const float lsum = logf(sum);
    const int tg = targets[t];
    out_logprob[t] = (tg >= 0 && tg < V) ? (p[(tg / span_cols) * kScorePartFloats + 2] - mx) - lsum : 0.f;
    if (out_lse) out_lse[t] = mx + lsum;
    if (out_argmax) out_argmax[t] = bid;
    if (out_argmax_logprob) out_argmax_logprob[t] = (bval - mx) - lsum;
}

}  // namespace

}  // namespace llmie

using namespace llmie;

extern "C" size_t llmie_score_tokens_workspace_bytes(int rows, int hidden, int vocab) {
    if (rows < 1 || hidden < 1 || vocab < 1) return 0;
    return score_x_bytes(rows, hidden) + static_cast<size_t>(rows) * score_spans(vocab).spans * kScorePartFloats * sizeof(float);
}

extern "C" int llmie_score_tokens(const void *hidden, const void *norm_gamma, float rms_eps, const void *lm_head, const void *lm_bias,
                                  const int32_t *targets, float *out_logprob, float *out_lse, int32_t *out_argmax,
                                  float *out_argmax_logprob, int rows, int hidden_size, int vocab, void *workspace,
                                  size_t workspace_bytes, llmie_dtype dtype, llmie_stream stream) {
    LLMIE_REQUIRE(hidden && lm_head && targets && out_logprob, "score_tokens: hidden, lm_head, targets and out_logprob must be non-NULL");
    LLMIE_REQUIRE(rows >= 1 && hidden_size >= 1 && vocab >= 1, "score_tokens: bad shape rows=%d hidden=%d vocab=%d", rows, hidden_size, vocab);
    if (dtype != LLMIE_F16) LLMIE_UNSUPPORTED("score_tokens: dtype %d (fp16 hidden states and LM head only)", (int)dtype);
    if (hidden_size % 64 != 0) LLMIE_UNSUPPORTED("score_tokens: hidden size %d is not a multiple of 64", hidden_size);
    if ((reinterpret_cast<uintptr_t>(hidden) | reinterpret_cast<uintptr_t>(lm_head)) % 16)
        LLMIE_UNSUPPORTED("score_tokens: hidden and lm_head must be 16-byte aligned");
    const size_t need = llmie_score_tokens_workspace_bytes(rows, hidden_size, vocab);
    if (!workspace || workspace_bytes < need || reinterpret_cast<uintptr_t>(workspace) % 16) {
        set_error("score_tokens: workspace of %zu bytes at %p, %zu bytes at a 16-byte aligned address needed "
                  "(llmie_score_tokens_workspace_bytes)", workspace ? workspace_bytes : size_t{0}, workspace, need);
        return LLMIE_ERR_WORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    const ScoreSpans sp = score_spans(vocab);
    half_t *xn = static_cast<half_t *>(workspace);
    float *part = reinterpret_cast<float *>(static_cast<char *>(workspace) + score_x_bytes(rows, hidden_size));
    const half_t *x = static_cast<const half_t *>(hidden);
    if (norm_gamma) {
        // llmie_rmsnorm itself on a copy: the normalised rows are its bits by construction (a device-to-device copy on the stream
        // neither allocates nor synchronises and is legal inside a graph capture)
        const hipError_t e = hipMemcpyAsync(xn, hidden, score_x_bytes(rows, hidden_size), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) {
            set_error("score_tokens: copy of the hidden states failed: %s", hipGetErrorString(e));
            return LLMIE_ERR_LAUNCH;
        }
        const int rc = llmie_rmsnorm(xn, nullptr, norm_gamma, rms_eps, rows, hidden_size, LLMIE_F16, stream);
        if (rc != LLMIE_OK) return rc;
        x = xn;
    }
    const dim3 grid(sp.spans, (rows + kScoreBM - 1) / kScoreBM);
    score_tile_kernel<<<grid, 256, 0, st>>>(x, static_cast<const half_t *>(lm_head), static_cast<const half_t *>(lm_bias), targets, part,
                                            rows, vocab, hidden_size, sp.tiles_per_span, sp.spans);
    const int rc = launch_status("score_tokens(tiles)");
    if (rc != LLMIE_OK) return rc;
    score_merge_kernel<<<(rows + 255) / 256, 256, 0, st>>>(part, targets, out_logprob, out_lse, out_argmax, out_argmax_logprob, rows,
                                                           vocab, sp.spans, sp.tiles_per_span * kScoreBN);
    return launch_status("score_tokens(merge)");
}
