// fp8 (OCP e4m3fn, the gfx950 format -- not MI300's fnuz) linear for the decoder engine:
//   llmie_quantize_fp8      W fp16 [N,K] -> e4m3 [N,K] + fp32 per-row scale (amax/448)
//   llmie_linear_fp8        x fp16 [M,K] is quantised per token to e4m3 on the fly (scale amax/448), then
//                           y[m,n] = wscale[n] * xscale[m] * sum_k Wq[n,k] xq[m,k] on v_mfma_f32_16x16x32_fp8_fp8
//                           (fp32 accumulate): the split-K skinny kernel of gemm_kernels.cuh in its fp8 form (64 weight rows
//                           per workgroup, K sliced over workgroups, e4m3 activation tile shared through swizzled LDS, fp32
//                           slabs); M <= 8 takes the K-split GEMV with the same arithmetic (gemv_ksplit_kernel<.., FP8>).
// A 16-byte weight load per lane = 16 consecutive k of one row = two MFMA A operands with no conversion at all:
// the stream is half the bytes of fp16 and needs no de-quantisation ALU work.
#include "gemm_kernels.cuh"
#include "llmie_internal.h"

#include <cstdlib>

namespace llmie {

typedef long i64_t;

// one workgroup per row: amax -> scale = amax/448 (1 when the row is all zero), q = e4m3(w/scale)
template <typename ST>
__global__ __launch_bounds__(256) void quantize_rows_fp8_kernel(const half_t *__restrict__ w, uint8_t *__restrict__ q,
                                                                float *__restrict__ scale, int K) {
    __shared__ float red[4];
    const size_t row = blockIdx.x;
    const half_t *src = w + row * K;
    float amax = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) amax = fmaxf(amax, fabsf(to_f32(src[k])));
    amax = block_max<4>(amax, red);
    const float s = amax > 0.f ? amax / 448.0f : 1.0f;
    if (threadIdx.x == 0) scale[row] = s;
    unsigned int *dst = reinterpret_cast<unsigned int *>(q + row * K);
    for (int k4 = threadIdx.x; k4 < K / 4; k4 += 256) {
        const int k = 4 * k4;
        dst[k4] = pack4_e4m3(to_f32(src[k]) / s, to_f32(src[k + 1]) / s, to_f32(src[k + 2]) / s, to_f32(src[k + 3]) / s);
    }
}

// Same arithmetic with the row held in registers: 16-byte loads (R chunks of 8 halves per thread), one pass over memory
// (read 2K + write K bytes per row) -- the scalar two-pass form above ran at 1.2 TB/s on [4096, 11008] activations.
template <int R>
__global__ __launch_bounds__(256) void quantize_rows_fp8_vec_kernel(const half_t *__restrict__ w, uint8_t *__restrict__ q,
                                                                    float *__restrict__ scale, int K) {
    __shared__ float red[4];
    const size_t row = blockIdx.x;
    const half8_t *src = reinterpret_cast<const half8_t *>(w + row * K);
    const int nch = K / 8;
    half8_t v[R];
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int c = threadIdx.x + 256 * i;
        v[i] = src[c < nch ? c : nch - 1];
        if (c < nch) {
#pragma unroll
            for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(to_f32(v[i][e])));
        }
    }
    amax = block_max<4>(amax, red);
    const float s = amax > 0.f ? amax / 448.0f : 1.0f;
    if (threadIdx.x == 0) scale[row] = s;
    uint2 *dst = reinterpret_cast<uint2 *>(q + row * K);
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int c = threadIdx.x + 256 * i;
        if (c < nch)
            dst[c] = uint2{pack4_e4m3(to_f32(v[i][0]) / s, to_f32(v[i][1]) / s, to_f32(v[i][2]) / s, to_f32(v[i][3]) / s),
                           pack4_e4m3(to_f32(v[i][4]) / s, to_f32(v[i][5]) / s, to_f32(v[i][6]) / s, to_f32(v[i][7]) / s)};
    }
}

int quantize_rows_fp8(const half_t *x, uint8_t *xq, float *xscale, int M, int K, hipStream_t st) {
    const int per_thread = (K / 8 + 255) / 256;
    if (K % 8 == 0 && per_thread <= 8 && reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(xq) % 8 == 0) {
        if (per_thread <= 2) quantize_rows_fp8_vec_kernel<2><<<M, 256, 0, st>>>(x, xq, xscale, K);
        else if (per_thread <= 4) quantize_rows_fp8_vec_kernel<4><<<M, 256, 0, st>>>(x, xq, xscale, K);
        else if (per_thread <= 6) quantize_rows_fp8_vec_kernel<6><<<M, 256, 0, st>>>(x, xq, xscale, K);
        else quantize_rows_fp8_vec_kernel<8><<<M, 256, 0, st>>>(x, xq, xscale, K);
    } else {
        quantize_rows_fp8_kernel<float><<<M, 256, 0, st>>>(x, xq, xscale, K);
    }
    return launch_status("quantize_rows_fp8");
}

int linear_fp8_gemv(const LinearOperands &o, hipStream_t st) {
    const int M = o.M, K = o.K;
    if (!ksplit_eligible(M, K, 8) || (mis16(o.x) | mis16(o.w)) != 0 || (o.gamma && (mis16(o.gamma) | mis16(o.pre_bias)) != 0)) {
        set_error("linear_fp8: shape M=%d K=%d not on the GEMV path", M, K);
        return LLMIE_ERR_UNSUPPORTED;
    }
    const GemvArgs a{static_cast<const half_t *>(o.x), o.w, static_cast<half_t *>(o.y), K, o.N, static_cast<const half_t *>(o.bias),
                     static_cast<const half_t *>(o.residual), static_cast<const half_t *>(o.gamma), static_cast<const half_t *>(o.pre_bias),
                     o.eps, o.epi, o.gamma ? 1 : 0, o.scale, 0};
    if (!gemv_fp8_launch(M, a, st)) {
        set_error("linear_fp8: no GEMV instantiation for M=%d K=%d", M, K);
        return LLMIE_ERR_UNSUPPORTED;
    }
    return launch_status("linear_fp8(gemv)");
}

int linear_fp8(const LinearOperands &o, const LinearScratch &s, hipStream_t st) {
    const LinearCall c = linear_call(WF_FP8, o, s);
    const LinearPlan p = plan_linear_fp8(c);
    if (p.route == LR_REFUSED) return linear_refuse(c, p);
    if (p.route == LR_FP8_GEMV) return linear_fp8_gemv(o, st);
    const int M = o.M, K = o.K, N = o.N;
    const half_t *bias = static_cast<const half_t *>(o.bias), *residual = static_cast<const half_t *>(o.residual);
    const float *w_scale = static_cast<const float *>(o.scale);
    half_t *y = static_cast<half_t *>(o.y);
    uint8_t *xq = static_cast<uint8_t *>(s.act);
    float *xscale = reinterpret_cast<float *>(xq + fp8_align(static_cast<size_t>(M) * K));
    int rc = quantize_rows_fp8(static_cast<const half_t *>(o.x), xq, xscale, M, K, st);
    if (rc) return rc;
    if (p.route == LR_FP8_GEMM256) {
        gemm256_launch(G256_E4M3, xq, o.w, y, M, N, K, bias, residual, xscale, w_scale, st);
        return launch_status("linear_fp8(gemm256)");
    }
    for (int m0 = 0; m0 < M; m0 += p.pass_rows) {   // LR_FP8_SPLITK
        const int mc = M - m0 < p.pass_rows ? M - m0 : p.pass_rows;
        SplitKSlabs sk;
        rc = linear_splitk_partial(WF_FP8, xq + static_cast<size_t>(m0) * K, o.w, mc, K, N, st, &sk, s.slabs);
        if (rc) return rc;
        rc = splitk_finalize(sk, SlabScale{nullptr, w_scale, xscale + m0}, y + static_cast<size_t>(m0) * N, EPI_NONE, bias,
                             residual ? residual + static_cast<size_t>(m0) * N : nullptr, st);
        if (rc) return rc;
    }
    return launch_status("linear_fp8");
}

}  // namespace llmie

using namespace llmie;

extern "C" size_t llmie_linear_fp8_workspace_bytes(int M, int K, int N) {
    if (M <= 0 || K <= 0 || N < 0) return 0;
    // quantised activations + per-token scales, then the fp32 slabs of the split-K form wherever the shape's plan is not the GEMV (also
    // under the tiled GEMM's sizes -- more than that route needs, kept: callers share one workspace across row counts);
    // N = 0: the activation part only (llmie_linear_fp8_swiglu)
    const bool splitk = N > 0 && plan_linear_fp8(linear_call_sizing(WF_FP8, M, K, N, EPI_NONE)).route != LR_FP8_GEMV;
    return fp8_act_bytes(M, K) + (splitk ? fp8_align(linear_splitk_ws_floats(WF_FP8, M, K, N) * sizeof(float)) : 0);
}

extern "C" int llmie_quantize_fp8(const void *w, uint8_t *wq, float *scale, int N, int K, llmie_stream stream) {
    LLMIE_REQUIRE(w && wq && scale && N > 0 && K > 0 && K % 4 == 0, "quantize_fp8: bad arguments (K %% 4 == 0)");
    return quantize_rows_fp8((const half_t *)w, wq, scale, N, K, as_stream(stream));
}

extern "C" int llmie_linear_fp8(const void *x, const uint8_t *w_fp8, const float *w_scale, void *y, int M, int K, int N,
                                const void *bias, const void *residual, void *workspace, size_t workspace_bytes,
                                llmie_stream stream) {
    LLMIE_REQUIRE(x && w_fp8 && w_scale && y && workspace, "linear_fp8: NULL pointer");
    LLMIE_REQUIRE(M > 0 && K > 0 && N > 0, "linear_fp8: bad shape");
    const size_t act = fp8_act_bytes(M, K);
    if (workspace_bytes < act) {
        set_error("linear_fp8: workspace too small (%zu < %zu bytes)", workspace_bytes, llmie_linear_fp8_workspace_bytes(M, K, N));
        return LLMIE_ERR_WORKSPACE;
    }
    const SlabWs slabs{reinterpret_cast<float *>(static_cast<char *>(workspace) + act), (workspace_bytes - act) / sizeof(float)};
    return linear_fp8(LinearOperands{x, w_fp8, w_scale, y, M, K, N, EPI_NONE, 0, bias, residual}, LinearScratch{slabs, nullptr, 0, workspace, act},
                      as_stream(stream));
}

extern "C" int llmie_linear_fp8_swiglu(const void *x, const uint8_t *w_fp8, const float *w_scale, void *y, int M, int K,
                                       int two_inter, void *workspace, size_t workspace_bytes, llmie_stream stream) {
    LLMIE_REQUIRE(x && w_fp8 && w_scale && y && workspace, "linear_fp8_swiglu: NULL pointer");
    LLMIE_REQUIRE(M > 0 && K > 0 && two_inter > 0 && two_inter % 2 == 0, "linear_fp8_swiglu: bad shape");
    if (!gemm256_swiglu_fills(M, two_inter) || K % 128 != 0 || reinterpret_cast<uintptr_t>(w_fp8) % 16 ||
        reinterpret_cast<uintptr_t>(workspace) % 256 || reinterpret_cast<uintptr_t>(y) % 8)
        LLMIE_UNSUPPORTED("linear_fp8_swiglu: prefill-sized shapes only (>= 192 tiles of 256 tokens x 128 columns, K %% 128 == 0, "
                          "two_inter %% 8 == 0); use llmie_linear_fp8 + llmie_silu_and_mul otherwise");
    if (workspace_bytes < llmie_linear_fp8_workspace_bytes(M, K, 0)) {
        set_error("linear_fp8_swiglu: workspace too small");
        return LLMIE_ERR_WORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    uint8_t *xq = static_cast<uint8_t *>(workspace);
    float *xscale = reinterpret_cast<float *>(xq + fp8_align(static_cast<size_t>(M) * K));
    const int rc = quantize_rows_fp8((const half_t *)x, xq, xscale, M, K, st);
    if (rc) return rc;
    gemm256_swiglu_launch(G256_E4M3, xq, w_fp8, (half_t *)y, M, two_inter, K, xscale, w_scale, st);
    return launch_status("linear_fp8_swiglu");
}

