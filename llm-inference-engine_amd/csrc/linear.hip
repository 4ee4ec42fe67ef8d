// llmie_linear / llmie_batched_gemm: shape dispatch over the kernels in gemm_kernels.cuh.
#include "gemm_kernels.cuh"
#include "gemm256.cuh"
#include "gemm8p.cuh"
#include "gemm_mid.cuh"
#include "llmie_internal.h"

#include <algorithm>
#include <cstdlib>

namespace llmie {

// ---- decode GEMV dispatch ----
// K-split kernel: XC = 16-byte chunks per thread = ceil(K*WBITS/128/256) rounded up to a form of the table below; RPW rows per
// iteration so that RPW*XC ~ 16 loads are in flight per lane; register budget M*XC*XE <= 16 half8 of activations.
template <int M, int RPW, int XC, int WBITS, bool DB = false, bool FP8 = false, int RI = 1> static void launch_ksplit(const GemvArgs &a, hipStream_t st) {
    const bool swiglu = a.epi == EPI_SWIGLU;
    const int groups = swiglu ? (a.N / 2 + (RPW / 2) * RI - 1) / ((RPW / 2) * RI) : (a.N + RPW * RI - 1) / (RPW * RI);
    // long-lived workgroups (the prologue -- activation slice + norm -- is paid once per workgroup), evenly loaded
    // (measured per format, interleaved A/B of whole decode steps: fp16 and int4 +0.4 .. +2 % with 512 against 768, int8 -0.6 %, fp8 -2 .. -7 %;
    // 384 and 1024 lose everywhere)
    constexpr int target = (WBITS == 16 || WBITS == 4) ? 512 : 768;
    const int iters = (groups + target - 1) / target;
    const int grid = (groups + iters - 1) / iters;
    gemv_ksplit_kernel<M, RPW, XC, WBITS, DB, FP8, RI><<<grid, 256, 0, st>>>(a);
}

static int ksplit_xc(int K, int wbits) { return (K * wbits / 128 + 255) / 256; }

// The forms of the K-split kernel, by 16-byte chunks per thread: a row of ksplit_xc chunks runs on the first form that covers it, if
// M rows of it fit the register budget.  One table for the eligibility test and for the launcher.
struct KsplitForm {
    int xc, rpw;   // chunks per thread, rows per iteration (xc = 0: no such form)
};
constexpr int kKsplitForms = 5;
constexpr KsplitForm ksplit_form_at(int wbits, bool fp8, int i) {
    // fp16, two chunks: 4 rows per iteration in A/B against 8 x 2 (+1.6 % batch 1, +4.4 % batch 3) and 2 x 2, 16 x 2
    constexpr KsplitForm f16[kKsplitForms] = {{1, 8}, {2, 4}, {4, 4}, {6, 4}, {8, 2}};
    // quantised rows are short: double buffered (16 loads in flight per lane)
    constexpr KsplitForm q[kKsplitForms] = {{1, 8}, {2, 4}, {3, 2}, {0, 0}, {0, 0}};
    if (wbits == 16) return f16[i];
    if (i == 0 && wbits == 8 && !fp8) return KsplitForm{1, 4};   // int8: 4 rows per iteration (+2.8 % in A/B); fp8, int4: 8
    return q[i];
}
// index of the form that takes (M, K), -1: none
static int ksplit_form(int M, int K, int wbits) {
    if (M < 1 || M > 8 || K % (128 / wbits) != 0) return -1;   // whole 16-byte chunks
    const int xe = wbits == 16 ? 1 : (wbits == 8 ? 2 : 4);
    const int xc = ksplit_xc(K, wbits);
    for (int i = 0; i < kKsplitForms; ++i) {
        const KsplitForm f = ksplit_form_at(wbits, false, i);
        if (f.xc && xc <= f.xc) return M * f.xc * xe <= 16 ? i : -1;
    }
    return -1;
}
bool ksplit_eligible(int M, int K, int wbits) { return ksplit_form(M, K, wbits) >= 0; }

template <int M, int WBITS, bool FP8, int I> static void launch_ksplit_form(const GemvArgs &a, hipStream_t st) {
    constexpr KsplitForm f = ksplit_form_at(WBITS, FP8, I);
    if constexpr (f.xc != 0 && M * f.xc * WFmt<WBITS>::XE <= 16) {   // (register budget: ksplit_form picks no other)
        if constexpr (WBITS == 4 && I == 0) {
            // rows of at most 2 KiB (K <= 4096): two consecutive rows per workgroup instruction, or half the threads idle
            if (a.K * WBITS / 128 <= 128 && (a.epi != EPI_SWIGLU || (a.N / 2) % 2 == 0)) {
                launch_ksplit<M, 8, 1, WBITS, true, FP8, 2>(a, st);
                return;
            }
        }
        launch_ksplit<M, f.rpw, f.xc, WBITS, WBITS != 16, FP8>(a, st);
    }
}
template <int M, int WBITS, bool FP8 = false> static void dispatch_ksplit(int form, const GemvArgs &a, hipStream_t st) {
    switch (form) {
        case 0: launch_ksplit_form<M, WBITS, FP8, 0>(a, st); break;
        case 1: launch_ksplit_form<M, WBITS, FP8, 1>(a, st); break;
        case 2: launch_ksplit_form<M, WBITS, FP8, 2>(a, st); break;
        case 3: launch_ksplit_form<M, WBITS, FP8, 3>(a, st); break;
        case 4: launch_ksplit_form<M, WBITS, FP8, 4>(a, st); break;
        default: break;
    }
}

// the GEMV family's route for M rows of K (16-byte aligned operands): K-split register budget, else the LDS fallback's 64 KB
static int gemv_f16_route(int M, int K) {
    if (K % 8 || M < 1 || M > 8) return LR_REFUSED;
    if (ksplit_form(M, K, 16) >= 0) return LR_GEMV_KSPLIT;
    return static_cast<size_t>(M) * K * 2 <= 64 * 1024 ? LR_GEMV_LDS : LR_REFUSED;
}

template <int M> static void dispatch_gemv_m(const GemvArgs &a, hipStream_t st) {
    const int form = ksplit_form(M, a.K, 16);
    if (form >= 0) return dispatch_ksplit<M, 16>(form, a, st);
    const bool swiglu = a.epi == EPI_SWIGLU;
    const int npairs = swiglu ? a.N / 2 : (a.N + 1) / 2;
    int wgs = (npairs + 3) / 4;
    if (wgs > 2048) wgs = 2048;
    gemv_lds_kernel<M><<<wgs, 256, static_cast<size_t>(M) * a.K * sizeof(half_t), st>>>(a);
}

// fp16 GEMV; needs gemv_f16_route(M, a.K) != LR_REFUSED
static void dispatch_gemv(int M, const GemvArgs &a, hipStream_t st) {
    switch (M) {
        case 1: return dispatch_gemv_m<1>(a, st);
        case 2: return dispatch_gemv_m<2>(a, st);
        case 3: return dispatch_gemv_m<3>(a, st);
        case 4: return dispatch_gemv_m<4>(a, st);
        case 5: return dispatch_gemv_m<5>(a, st);
        case 6: return dispatch_gemv_m<6>(a, st);
        case 7: return dispatch_gemv_m<7>(a, st);
        case 8: return dispatch_gemv_m<8>(a, st);
        default: return;
    }
}

// quantised-weight GEMV (M <= 8): true when launched (a form of the table takes the shape)
template <int WBITS, bool FP8 = false> static bool dispatch_gemv_q(int M, const GemvArgs &a, hipStream_t st) {
    const int form = ksplit_form(M, a.K, WBITS);
    if (form < 0) return false;
    switch (M) {
        case 1: dispatch_ksplit<1, WBITS, FP8>(form, a, st); break;
        case 2: dispatch_ksplit<2, WBITS, FP8>(form, a, st); break;
        case 3: dispatch_ksplit<3, WBITS, FP8>(form, a, st); break;
        case 4: dispatch_ksplit<4, WBITS, FP8>(form, a, st); break;
        case 5: dispatch_ksplit<5, WBITS, FP8>(form, a, st); break;
        case 6: dispatch_ksplit<6, WBITS, FP8>(form, a, st); break;
        case 7: dispatch_ksplit<7, WBITS, FP8>(form, a, st); break;
        default: dispatch_ksplit<8, WBITS, FP8>(form, a, st); break;
    }
    return true;
}
void gemv_q_launch(int wbits, int M, const GemvArgs &a, hipStream_t st) {
    if (wbits == 8) dispatch_gemv_q<8>(M, a, st);
    else dispatch_gemv_q<4>(M, a, st);
}
// fp8 (e4m3 weights, fp32 row scales in a.scale, activations quantised per token in the prologue)
bool gemv_fp8_launch(int M, const GemvArgs &a, hipStream_t st) { return dispatch_gemv_q<8, true>(M, a, st); }

template <int EPI>
static void dispatch_skinny(int M, const half_t *x, const half_t *W, half_t *y, int K, int N,
                            const half_t *bias, const half_t *residual, hipStream_t st) {
    constexpr int NW = 8;
    const int mt = (M + 15) / 16;
    if constexpr (EPI == EPI_SWIGLU) {
        const int wgs = (N / 2 + 15) / 16;
        switch (mt) {
            case 1: skinny_mfma_f16_kernel<1, 2, NW, EPI><<<wgs, NW * 64, 0, st>>>(x, W, y, M, K, N, bias, residual); break;
            case 2: skinny_mfma_f16_kernel<2, 2, NW, EPI><<<wgs, NW * 64, 0, st>>>(x, W, y, M, K, N, bias, residual); break;
            case 3: skinny_mfma_f16_kernel<3, 2, NW, EPI><<<wgs, NW * 64, 0, st>>>(x, W, y, M, K, N, bias, residual); break;
            case 4: skinny_mfma_f16_kernel<4, 2, NW, EPI><<<wgs, NW * 64, 0, st>>>(x, W, y, M, K, N, bias, residual); break;
            default: break;
        }
    } else {
        const int tiles = (N + 15) / 16;
        switch (mt) {
            case 1: skinny_mfma_f16_kernel<1, 1, NW, EPI><<<tiles, NW * 64, 0, st>>>(x, W, y, M, K, N, bias, residual); break;
            case 2: skinny_mfma_f16_kernel<2, 2, NW, EPI><<<(tiles + 1) / 2, NW * 64, 0, st>>>(x, W, y, M, K, N, bias, residual); break;
            case 3: skinny_mfma_f16_kernel<3, 2, NW, EPI><<<(tiles + 1) / 2, NW * 64, 0, st>>>(x, W, y, M, K, N, bias, residual); break;
            case 4: skinny_mfma_f16_kernel<4, 2, NW, EPI><<<(tiles + 1) / 2, NW * 64, 0, st>>>(x, W, y, M, K, N, bias, residual); break;
            default: break;
        }
    }
}

template <typename T>
static void launch_generic(const T *a, const T *b, T *c, int batch, int M, int N, int K, bool trans_b,
                           const T *bias, const T *residual, hipStream_t st) {
    dim3 grid((N + 63) / 64, (M + 63) / 64, batch);
    const size_t sa = static_cast<size_t>(M) * K, sb = static_cast<size_t>(N) * K, sc = static_cast<size_t>(M) * N;
    if (trans_b)
        generic_gemm_kernel<T, true><<<grid, 256, 0, st>>>(a, b, c, M, N, K, sa, sb, sc, bias, residual);
    else
        generic_gemm_kernel<T, false><<<grid, 256, 0, st>>>(a, b, c, M, N, K, sa, sb, sc, bias, residual);
}

// fp16, W[N,K]: the decode / prefill projection path.  epi selects the fused epilogue; a non-null
// `norm` fuses rmsnorm(x + pre_bias)*gamma in front of the projection (GEMV path only: returns
// LLMIE_ERR_UNSUPPORTED otherwise so the caller can run the norm as its own kernel).
// y = sum over the KS slabs (* scales of the weight format) (+bias)(+residual) | SwiGLU over (n, N/2+n)
static __global__ __launch_bounds__(256) void skinny_finalize_kernel(const float *__restrict__ slab, half_t *y, int M, int N, int KS,
                                                              const SlabScale scale, const half_t *__restrict__ bias,
                                                              const half_t *residual, int epi) {
    const int out_n = epi == EPI_SWIGLU ? N / 2 : N;
    const size_t total = static_cast<size_t>(M) * out_n;
    const size_t slab_sz = static_cast<size_t>(M) * N;
    for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < total; i += static_cast<size_t>(gridDim.x) * 256) {
        const int m = static_cast<int>(i / out_n), n = static_cast<int>(i - static_cast<size_t>(m) * out_n);
        auto gather = [&](int col) {
            float v = 0.f;
            for (int k = 0; k < KS; ++k) v += slab[k * slab_sz + static_cast<size_t>(m) * N + col];
            return scale.apply(v, m, col);
        };
        float v;
        if (epi == EPI_SWIGLU) {
            const float gt = gather(n), up = gather(n + out_n);
            v = (gt / (1.0f + expf(-gt))) * up;
        } else {
            v = gather(n);
            if (bias) v += to_f32(bias[n]);
            if (residual) v += to_f32(residual[static_cast<size_t>(m) * N + n]);
        }
        y[static_cast<size_t>(m) * out_n + n] = from_f32<half_t>(v);
    }
}

// The same consumer, four columns per thread and every slab load of them in flight at once (round 3).  skinny_finalize_kernel
// above walks the KS slabs of ONE element with dependent loads -- the slabs were just written by other XCDs, so each is a full
// memory round trip: 7.4 us per launch at 128 x 12288 x 4 slabs, which is mostly 4 serial latencies.  Same summation order
// (s0 + s1 + ...), same arithmetic per element: bit-identical results.  N % 4 == 0 (SwiGLU: N % 8 == 0).
template <bool SWIGLU>
static __global__ __launch_bounds__(256) void splitk_finalize4_kernel(const float *__restrict__ slab, half_t *y, int M, int N, int KS,
                                                                      const SlabScale scale, const half_t *__restrict__ bias,
                                                                      const half_t *residual) {
    const int out_n = SWIGLU ? N / 2 : N, n4 = out_n / 4;
    const size_t total = static_cast<size_t>(M) * n4, slab_sz = static_cast<size_t>(M) * N;
    constexpr int NV = SWIGLU ? 2 : 1;   // column groups per item: the gate columns and the matching up columns
    for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < total; i += static_cast<size_t>(gridDim.x) * 256) {
        const int m = static_cast<int>(i / n4), n = static_cast<int>(i - static_cast<size_t>(m) * n4) * 4;
        floatx4 v[NV];
        for (int k0 = 0; k0 < KS; k0 += 8) {
            floatx4 t[8][NV];
#pragma unroll
            for (int kk = 0; kk < 8; ++kk)
#pragma unroll
                for (int g = 0; g < NV; ++g)
                    t[kk][g] = *reinterpret_cast<const floatx4 *>(slab + static_cast<size_t>(min(k0 + kk, KS - 1)) * slab_sz +
                                                                  static_cast<size_t>(m) * N + n + g * out_n);
#pragma unroll
            for (int kk = 0; kk < 8; ++kk)
                if (k0 + kk < KS) {
#pragma unroll
                    for (int g = 0; g < NV; ++g) {
                        if (k0 + kk == 0) v[g] = floatx4{0.f, 0.f, 0.f, 0.f} + t[kk][g];
                        else v[g] += t[kk][g];
                    }
                }
        }
        half4_t o4;
        if constexpr (SWIGLU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float gt = scale.apply(v[0][e], m, n + e), up = scale.apply(v[1][e], m, n + e + out_n);
                o4[e] = from_f32<half_t>((gt / (1.0f + expf(-gt))) * up);
            }
        } else {
            half4_t b4{0, 0, 0, 0}, r4{0, 0, 0, 0};
            if (bias) b4 = *reinterpret_cast<const half4_t *>(bias + n);
            if (residual) r4 = *reinterpret_cast<const half4_t *>(residual + static_cast<size_t>(m) * N + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float t = scale.apply(v[0][e], m, n + e);
                if (bias) t += to_f32(b4[e]);
                if (residual) t += to_f32(r4[e]);
                o4[e] = from_f32<half_t>(t);
            }
        }
        *reinterpret_cast<half4_t *>(y + static_cast<size_t>(m) * out_n + n) = o4;
    }
}
static void launch_finalize(const float *slab, half_t *y, int M, int N, int KS, const SlabScale &sc, const half_t *bias, const half_t *residual,
                            int epi, hipStream_t st) {
    const int out_n = epi == EPI_SWIGLU ? N / 2 : N;
    const bool vec = out_n % 4 == 0 && (reinterpret_cast<uintptr_t>(slab) % 16) == 0 &&
                     ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(residual)) % 8) == 0;
    if (vec) {
        const size_t items = static_cast<size_t>(M) * (out_n / 4);
        int fgrid = static_cast<int>((items + 255) / 256);
        if (fgrid > 4096) fgrid = 4096;
        if (epi == EPI_SWIGLU) splitk_finalize4_kernel<true><<<fgrid, 256, 0, st>>>(slab, y, M, N, KS, sc, bias, residual);
        else splitk_finalize4_kernel<false><<<fgrid, 256, 0, st>>>(slab, y, M, N, KS, sc, bias, residual);
        return;
    }
    const size_t total = static_cast<size_t>(M) * out_n;
    int fgrid = static_cast<int>((total + 255) / 256);
    if (fgrid > 2048) fgrid = 2048;
    skinny_finalize_kernel<<<fgrid, 256, 0, st>>>(slab, y, M, N, KS, sc, bias, residual, epi);
}

// Split-K planning, shared by the launcher and by the workspace-size query (the slabs are CALLER-owned: nothing on the
// compute path allocates, so a first call may already run under hipGraph capture).
constexpr int kSplitKPassRows = 128;   // activation rows per pass (16 per MFMA tile)
struct SplitKPlan {
    int form;   // 0 = 64-weight-row skinny kernel, 1 = 128-row LDS-DMA kernel (gemm_mid.cuh), 2 = its 64-row form
    int ks;     // K slices = slabs
    int per;    // form 1 / 2: K tiles per slice; form 0: sub-blocks per slice
    int wn;     // form 1 / 2: 64-row groups per workgroup (4 = 256 weight rows)
    bool ok;
};
static SplitKPlan splitk_plan(int wbits, int M, int K, int N) {
    SplitKPlan p{0, 1, 0, 2, false};
    const int bk = wbits == 16 ? 128 : (wbits == 4 ? 512 : 256);  // k per sub-block (4 weight loads per lane)
    if (wbits == 4 && (M > 64 || K % 256)) return p;
    if (M < 1 || M > kSplitKPassRows || (wbits != 4 && K % bk) || K < 512 || (wbits != 16 && wbits != 8 && wbits != 4 && wbits != WF_FP8))
        return p;
    p.ok = true;
    // 64 < M <= 128, fp16 or e4m3 operands: 128-row LDS-DMA kernel; 32 < M <= 64: its 64-row form (measured fp16 M=64:
    // gate/up 55.6 -> 44.7 us, qkv 33.0 -> 29.8, down 29.2 -> 25.8 against the skinny kernel; about equal at M = 32)
    const bool mid64 = M <= 64 && M >= 33;
    // (int8 weights, round 3: the same kernel with raw int8 weight tiles; 128 or 256 weight rows per workgroup, from 65 rows)
    if ((wbits == 16 || wbits == WF_FP8 || (wbits == 8 && M >= 65)) && (M >= 65 || mid64) && K % 128 == 0 && N >= 128) {
        const bool fp8 = wbits == WF_FP8;
        p.form = mid64 ? 2 : 1;
        const int KT = K / (fp8 ? 128 : 64);
        auto slices = [&](int wn) {
            const int mtiles = (N + 64 * wn - 1) / (64 * wn);
            int ks = 256 / mtiles;
            ks = ks < 1 ? 1 : (ks > 8 ? 8 : ks);
            if (ks > KT / 4) ks = KT / 4 > 0 ? KT / 4 : 1;
            return ks;
        };
        p.wn = N >= 8192 ? 4 : 2;   // wide N: 256 weight rows per workgroup
        if (N >= 8192) {
            // one workgroup per CU: tiles x slices should come close to 256 -- 192-row tiles where they fill the chip better than
            // 256-row ones (N = 22016: 115 x 2 = 230 against 86 x 2 = 172; N = 12288: 64 x 4 = 256, one slab less than 48 x 5)
            const int t4 = (N + 255) / 256, t3 = (N + 191) / 192;
            if (t3 * slices(3) > t4 * slices(4)) p.wn = 3;
        }
        const int ks = slices(p.wn);
        p.per = (KT + ks - 1) / ks;
        p.ks = (KT + p.per - 1) / p.per;  // every slice non-empty
        return p;
    }
    const int tiles = (N + 63) / 64, total_blocks = (K + bk - 1) / bk;
    // K slices: enough workgroups to fill the chip (512), but >= 4 sub-blocks per slice (the weight ring depth) and as few
    // slabs as possible (slab traffic = 2 * KS * M * N * 4 bytes)
    int KS = 1;
    const int min_blocks = wbits == 4 ? 1 : 4;  // int4 sub-blocks are 512 k wide: K = 4096 has only 8 of them
    while (KS < 16 && tiles * KS < 512 && total_blocks / (KS * 2) >= min_blocks) KS *= 2;
    p.ks = KS;
    p.per = (total_blocks + KS - 1) / KS;
    return p;
}
// fp32 floats of slab workspace a split-K projection of M rows needs (M > 128 runs in passes of 128 rows that reuse it);
// 0 = this shape has no split-K form
size_t linear_splitk_ws_floats(int wbits, int M, int K, int N) {
    const int rows = wbits == 4 ? (M < 64 ? M : 64) : (M < kSplitKPassRows ? M : kSplitKPassRows);
    if (rows < 1) return 0;
    const SplitKPlan p = splitk_plan(wbits, rows, K, N);
    return p.ok ? static_cast<size_t>(p.ks) * rows * N : 0;
}

// split-K skinny MFMA path, first half: partial products of one pass (M <= 128) into the caller's fp32 slabs [KS][M][N]
// (`ws`, >= linear_splitk_ws_floats floats, 16-byte aligned).  The consumer (finalize kernel, splitk_rownorm, or the
// decode attention reading q/k/v straight from the slabs) must be enqueued before the next launch that writes `ws`.
int linear_splitk_partial(int wbits, const void *x, const void *W, int M, int K, int N, hipStream_t st, SplitKSlabs *out,
                          SlabWs ws, const half_t *gscale) {
    // wbits: 16 = fp16 weights, 8 = int8 weights, 4 = int4 weights with group-128 scales `gscale` applied in the kernel (all
    // with fp16 activations), WF_FP8 = e4m3 weights and e4m3 activations
    const SplitKPlan p = splitk_plan(wbits, M, K, N);
    if (wbits == 4 && (!gscale || reinterpret_cast<uintptr_t>(gscale) % 4 || !p.ok)) {
        set_error("linear(split-K int4): needs M <= 64 per pass, K %% 256 == 0, group-128 scales");
        return LLMIE_ERR_UNSUPPORTED;
    }
    if (!p.ok || (reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(W)) % 16) {
        set_error("linear(split-K): unsupported shape M=%d K=%d (bits=%d)", M, K, wbits);
        return LLMIE_ERR_UNSUPPORTED;
    }
    const size_t need = static_cast<size_t>(p.ks) * M * N;
    if (!ws.p || ws.floats < need || reinterpret_cast<uintptr_t>(ws.p) % 16) {
        set_error("linear(split-K): slab workspace too small or misaligned (%zu < %zu bytes); size it with "
                  "llmie_linear_workspace_bytes()", ws.p ? ws.floats * sizeof(float) : static_cast<size_t>(0), need * sizeof(float));
        return LLMIE_ERR_WORKSPACE;
    }
    if (p.form != 0) {
        const bool fp8 = wbits == WF_FP8, mid64 = p.form == 2;
        const int wn = p.wn, ks = p.ks, per = p.per;
        const int mtiles = (N + 64 * wn - 1) / (64 * wn);
        float *mslab = ws.p;
    static const bool attr_set = [] {   // once per process, thread-safe (function-local static initialisation)
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mid_splitk_kernel<false, 4, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 16384);
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mid_splitk_kernel<true, 4, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 3 * 16384);
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mid_splitk_kernel<false, 2, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 2 * 16384);
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mid_splitk_kernel<true, 2, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 2 * 16384);
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mid_splitk_kernel<false, 3, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 40960);
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mid_splitk_kernel<true, 3, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * 40960);
            return true;
        }();
        (void)attr_set;
        const dim3 mgrid(mtiles * ks);
        if (wbits == 8) {   // int8 weights: stage = 16 KiB of activations + 16 KiB (192 / 256 rows) or 8 KiB (128 rows) of weights
            static const bool attrq = [] {
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mid_splitk_kernel<false, 4, 5, 128, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, 5 * 32768);
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mid_splitk_kernel<false, 3, 5, 128, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, 5 * 32768);
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mid_splitk_kernel<false, 2, 6, 128, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, 6 * 24576);
                return true;
            }();
            (void)attrq;
            if (wn == 4) mid_splitk_kernel<false, 4, 5, 128, 8><<<mgrid, 512, 5 * 32768, st>>>(x, W, mslab, M, N, K, ks, per);
            else if (wn == 3) mid_splitk_kernel<false, 3, 5, 128, 8><<<mgrid, 512, 5 * 32768, st>>>(x, W, mslab, M, N, K, ks, per);
            else mid_splitk_kernel<false, 2, 6, 128, 8><<<mgrid, 512, 6 * 24576, st>>>(x, W, mslab, M, N, K, ks, per);
        } else if (mid64) {
            static const bool attr64 = [] {   // once per process, thread-safe (function-local static initialisation)
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mid_splitk_kernel<false, 4, 4, 64>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 40960);
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mid_splitk_kernel<true, 4, 4, 64>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 40960);
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mid_splitk_kernel<false, 2, 6, 64>), hipFuncAttributeMaxDynamicSharedMemorySize, 6 * 24576);
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mid_splitk_kernel<true, 2, 6, 64>), hipFuncAttributeMaxDynamicSharedMemorySize, 6 * 24576);
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mid_splitk_kernel<false, 3, 5, 64>), hipFuncAttributeMaxDynamicSharedMemorySize, 5 * 32768);
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mid_splitk_kernel<true, 3, 5, 64>), hipFuncAttributeMaxDynamicSharedMemorySize, 5 * 32768);
                return true;
            }();
            (void)attr64;
            if (wn == 4) {
                if (fp8) mid_splitk_kernel<true, 4, 4, 64><<<mgrid, 512, 4 * 40960, st>>>(x, W, mslab, M, N, K, ks, per);
                else mid_splitk_kernel<false, 4, 4, 64><<<mgrid, 512, 4 * 40960, st>>>(x, W, mslab, M, N, K, ks, per);
            } else if (wn == 3) {   // stage = 8 KiB of activations + 24 KiB of weights: five stages fill the 160 KiB exactly
                if (fp8) mid_splitk_kernel<true, 3, 5, 64><<<mgrid, 512, 5 * 32768, st>>>(x, W, mslab, M, N, K, ks, per);
                else mid_splitk_kernel<false, 3, 5, 64><<<mgrid, 512, 5 * 32768, st>>>(x, W, mslab, M, N, K, ks, per);
            } else {
                if (fp8) mid_splitk_kernel<true, 2, 6, 64><<<mgrid, 512, 6 * 24576, st>>>(x, W, mslab, M, N, K, ks, per);
                else mid_splitk_kernel<false, 2, 6, 64><<<mgrid, 512, 6 * 24576, st>>>(x, W, mslab, M, N, K, ks, per);
            }
        } else if (wn == 4) {
            if (fp8) mid_splitk_kernel<true, 4, 3><<<mgrid, 512, 3 * 3 * 16384, st>>>(x, W, mslab, M, N, K, ks, per);
            else mid_splitk_kernel<false, 4, 3><<<mgrid, 512, 3 * 3 * 16384, st>>>(x, W, mslab, M, N, K, ks, per);
        } else if (wn == 3) {
            if (fp8) mid_splitk_kernel<true, 3, 3><<<mgrid, 512, 3 * 40960, st>>>(x, W, mslab, M, N, K, ks, per);
            else mid_splitk_kernel<false, 3, 3><<<mgrid, 512, 3 * 40960, st>>>(x, W, mslab, M, N, K, ks, per);
        } else {
            if (fp8) mid_splitk_kernel<true, 2, 4><<<mgrid, 512, 4 * 2 * 16384, st>>>(x, W, mslab, M, N, K, ks, per);
            else mid_splitk_kernel<false, 2, 4><<<mgrid, 512, 4 * 2 * 16384, st>>>(x, W, mslab, M, N, K, ks, per);
        }
        out->slab = mslab;
        out->KS = ks;
        out->M = M;
        out->N = N;
        return launch_status("linear(split-K 128-row)");
    }
    const int tiles = (N + 63) / 64, KS = p.ks, spp = p.per;
    float *slab = ws.p;
    const int mt = (M + 15) / 16;
    const dim3 grid(tiles * KS);
#define LLMIE_SK(MT_)                                                                                          \
    (wbits == 16 ? skinny_splitk_kernel<MT_, 16><<<grid, 256, 0, st>>>(x, W, slab, M, K, N, KS, spp, nullptr)     \
     : wbits == 8 ? skinny_splitk_kernel<MT_, 8><<<grid, 256, 0, st>>>(x, W, slab, M, K, N, KS, spp, nullptr)     \
                  : skinny_splitk_kernel<MT_, 8, true><<<grid, 256, 0, st>>>(x, W, slab, M, K, N, KS, spp, nullptr))
    if (wbits == 4) {
        switch (mt) {
            case 1: skinny_splitk_kernel<1, 4><<<grid, 256, 0, st>>>(x, W, slab, M, K, N, KS, spp, gscale); break;
            case 2: skinny_splitk_kernel<2, 4><<<grid, 256, 0, st>>>(x, W, slab, M, K, N, KS, spp, gscale); break;
            case 3: skinny_splitk_kernel<3, 4><<<grid, 256, 0, st>>>(x, W, slab, M, K, N, KS, spp, gscale); break;
            default: skinny_splitk_kernel<4, 4><<<grid, 256, 0, st>>>(x, W, slab, M, K, N, KS, spp, gscale); break;
        }
    } else
    switch (mt) {
        case 1: LLMIE_SK(1); break;
        case 2: LLMIE_SK(2); break;
        case 3: LLMIE_SK(3); break;
        case 4: LLMIE_SK(4); break;
        case 5: LLMIE_SK(5); break;
        case 6: LLMIE_SK(6); break;
        case 7: LLMIE_SK(7); break;
        default: LLMIE_SK(8); break;
    }
#undef LLMIE_SK
    out->slab = slab;
    out->KS = KS;
    out->M = M;
    out->N = N;
    return launch_status("linear(split-K)");
}

// split-K skinny MFMA path: 8 < M (any M, 128 rows of x per pass); wbits 16 or 8
int linear_splitk(int wbits, const LinearOperands &o, const LinearScratch &s, hipStream_t st) {
    // wbits 8: `scale` = per-row fp16 scales applied by the finalize; wbits 4: `scale` = group-128 scales applied in the kernel
    const half_t *x = static_cast<const half_t *>(o.x), *scale = static_cast<const half_t *>(o.scale);
    const half_t *bias = static_cast<const half_t *>(o.bias), *residual = static_cast<const half_t *>(o.residual);
    half_t *y = static_cast<half_t *>(o.y);
    const void *W = o.w;
    const int M = o.M, K = o.K, N = o.N, epi = o.epi;
    const SlabWs ws = s.slabs;
    const int mpass = wbits == 4 ? 64 : kSplitKPassRows;
    const int out_n = epi == EPI_SWIGLU ? N / 2 : N;
    for (int m0 = 0; m0 < M; m0 += mpass) {
        const int mc = M - m0 < mpass ? M - m0 : mpass;
        SplitKSlabs sk;
        const int rc = linear_splitk_partial(wbits, x + static_cast<size_t>(m0) * K, W, mc, K, N, st, &sk, ws, wbits == 4 ? scale : nullptr);
        if (rc) return rc;
        launch_finalize(sk.slab, y + static_cast<size_t>(m0) * out_n, mc, N, sk.KS, SlabScale{wbits == 4 ? nullptr : scale, nullptr, nullptr}, bias,
                        residual ? residual + static_cast<size_t>(m0) * N : nullptr, epi, st);
    }
    return launch_status("linear(split-K)");
}

// elementwise consumer of the slabs: y = scale(sum_ks slab) (+bias) (+residual) | SwiGLU over (n, N/2 + n)
int splitk_finalize(const SplitKSlabs &sk, const SlabScale &sc, half_t *y, int epi, const half_t *bias, const half_t *residual,
                    hipStream_t st) {
    launch_finalize(sk.slab, y, sk.M, sk.N, sk.KS, sc, bias, residual, epi, st);
    return launch_status("linear(split-K finalize)");
}

// Row epilogue of a split-K projection fused with the residual stream and the next RMSNorm (one launch instead of
// finalize + launchFusedAddBiasResidualAndRMSNorm, add_residual_and_rmsnorm.cu:43-121 semantics):
//   t = sum_ks slab[ks][m][:] (* wscale[:]) + resid[m][:];   resid[m][:] = t;   t += bias;
//   y[m][:] = gamma ? t * rsqrt(mean(t^2) + eps) * gamma : t
// One 1024-thread workgroup per row (a thread owns 4 columns per 4096; every slab load of the row is in flight at
// once: the slabs were just written by other XCDs, so each load is a full memory round trip).  N <= 8192, N % 4 == 0.
// With xq != null the normalised row is ALSO quantised per token to e4m3 (scale amax/448 -> xscale[m]; the arithmetic of
// quantize_rows_fp8_kernel on the fp16-rounded values), the input format of the next fp8 projection.
static __global__ __launch_bounds__(1024) void splitk_rownorm_kernel(const float *__restrict__ slab, int KS, int M, int N,
                                                                     const SlabScale wscale,
                                                                     const half_t *__restrict__ bias, half_t *resid,
                                                                     const half_t *__restrict__ gamma, float eps, half_t *y,
                                                                     uint8_t *xq, float *xscale) {
    __shared__ float red[16];
    const int m = blockIdx.x, tid = threadIdx.x;
    const size_t slab_sz = static_cast<size_t>(M) * N;
    constexpr int NC = 2;
    floatx4 v[NC];
    half4_t r4[NC];
    int col[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        col[i] = (i * 1024 + tid) * 4;
        v[i] = floatx4{0.f, 0.f, 0.f, 0.f};
        if (col[i] < N) r4[i] = *reinterpret_cast<const half4_t *>(resid + static_cast<size_t>(m) * N + col[i]);
    }
    for (int k0 = 0; k0 < KS; k0 += 8) {
        floatx4 t[8][NC];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
#pragma unroll
            for (int i = 0; i < NC; ++i)
                if (col[i] < N)
                    t[kk][i] = *reinterpret_cast<const floatx4 *>(slab + static_cast<size_t>(min(k0 + kk, KS - 1)) * slab_sz +
                                                                  static_cast<size_t>(m) * N + col[i]);
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
            if (k0 + kk < KS) {
#pragma unroll
                for (int i = 0; i < NC; ++i) v[i] += t[kk][i];
            }
    }
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        if (col[i] < N) {
            const int c = col[i];
            half4_t o4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float t = wscale.apply(v[i][e], m, c + e);
                // same roundings as the unfused sequence: projection output -> fp16, residual sum -> fp16
                t = to_f32(from_f32<half_t>(t)) + to_f32(r4[i][e]);
                o4[e] = from_f32<half_t>(t);
                t = to_f32(o4[e]);
                if (bias) t += to_f32(bias[c + e]);
                v[i][e] = t;
                ss = fmaf(t, t, ss);
            }
            *reinterpret_cast<half4_t *>(resid + static_cast<size_t>(m) * N + c) = o4;
        }
    }
    float inv = 1.f;
    if (gamma) inv = rsqrtf(block_sum<16>(ss, red) / static_cast<float>(N) + eps);
    half4_t o4[NC];
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        if (col[i] < N) {
            const int c = col[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o4[i][e] = from_f32<half_t>(gamma ? v[i][e] * inv * to_f32(gamma[c + e]) : v[i][e]);
                amax = fmaxf(amax, fabsf(to_f32(o4[i][e])));
            }
            if (y) *reinterpret_cast<half4_t *>(y + static_cast<size_t>(m) * N + c) = o4[i];
        }
    }
    if (xq) {
        amax = block_max<16>(amax, red);
        const float sc = amax > 0.f ? amax / 448.0f : 1.0f;
        if (tid == 0) xscale[m] = sc;
#pragma unroll
        for (int i = 0; i < NC; ++i)
            if (col[i] < N)
                *reinterpret_cast<unsigned int *>(xq + static_cast<size_t>(m) * N + col[i]) =
                    pack4_e4m3(to_f32(o4[i][0]) / sc, to_f32(o4[i][1]) / sc, to_f32(o4[i][2]) / sc, to_f32(o4[i][3]) / sc);
    }
}

bool splitk_rownorm_eligible(int N) { return N % 4 == 0 && N <= 8192; }

int splitk_rownorm(const SplitKSlabs &sk, const SlabScale &wscale, const half_t *bias, half_t *resid, const half_t *gamma,
                   float eps, half_t *y, uint8_t *xq, float *xscale, hipStream_t st) {
    if (!splitk_rownorm_eligible(sk.N)) {
        set_error("splitk_rownorm: N=%d not supported", sk.N);
        return LLMIE_ERR_UNSUPPORTED;
    }
    splitk_rownorm_kernel<<<sk.M, 1024, 0, st>>>(sk.slab, sk.KS, sk.M, sk.N, wscale, bias, resid, gamma, eps, y, xq, xscale);
    return launch_status("splitk_rownorm");
}

// does the GEMV family take (M, K)?
bool gemv_f16_eligible(int M, int K, const void *x, const void *W) {
    return (mis16(x) | mis16(W)) == 0 && gemv_f16_route(M, K) != LR_REFUSED;
}

// ---- the 256-row tiled GEMM family: gemm8p.cuh (eight-phase; 32-bit DMA offsets) and gemm256.cuh (two-stage, any size); fp16
// operands, e4m3 operands with per-token / per-row scales, or int8 weights under fp16 activations.  One tile planner (pure host code:
// no HIP call, no error text), one launcher; llmie_gemm256_tiles reports the plan, tests/test_gemm256_tiles_cpu.py pins it.
//
// Tile plan by rounds of the CUs (one 512-thread workgroup per CU): a narrow tile costs ~0.6 of a wide one (measured: 0.96 vs 1.12
// PFLOP/s on full rounds of 256 x 128 against 256 x 256 tiles).  A half-empty last round of wide tiles (qkv at 2048 tokens: 384
// tiles = 1.5 rounds) is avoided by running the whole rounds wide and the left-over columns narrow in a second launch, when that is
// cheaper (SwiGLU at 4096 tokens: 1376 tiles = 5.4 rounds; not at 2048 tokens: 2.7 rounds would become 2 + 2 x 0.6).
constexpr int kG256Cus = 256;             // workgroups of one round
constexpr float kG256NarrowCost = 0.6f;   // a narrow tile, in wide tiles
constexpr int kG256FillWide = 192;        // wide tiles from which a grid fills the chip
// Narrow tiles that fill it = wide tiles from which the rounds decide: HALF the chip (round 3: at 1024 tokens the O / down projections,
// N = 4096: 128 tiles, used to fall to the 128 x 128 kernel -- 80 / 181 us against 58 / 140 us; 1 x 1024 prefill 57.7k -> 65.5k tok/s)
constexpr int kG256FillNarrow = 128;
static int g256_row_tiles(int M) { return (M + 255) / 256; }
static int g256_rounds(int tiles) { return (tiles + kG256Cus - 1) / kG256Cus; }
static int g256_ceil(int n, int w) { return (n + w - 1) / w; }

struct G256Rules {
    int wide, narrow;    // widths of the form's column tiles, in output columns
    bool whole_tiles;    // the output is a whole number of narrow tiles and no tile straddles its end (else: the last tile is ragged)
    int align;           // output columns % align == 0 lets the rounds decide and permits a split
    int gate;            // wide tiles below which the rounds do not decide (the fill gate)
    bool narrow_alone;   // the form runs all-narrow grids
    bool tie_narrow;     // all-wide and all-narrow cost the same: narrow (else wide)
};
static const G256Rules &g256_rules(G256Form form) {
    static const G256Rules rules[] = {
        // plain: 256 / 128 wide; ragged last tile; the epilogue stores 4 columns at a time (768 x 12288 is ONE round of 144 wide tiles
        // or TWO of 288 narrow ones -- 97 against 119 us: from half the chip on, the rounds decide)
        {256, 128, false, 4, kG256FillNarrow, true, false},
        // SwiGLU: 128 / 64 columns of the [M, I] output (256 / 128 weight rows); the 64-wide kernel only takes left-over columns; no gate
        // (callers come with gemm256_swiglu_fills)
        {128, 64, false, 4, 0, false, false},
        // QKV + RoPE: the ROPE forms fetch their weight rows unclamped, in permuted order, so every range is whole tiles: N % 128 == 0
        // always, all-wide only where N % 256 == 0; starts from all-narrow, so ties stay narrow
        {256, 128, true, 128, kG256FillNarrow, true, true},
    };
    return rules[form];
}

bool gemm256_fills(int M, int N) {
    const int tm = g256_row_tiles(M);
    return tm * g256_ceil(N, 256) >= kG256FillWide || tm * g256_ceil(N, 128) >= kG256FillNarrow;
}
// SwiGLU form: W = fused gate_up [2I, K], y = silu(x.Wg^T) * (x.Wu^T) [M, I]
bool gemm256_swiglu_fills(int M, int two_inter) {
    return two_inter % 8 == 0 && g256_row_tiles(M) * g256_ceil(two_inter / 2, 128) >= kG256FillWide;
}
int gemm256_narrow_rounds(int M, int N) { return g256_rounds(g256_row_tiles(M) * g256_ceil(N, 128)); }
bool gemm8p_fits(int N, int K, int elem_bytes) { return (static_cast<size_t>(N) + 512) * K * elem_bytes < (size_t{1} << 32); }

G256Plan plan_gemm256(G256Form form, G256Operands ops, int M, int N, int K) {
    const G256Rules &r = g256_rules(form);
    const int cols = form == G256_SWIGLU ? N / 2 : N, tm = g256_row_tiles(M);
    auto tiles_of = [&](int n, int w) { return r.whole_tiles ? n / w : g256_ceil(n, w); };
    const int tn_wide = tiles_of(cols, r.wide), tn_narrow = tiles_of(cols, r.narrow);
    // bytes per element of the fit: int8 weights count 2 like the fp16 activations beside them
    const int fit_bytes = ops == G256_E4M3 ? 1 : 2;
    G256Plan p{1, {{true, r.wide, 0, tn_wide}, {}}};
    // SwiGLU decides the family on the whole matrix, before the ranges: the two-stage kernel has no 64-wide form.  (int8 weights have
    // no two-stage form at all: plan_linear_wq routes them here only where the offsets fit)
    if (form == G256_SWIGLU && !gemm8p_fits(N, K, fit_bytes)) {
        p.range[0].eight_phase = false;
        return p;
    }
    if (cols % r.align != 0 || tm * tn_wide < r.gate) {
        if (r.narrow_alone && tm * tn_wide < kG256FillWide) p.range[0] = {true, r.narrow, 0, tn_narrow};
    } else {
        constexpr float never = 1e30f;
        const bool wide_ok = !r.whole_tiles || cols % r.wide == 0;
        const float c_wide = wide_ok ? static_cast<float>(g256_rounds(tm * tn_wide)) : never;
        const float c_narrow = r.narrow_alone ? g256_rounds(tm * tn_narrow) * kG256NarrowCost : never;
        const bool narrow = r.tie_narrow ? !(c_wide < c_narrow) : c_narrow < c_wide;
        if (narrow) p.range[0] = {true, r.narrow, 0, tn_narrow};
        const int a = (tm * tn_wide / kG256Cus) * kG256Cus / tm;   // wide column tiles that make whole rounds
        if (a > 0 && a * r.wide < cols) {
            const int b = tiles_of(cols - a * r.wide, r.narrow);
            const float c = static_cast<float>(g256_rounds(tm * a)) + g256_rounds(tm * b) * kG256NarrowCost;
            if (c < (narrow ? c_narrow : c_wide)) p = G256Plan{2, {{true, r.wide, 0, a}, {true, r.narrow, a * r.wide, b}}};
        }
    }
    // plain: each range by its own size (its W pointer is advanced to the range); int8 weights never leave the eight-phase kernels
    // (plan_linear_wq checks the whole matrix).  QKV + RoPE: gemm256_qkv_rope_eligible checks the whole matrix.
    if (form == G256_PLAIN && ops != G256_W8)
        for (int i = 0; i < p.ranges; ++i) {
            G256Range &g = p.range[i];
            g.eight_phase = gemm8p_fits(std::min(g.tiles * g.width, N - g.col0), K, fit_bytes);
        }
    return p;
}

// "8p 256x32@0 128x2@8192": family (8p eight-phase, 2s two-stage; again before a range that changes it), then WIDTHxTILES@FIRSTCOL
static void g256_plan_text(const G256Plan &p, char *buf, size_t size) {
    size_t len = 0;
    for (int i = 0; i < p.ranges && len < size; ++i) {
        const G256Range &g = p.range[i];
        if (i == 0 || g.eight_phase != p.range[i - 1].eight_phase)
            len += snprintf(buf + len, size - len, "%s%s", i ? " " : "", g.eight_phase ? "8p" : "2s");
        if (len < size) len += snprintf(buf + len, size - len, " %dx%d@%d", g.width, g.tiles, g.col0);
    }
}

// One launch: the dynamic-LDS attribute is set once per instantiation and process (function-local static initialisation: thread-safe)
struct G256Args {
    const void *x, *W;
    half_t *y;
    int M, N, K;
    const half_t *bias, *residual;
    int tiles_n;
    const float *xscale, *wscale;
    int ldc, col0;
    const QkvRopeArgs *rap;
    int layer;
};
template <auto Kernel, int LDS_BYTES, bool EIGHT_PHASE> static void g256_run(const G256Args &a, int grid, hipStream_t st) {
    static const bool attr_set = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
        return true;
    }();
    (void)attr_set;
    constexpr int group_m = 4;   // XCD-aware tile order: row tiles per group
    if constexpr (EIGHT_PHASE)
        Kernel<<<grid, 512, LDS_BYTES, st>>>(a.x, a.W, a.y, a.M, a.N, a.K, a.bias, a.residual, a.tiles_n, a.xscale, a.wscale, a.ldc, group_m,
                                             a.col0, a.rap, a.layer);
    else
        Kernel<<<grid, 512, LDS_BYTES, st>>>(a.x, a.W, a.y, a.M, a.N, a.K, a.bias, a.residual, a.tiles_n, a.xscale, a.wscale, a.ldc, group_m);
}
// (family, width) -> instantiation, for one form, operand format and epilogue
template <G256Form FORM, bool FP8, int WQ, bool EPI> static void g256_run_range(const G256Range &g, const G256Args &a, int grid, hipStream_t st) {
    constexpr bool SWIGLU = FORM == G256_SWIGLU, ROPE = FORM == G256_QKV_ROPE;
    constexpr int stage_bytes = 2 * 4 * 128 * 128, stage_bytes_narrow = 2 * 3 * 128 * 128, ring_bytes = 9 * 128 * 128;
    const bool wide = g.width == (SWIGLU ? 128 : 256);
    if (g.eight_phase) {
        if (wide) g256_run<gemm8p_kernel<FP8, EPI, SWIGLU, WQ, ROPE>, stage_bytes, true>(a, grid, st);
        else g256_run<gemm8p_n128_kernel<FP8, EPI, SWIGLU, WQ, ROPE>, ring_bytes, true>(a, grid, st);
    } else if constexpr (!ROPE) {   // (the two-stage kernel reads W as the activations' format: never planned for int8 weights)
        if (wide) g256_run<gemm256_kernel<FP8, EPI, 4, SWIGLU>, stage_bytes, false>(a, grid, st);
        else if constexpr (!SWIGLU) g256_run<gemm256_kernel<FP8, EPI, 2>, stage_bytes_narrow, false>(a, grid, st);
    }
}
// plan, then one launch per column range
static void g256_launch(G256Form form, G256Operands ops, G256Args a, int N, hipStream_t st) {
    const G256Plan p = plan_gemm256(form, ops, a.M, N, a.K);
    const bool epi = a.bias || a.residual;
    const size_t w_elem = ops == G256_F16 ? 2 : 1;
    const G256Args whole = a;
    for (int i = 0; i < p.ranges; ++i) {
        const G256Range &g = p.range[i];
        a = whole;
        a.tiles_n = g.tiles;
        if (form == G256_SWIGLU) {   // operands whole, N = 2I: the kernel finds its gate / up rows and output columns from col0
            a.col0 = g.col0;
        } else {
            a.W = static_cast<const unsigned char *>(whole.W) + static_cast<size_t>(g.col0) * a.K * w_elem;
            a.N = std::min(g.tiles * g.width, N - g.col0);
            a.ldc = N;
        }
        if (form == G256_QKV_ROPE) {   // C, the scales and the bias stay whole: the epilogue indexes them by col0 + tile column
            a.col0 = g.col0;
        } else if (form == G256_PLAIN) {
            a.y += g.col0;
            if (a.bias) a.bias += g.col0;
            if (a.residual) a.residual += g.col0;
            // int8 weights: the row scales are fp16, carried through the float pointer of the kernels' shared signature
            if (a.wscale)
                a.wscale = ops == G256_W8 ? reinterpret_cast<const float *>(reinterpret_cast<const half_t *>(whole.wscale) + g.col0)
                                          : whole.wscale + g.col0;
        }
        const int grid = g256_row_tiles(a.M) * g.tiles;
        switch (form) {
            case G256_PLAIN:
                if (ops == G256_W8) epi ? g256_run_range<G256_PLAIN, false, 8, true>(g, a, grid, st) : g256_run_range<G256_PLAIN, false, 8, false>(g, a, grid, st);
                else if (ops == G256_E4M3) epi ? g256_run_range<G256_PLAIN, true, 0, true>(g, a, grid, st) : g256_run_range<G256_PLAIN, true, 0, false>(g, a, grid, st);
                else epi ? g256_run_range<G256_PLAIN, false, 0, true>(g, a, grid, st) : g256_run_range<G256_PLAIN, false, 0, false>(g, a, grid, st);
                break;
            case G256_SWIGLU:
                if (ops == G256_W8) g256_run_range<G256_SWIGLU, false, 8, false>(g, a, grid, st);
                else if (ops == G256_E4M3) g256_run_range<G256_SWIGLU, true, 0, false>(g, a, grid, st);
                else g256_run_range<G256_SWIGLU, false, 0, false>(g, a, grid, st);
                break;
            case G256_QKV_ROPE:
                if (ops == G256_W8) g256_run_range<G256_QKV_ROPE, false, 8, false>(g, a, grid, st);
                else if (ops == G256_E4M3) g256_run_range<G256_QKV_ROPE, true, 0, false>(g, a, grid, st);
                else g256_run_range<G256_QKV_ROPE, false, 0, false>(g, a, grid, st);
                break;
        }
    }
}

void gemm256_launch(G256Operands ops, const void *x, const void *W, half_t *y, int M, int N, int K, const half_t *bias,
                    const half_t *residual, const float *xscale, const float *wscale, hipStream_t st) {
    g256_launch(G256_PLAIN, ops, G256Args{x, W, y, M, N, K, bias, residual, 0, xscale, wscale, 0, 0, nullptr, 0}, N, st);
}
void gemm256_swiglu_launch(G256Operands ops, const void *x, const void *W, half_t *y, int M, int two_inter, int K, const float *xscale,
                           const float *wscale, hipStream_t st) {
    g256_launch(G256_SWIGLU, ops, G256Args{x, W, y, M, two_inter, K, nullptr, nullptr, 0, xscale, wscale, 0, 0, nullptr, 0}, two_inter, st);
}

// ---- QKV projection of a prefill with RoPE + KV-cache append as its epilogue (gemm8p.cuh ROPE forms; context_attention.cpp:158-205
// as one launch sequence).  N = (head_num + 2 kv_head_num) * 128.
bool gemm256_qkv_rope_eligible(G256Operands ops, int M, int N, int K, const void *x, const void *W, const void *wscale, const void *qkv) {
    const bool fp8 = ops == G256_E4M3;
    return N % 128 == 0 && K % (fp8 ? 128 : 64) == 0 && gemm256_fills(M, N) && gemm8p_fits(N, K, fp8 ? 1 : 2) &&
           (reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(W)) % 16 == 0 &&
           (reinterpret_cast<uintptr_t>(wscale) % (fp8 ? 16 : 8)) == 0 && reinterpret_cast<uintptr_t>(qkv) % 8 == 0;
}
// rap: DEVICE pointer (prefill_token_table); bias: this layer's QKV bias or null
void gemm256_qkv_rope_launch(G256Operands ops, const void *x, const void *W, half_t *qkv, int M, int N, int K, const float *xscale,
                             const float *wscale, const half_t *bias, const QkvRopeArgs *rap, int layer, hipStream_t st) {
    g256_launch(G256_QKV_ROPE, ops, G256Args{x, W, qkv, M, N, K, bias, nullptr, 0, xscale, wscale, 0, 0, rap, layer}, N, st);
}

// ---- route planning: which kernel a projection runs on.  Pure host code: no HIP call, no error text, no launch. ----
LinearCall linear_call(int bits, const LinearOperands &o, const LinearScratch &s) {
    return LinearCall{bits, o.M, o.K, o.N, o.epi, o.group, o.bias != nullptr, o.residual != nullptr, o.gamma != nullptr, o.pre_bias != nullptr,
                      mis16(o.x), mis16(o.w), mis16(o.y), mis16(o.bias), mis16(o.residual), mis16(o.gamma), mis16(o.pre_bias), mis16(o.scale),
                      mis16(s.image), s.slabs.p != nullptr, s.slabs.p ? s.slabs.floats : 0, s.image != nullptr, s.image ? s.image_bytes : 0,
                      s.act != nullptr, s.act ? s.act_bytes : 0, static_cast<unsigned>(reinterpret_cast<uintptr_t>(s.act) % 256)};
}
LinearCall linear_call_sizing(int bits, int M, int K, int N, int epi, int group) {
    LinearCall c{};
    c.bits = bits, c.M = M, c.K = K, c.N = N, c.epi = epi, c.group = group;
    c.slabs = c.image = c.act = true;
    c.slab_floats = c.image_bytes = c.act_bytes = ~static_cast<size_t>(0);
    return c;
}

static LinearPlan planned(int route) { return LinearPlan{route, LREF_NONE, 0, 0, 0, LR_REFUSED}; }
static LinearPlan refused(int why) { return LinearPlan{LR_REFUSED, why, 0, 0, 0, LR_REFUSED}; }
// a split-K route in passes of `pass` rows over the caller's slabs (sized for the first pass, the largest)
static LinearPlan planned_splitk(const LinearCall &c, int route, int pass) {
    LinearPlan p = planned(route);
    p.pass_rows = pass;
    p.slab_floats = linear_splitk_ws_floats(c.bits, c.M < pass ? c.M : pass, c.K, c.N);
    if (c.slab_floats < p.slab_floats) p.route = LR_REFUSED, p.refusal = LREF_SLABS;
    return p;
}

LinearPlan plan_linear_f16(const LinearCall &c) {
    const int M = c.M, K = c.K, N = c.N;
    const bool swiglu = c.epi == EPI_SWIGLU;
    const bool aligned = K % 8 == 0 && (c.mis_x | c.mis_w) == 0;
    const bool epi8 = (c.mis_bias | c.mis_residual) % 8 == 0;
    // a fused norm rides on the GEMV routes only
    if (c.gamma || c.pre_bias)
        return aligned && c.gamma && (c.mis_gamma | c.mis_pre_bias) == 0 && gemv_f16_route(M, K) != LR_REFUSED ? planned(gemv_f16_route(M, K))
                                                                                                                 : refused(LREF_F16_NORM);
    if (aligned && gemv_f16_route(M, K) != LR_REFUSED) return planned(gemv_f16_route(M, K));
    // decode / short-prefill batches: split-K over the caller's slabs (without a workspace: the non-split kernels below).
    // Round 3, 192 < M where the eight-phase kernels' 256-row grid does not fill the chip (N = 4096 at 256-1023 tokens): such
    // shapes used to fall to the 128 x 128 kernel -- 82 us for the O and 190 us for the down projection of a 7B layer WHATEVER the
    // row count.  Two cheaper forms, picked by a two-term time model fitted to the measurements (tools/dev/s2_run18.sh sweep):
    //   split-K passes of 128 rows:  passes x (weight bytes / 4.2 TB/s + 10 us)          O: 19.5 us per pass, down: 30 us
    //   256 x 128 eight-phase tiles: rounds of 256 tiles x K / 64 k-tiles x 0.9 us        O: 58 us, down: 140 us per round
    bool mid_rows = false, mid_tiles = false;
    if (M > 192 && !swiglu && aligned && K % 64 == 0 && !gemm256_fills(M, N)) {
        const int passes = (M + kSplitKPassRows - 1) / kSplitKPassRows;
        const float t_split = passes * (static_cast<float>(N) * K * 2.f / 4.2e6f + 10.f);
        const float t_tiles = static_cast<float>(gemm256_narrow_rounds(M, N)) * (K / 64) * 0.9f;
        const bool split_ok = c.slabs && K % 128 == 0 && K >= 512 && c.slab_floats >= linear_splitk_ws_floats(16, kSplitKPassRows, K, N);
        const bool tiles_ok = gemm8p_fits(N, K, 2) && c.mis_y % 8 == 0 && epi8;
        mid_rows = split_ok && (!tiles_ok || t_split < t_tiles);
        mid_tiles = tiles_ok && !mid_rows;
    }
    if (c.slabs && aligned && (M <= 192 || mid_rows) && K % 128 == 0 && K >= 512)
        return planned_splitk(c, mid_rows ? LR_SPLITK_PASSES : LR_SPLITK, kSplitKPassRows);
    if (aligned && M <= 64 && K % 32 == 0 && (!swiglu || (N / 2) % 16 == 0)) return planned(LR_SKINNY);
    if (swiglu)
        return aligned && K % 64 == 0 && gemm256_swiglu_fills(M, N) && c.mis_y % 8 == 0 ? planned(LR_SWIGLU256) : refused(LREF_F16_SWIGLU);
    if (aligned && K % 64 == 0 && c.mis_y % 8 == 0) {
        // 256 x 256 LDS-DMA kernel when its grid fills the chip (one 512-thread workgroup per CU); else 128 x 128 tiles
        if ((gemm256_fills(M, N) || mid_tiles) && epi8) return planned(gemm256_fills(M, N) ? LR_TILES256 : LR_TILES256_PART);
        return planned(LR_TILES128);
    }
    return planned(LR_GENERIC);
}

// Slab floats to reserve for an fp16 projection of M rows: the plan's, and those of the shape's split-K form where the plan needs
// none because M <= 8 runs the GEMV, or because a partly filled tile grid beats the passes in the time model.  (More than the plan
// needs: callers share one workspace across row counts, and the reservation has always been this.)
size_t linear_f16_reserve_slab_floats(int M, int K, int N) {
    const LinearPlan p = plan_linear_f16(linear_call_sizing(16, M, K, N, EPI_NONE));
    if (p.route == LR_GEMV_KSPLIT || p.route == LR_GEMV_LDS || p.route == LR_TILES256_PART) return linear_splitk_ws_floats(16, M, K, N);
    return p.slab_floats;
}

// the fp16 GEMM on the image of quantised weights: the same call with W = the image and no slabs
static LinearPlan planned_image(const LinearCall &c, int route) {
    LinearCall f = c;
    f.bits = 16, f.mis_w = c.mis_image, f.slabs = false, f.slab_floats = 0;
    const LinearPlan in = plan_linear_f16(f);
    if (in.route == LR_REFUSED) return in;
    LinearPlan p = planned(route);
    p.image_bytes = static_cast<size_t>(c.N) * c.K * sizeof(half_t);
    p.inner = in.route;
    return p;
}

// MXFP4 weights (mxfp4_linear.hip): e2m1 codes [N, K/2] + one e8m0 byte per 32 k.  Plain epilogue only; no route needs slabs (the
// MFMA kernel splits K over the waves of a workgroup), the image route needs room for the whole fp16 matrix.
static LinearPlan plan_linear_mxfp4(const LinearCall &c) {
    const int M = c.M;
    if (c.K % 32 != 0 || (c.mis_x | c.mis_w) != 0) return refused(LREF_MX4_SHAPE);
    if (c.epi != EPI_NONE || c.gamma || c.pre_bias) return refused(LREF_MX4_EPI);
    if (M <= kMx4GemvRows) return planned(LR_MX4_GEMV);
    if (M <= kMx4MfmaRows) return planned(LR_MX4_MFMA);
    if (M >= kWqPrefillRows && c.image && c.mis_image == 0 && c.image_bytes >= static_cast<size_t>(c.N) * c.K * sizeof(half_t)) {
        const LinearPlan p = planned_image(c, LR_WQ_IMAGE_PREFILL);
        if (p.route != LR_REFUSED) return p;
    }
    LinearPlan p = planned(LR_MX4_CHUNKS);
    p.pass_rows = kMx4MfmaRows;
    return p;
}

LinearPlan plan_linear_wq(const LinearCall &c) {
    if (c.bits == WF_MXFP4) return plan_linear_mxfp4(c);
    const int bits = c.bits, M = c.M, K = c.K, N = c.N;
    const bool swiglu = c.epi == EPI_SWIGLU, plain = c.epi == EPI_NONE;
    const bool aligned = (c.mis_x | c.mis_w | c.mis_gamma | c.mis_pre_bias) == 0 && (static_cast<size_t>(K) * bits / 8) % 16 == 0;
    // int8 [N, K] weights through the eight-phase kernels (gemm8p.cuh, WQ = 8): prefill-sized M whose 256-row grid fills the chip
    // (the fit counts 2 bytes per element although int8 weights are 1: kept, it is where these routes have always ended)
    const bool g8p_operands = bits == 8 && K % 64 == 0 && gemm8p_fits(N, K, 2) &&
                              (c.mis_x | c.mis_w) == 0 && (c.mis_scale | c.mis_y) % 8 == 0;
    const bool g8p = g8p_operands && N % 4 == 0 && gemm256_fills(M, N);
    const bool g8p_swiglu = g8p_operands && N % 8 == 0 && gemm256_swiglu_fills(M, N);
    const bool splitk_shape = aligned && K % 256 == 0 && K >= 512 && c.slabs;
    const bool image_ok = c.image && K % 8 == 0 && c.image_bytes >= static_cast<size_t>(N) * K * sizeof(half_t) && c.mis_image == 0 &&
                          c.mis_w % 8 == 0 && (bits == 8 || (c.group % 8 == 0 && K % c.group == 0));
    // ---- prefill-sized row counts: MFMA-bound, the weights are read M / 256 times from L2 instead of streamed once ----
    // (round 3) int8, M from 192, shapes whose 256-row grid does not fill the chip (N = 4096 of a 7B layer at 193 .. 1023 tokens):
    // split-K passes of 128 rows on the int8 rows against the fp16 image + a partly filled tile grid, by a time model fitted to the
    // sweep (us; O / down of a 7B layer: 22 / 33 per pass against 56 / 123 for the image route whatever the row count):
    //   passes x (N K bytes / 2.8 TB/s + 16)   <   N K x 3 bytes / 4 TB/s  +  K / 64 x 0.55
    bool int8_mid_passes = false;
    if (bits == 8 && M >= kWqPrefillRows && !c.gamma && plain && splitk_shape && !g8p &&
        c.slab_floats >= linear_splitk_ws_floats(8, kSplitKPassRows, K, N)) {
        const float nk = static_cast<float>(N) * K;
        const float t_passes = ((M + 127) / 128) * (nk / 2.8e6f + 16.f), t_image = nk * 3.f / 4.0e6f + (K / 64) * 0.55f;
        int8_mid_passes = t_passes * 1.05f < t_image;   // (ties go to the image route)
    }
    if (M >= kWqPrefillRows && !c.gamma && !int8_mid_passes) {
        // int8: the eight-phase GEMM takes the int8 rows as they are (raw bytes HBM -> LDS by DMA, de-quantised at fragment read,
        // scale in the epilogue)
        if (swiglu && !c.bias && !c.residual && g8p_swiglu) return planned(LR_W8_G8P_SWIGLU);
        if (plain && g8p && (c.mis_bias | c.mis_residual) % 8 == 0) return planned(LR_W8_G8P);
        // other shapes, and int4 (group scales along K): one pass writes the fp16 image of the matrix into the caller's scratch,
        // the fp16 GEMM reads it back (mostly from the 256 MiB Infinity Cache): + (bits / 8 + 2) bytes of traffic per weight
        // (the fp16 GEMM has no fused SwiGLU where its 256-row grid does not fill: the forms below)
        if (image_ok && (!swiglu || gemm256_swiglu_fills(M, N))) return planned_image(c, LR_WQ_IMAGE_PREFILL);
    }
    if (aligned && ksplit_eligible(M, K, bits)) return planned(LR_WQ_GEMV);
    if (bits == 4 && c.group == 128 && splitk_shape && M > 8 && !c.gamma) {   // MFMA path, group scales in the kernel
        if (c.mis_scale % 4) return refused(LREF_W4_SPLITK);
        return planned_splitk(c, LR_W4_SPLITK, 64);
    }
    if (aligned && bits == 4) {
        // other int4 shapes: batches beyond the GEMV's register budget run as row chunks of the largest eligible
        // size (the weights are streamed once per chunk -- correct for any batch, bandwidth-efficient only for small ones)
        int mc = 8;
        while (mc > 0 && !ksplit_eligible(mc, K, 4)) --mc;
        if (mc > 0) {
            LinearPlan p = planned(LR_W4_CHUNKS);
            p.pass_rows = mc;
            return p;
        }
    }
    if (c.gamma) return refused(LREF_WQ_NORM);
    if (bits == 8 && splitk_shape) return planned_splitk(c, int8_mid_passes ? LR_W8_SPLITK_PASSES : LR_W8_SPLITK, kSplitKPassRows);
    if (!plain) return refused(LREF_WQ_SWIGLU);
    if (bits == 8 && aligned && K % 64 == 0 && M <= 64) return planned(LR_W8_SKINNY);
    // shapes none of the quantised kernels take (K not a multiple of their sub-blocks): the fp16 image, where the caller gave room
    if (image_ok) return planned_image(c, LR_WQ_IMAGE_LAST);
    return refused(LREF_WQ_SHAPE);
}

// e4m3 weights x per-token e4m3 activations (fp8_linear.hip): the GEMV (M <= 8, K within its register budget; the only route with a
// fused norm or SwiGLU), the 256-row tiled GEMM on the quantised activations, or split-K passes of 128 rows over the caller's slabs.
LinearPlan plan_linear_fp8(const LinearCall &c) {
    const int M = c.M, K = c.K, N = c.N;
    const bool gemv = M <= 8 && ksplit_eligible(M, K, 8) && c.mis_x == 0;
    if (c.gamma || c.pre_bias || c.epi != EPI_NONE)
        return gemv && c.mis_w == 0 && (!c.gamma || (c.mis_gamma | c.mis_pre_bias) == 0) ? planned(LR_FP8_GEMV) : refused(LREF_FP8_GEMV);
    bool tiled = M > 8 && K % 128 == 0 && N % 4 == 0 && c.mis_scale == 0 && (c.mis_bias | c.mis_residual) % 8 == 0;
    if (tiled && !gemm256_fills(M, N)) {
        // (round 3) a grid that does not fill the chip against split-K passes of 128 rows, by the time model fitted to the sweep
        // (tools/dev/s2_run27.sh; us): O / down of a 7B layer 41 / 90 tiled at any row count, 18.9 / 22.3 per pass -- at 768 tokens
        // the six passes took 113 / 134 us
        tiled = M > 128 && gemm8p_fits(N, K, 1);
        if (tiled) {
            const float t_tiles = static_cast<float>(gemm256_narrow_rounds(M, N)) * (K / 128) * 1.15f;
            const float t_passes = ((M + 127) / 128) * (static_cast<float>(N) * K / 8.3e6f + 17.f);
            tiled = t_tiles < t_passes;
        }
    }
    if ((!tiled && (K % 256 != 0 || K < 512)) || c.mis_w != 0 || c.mis_act != 0) return refused(LREF_FP8_SHAPE);
    if (c.act_bytes < fp8_act_bytes(M, K)) return refused(LREF_FP8_ACT);
    if (gemv) return planned(LR_FP8_GEMV);
    // prefill-sized: MFMA-bound tiled GEMM on v_mfma_scale_f32_16x16x128_f8f6f4
    if (tiled) return planned(LR_FP8_GEMM256);
    return planned_splitk(c, LR_FP8_SPLITK, kSplitKPassRows);
}

// fp16 scratch to reserve beside the slabs for an int8 / int4 projection of M rows.  From kWqPrefillRows rows on: room for the whole
// image, also where the plan needs none (the int8 eight-phase and split-K routes) -- more than the plan needs, kept: callers share
// one workspace across shapes.  Below: int8 reserves what the plan needs (the last-resort image of shapes no int8 kernel takes);
// int4 has never reserved any there.
size_t linear_wq_dequant_bytes(int wbits, int M, int K, int N) {
    if (wbits == WF_MXFP4) return K % 32 == 0 && M >= kWqPrefillRows ? static_cast<size_t>(N) * K * sizeof(half_t) : 0;
    if ((wbits != 8 && wbits != 4) || K % 8 != 0) return 0;
    if (M >= kWqPrefillRows) return static_cast<size_t>(N) * K * sizeof(half_t);
    return wbits == 8 ? plan_linear_wq(linear_call_sizing(8, M, K, N, EPI_NONE)).image_bytes : 0;
}
WqWorkspace wq_workspace(int wbits, int M, int K, int N, void *workspace, size_t workspace_bytes) {
    const size_t dq = (linear_wq_dequant_bytes(wbits, M, K, N) + 255) & ~static_cast<size_t>(255);
    if (workspace && dq && workspace_bytes >= dq) {
        char *b = static_cast<char *>(workspace);
        return WqWorkspace{b, dq, SlabWs{reinterpret_cast<float *>(b + dq), (workspace_bytes - dq) / sizeof(float)}};
    }
    return WqWorkspace{nullptr, 0, SlabWs{static_cast<float *>(workspace), workspace_bytes / sizeof(float)}};
}

const char *linear_route_name(int route) {
    static const char *const names[] = {"refused", "gemv_ksplit", "gemv_lds", "splitk", "splitk_passes", "skinny", "swiglu256", "tiles256",
                                        "tiles256_part", "tiles128", "generic", "g8p", "g8p_swiglu", "int8_splitk_passes", "image_prefill",
                                        "image_last", "gemv_ksplit", "int4_splitk", "int4_chunks", "int8_splitk", "int8_skinny", "mxfp4_gemv",
                                        "mxfp4_mfma", "mxfp4_chunks", "fp8_gemv", "fp8_gemm256", "fp8_splitk"};
    return names[route];
}

int linear_refuse(const LinearCall &c, const LinearPlan &p) {
    const int M = c.M, K = c.K, N = c.N;
    switch (p.refusal) {
        case LREF_F16_SWIGLU:
            set_error("linear: fused SwiGLU epilogue without a split-K workspace needs M<=64, K%%32==0, (N/2)%%16==0 (M=%d K=%d N=%d)", M, K, N);
            return LLMIE_ERR_UNSUPPORTED;
        case LREF_SLABS:
            set_error("linear(split-K): slab workspace too small or misaligned (%zu < %zu bytes); size it with "
                      "llmie_linear_workspace_bytes()", c.slab_floats * sizeof(float), p.slab_floats * sizeof(float));
            return LLMIE_ERR_WORKSPACE;
        case LREF_W4_SPLITK:
            set_error("linear(split-K int4): needs M <= 64 per pass, K %% 256 == 0, group-128 scales");
            return LLMIE_ERR_UNSUPPORTED;
        case LREF_WQ_NORM:
            set_error("linear_wq: fused norm only on the GEMV path (M=%d K=%d bits=%d)", M, K, c.bits);
            return LLMIE_ERR_UNSUPPORTED;
        case LREF_WQ_SWIGLU:
            set_error("linear_wq: fused SwiGLU needs the GEMV or split-K path (M=%d K=%d bits=%d)", M, K, c.bits);
            return LLMIE_ERR_UNSUPPORTED;
        case LREF_MX4_SHAPE:
            set_error("linear_mxfp4: needs K %% 32 == 0 and 16-byte aligned x and wq (M=%d K=%d N=%d)", M, K, N);
            return LLMIE_ERR_UNSUPPORTED;
        case LREF_MX4_EPI:
            set_error("linear_mxfp4: plain epilogue (bias, residual) only: no fused norm or SwiGLU form (M=%d K=%d N=%d)", M, K, N);
            return LLMIE_ERR_UNSUPPORTED;
        case LREF_F16_NORM:
            set_error("linear(norm-fused): shape M=%d K=%d not on the GEMV path", M, K);
            return LLMIE_ERR_UNSUPPORTED;
        case LREF_FP8_SHAPE:
            set_error("linear_fp8: needs K %% 256 == 0, K >= 512 (K %% 128 == 0 for prefill-sized M x N), 16-byte aligned weights, "
                      "256-byte aligned workspace");
            return LLMIE_ERR_UNSUPPORTED;
        case LREF_FP8_ACT:
            set_error("linear_fp8: workspace too small (%zu < %zu bytes)", c.act_bytes, fp8_act_bytes(M, K));
            return LLMIE_ERR_WORKSPACE;
        case LREF_FP8_GEMV:
            set_error("linear_fp8: shape M=%d K=%d not on the GEMV path", M, K);
            return LLMIE_ERR_UNSUPPORTED;
        default:
            set_error("linear_wq: unsupported shape M=%d K=%d N=%d bits=%d without a split-K workspace (int8: M<=64, K%%64==0; int4: "
                      "M<=8 on the GEMV path); size one with llmie_linear_workspace_bytes()", M, K, N, c.bits);
            return LLMIE_ERR_UNSUPPORTED;
    }
}

int linear_f16_nk(const LinearOperands &o, const LinearScratch &s, hipStream_t st) {
    const LinearCall c = linear_call(16, o, s);
    const LinearPlan p = plan_linear_f16(c);
    const half_t *x = static_cast<const half_t *>(o.x), *W = static_cast<const half_t *>(o.w);
    const half_t *bias = static_cast<const half_t *>(o.bias), *residual = static_cast<const half_t *>(o.residual);
    half_t *y = static_cast<half_t *>(o.y);
    const int M = o.M, K = o.K, N = o.N, epi = o.epi;
    switch (p.route) {
        case LR_GEMV_KSPLIT:
        case LR_GEMV_LDS:
            if (o.gamma) {
                dispatch_gemv(M, GemvArgs{x, W, y, K, N, bias, residual, static_cast<const half_t *>(o.gamma), static_cast<const half_t *>(o.pre_bias),
                                          o.eps, epi, 1, nullptr, 0}, st);
                return launch_status("linear(norm-fused)");
            }
            dispatch_gemv(M, GemvArgs{x, W, y, K, N, bias, residual, nullptr, nullptr, 0.f, epi, 0, nullptr, 0}, st);
            return launch_status("linear");
        case LR_SPLITK:
        case LR_SPLITK_PASSES:
            return linear_splitk(16, o, s, st);
        case LR_SKINNY:
            if (epi == EPI_SWIGLU) dispatch_skinny<EPI_SWIGLU>(M, x, W, y, K, N, bias, residual, st);
            else dispatch_skinny<EPI_NONE>(M, x, W, y, K, N, bias, residual, st);
            return launch_status("linear");
        case LR_SWIGLU256:
            gemm256_swiglu_launch(G256_F16, x, W, y, M, N, K, nullptr, nullptr, st);
            return launch_status("linear(gemm256 SwiGLU)");
        case LR_TILES256:
        case LR_TILES256_PART:
            gemm256_launch(G256_F16, x, W, y, M, N, K, bias, residual, nullptr, nullptr, st);
            return launch_status("linear(gemm256)");
        case LR_TILES128: {
            dim3 grid((N + 127) / 128, (M + 127) / 128, 1);
            if (bias || residual)
                tiled_mfma_f16_kernel<true><<<grid, 256, 0, st>>>(x, W, y, M, N, K, 0, 0, 0, bias, residual);
            else
                tiled_mfma_f16_kernel<false><<<grid, 256, 0, st>>>(x, W, y, M, N, K, 0, 0, 0, nullptr, nullptr);
            return launch_status("linear");
        }
        case LR_GENERIC:
            launch_generic<half_t>(x, W, y, 1, M, N, K, true, bias, residual, st);
            return launch_status("linear");
        default:
            return linear_refuse(c, p);
    }
}

int linear_run(int bits, const LinearOperands &o, const LinearScratch &s, hipStream_t st) {
    switch (bits) {
        case 16: return linear_f16_nk(o, s, st);
        case 8:
        case 4: return linear_wq(bits, o, s, st);
        case WF_FP8: return linear_fp8(o, s, st);
        case WF_MXFP4: return linear_mxfp4(o, s, st);
        default: set_error("linear: weight format code %d not supported by this build", bits); return LLMIE_ERR_UNSUPPORTED;
    }
}

}  // namespace llmie

using namespace llmie;

// scratch of the projection entry points for this shape: [fp16 image of int8 / int4 weights | fp32 split-K slabs] (the counterpart of
// the workspace the reference's cublasWrapper owns)
extern "C" size_t llmie_linear_workspace_bytes(llmie_weight_format fmt, int M, int K, int N) {
    if (M <= 0 || K <= 0 || N <= 0) return 0;
    switch (fmt) {
        case LLMIE_W_F16: return linear_f16_reserve_slab_floats(M, K, N) * sizeof(float);
        case LLMIE_W_FP8: return linear_splitk_ws_floats(WF_FP8, M, K, N) * sizeof(float);
        case LLMIE_W_INT8:
        case LLMIE_W_INT4: {
            // the slabs of the shape's split-K form at every M, whatever route M takes (more than the eight-phase, image and GEMV
            // routes need, kept: callers share one workspace across row counts), behind the image (linear_wq_dequant_bytes)
            const int wbits = fmt == LLMIE_W_INT8 ? 8 : 4;
            const size_t dq = (linear_wq_dequant_bytes(wbits, M, K, N) + 255) & ~static_cast<size_t>(255);
            return dq + linear_splitk_ws_floats(wbits, M, K, N) * sizeof(float);
        }
        // MXFP4: the fp16 image from kWqPrefillRows rows on; no route takes slabs
        case LLMIE_W_MXFP4: return (linear_wq_dequant_bytes(WF_MXFP4, M, K, N) + 255) & ~static_cast<size_t>(255);
        default: return 0;
    }
}

static bool slab_ws_of(void *workspace, size_t bytes, SlabWs *out) {
    *out = SlabWs{static_cast<float *>(workspace), bytes / sizeof(float)};
    return !workspace || reinterpret_cast<uintptr_t>(workspace) % 16 == 0;
}

extern "C" int llmie_linear(const void *x, const void *w, void *y, int M, int K, int N, int trans_b,
                            const void *bias, const void *residual, llmie_dtype dtype, void *workspace,
                            size_t workspace_bytes, llmie_stream stream) {
    LLMIE_REQUIRE(x && w && y, "linear: NULL pointer");
    LLMIE_REQUIRE(M > 0 && K > 0 && N > 0, "linear: bad shape M=%d K=%d N=%d", M, K, N);
    SlabWs ws;
    LLMIE_REQUIRE(slab_ws_of(workspace, workspace_bytes, &ws), "linear: workspace must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    if (dtype == LLMIE_F16) {
        if (trans_b) return linear_f16_nk(LinearOperands{x, w, nullptr, y, M, K, N, EPI_NONE, 0, bias, residual}, LinearScratch{ws}, st);
        launch_generic<half_t>((const half_t *)x, (const half_t *)w, (half_t *)y, 1, M, N, K, false,
                               (const half_t *)bias, (const half_t *)residual, st);
        return launch_status("linear");
    }
    if (dtype == LLMIE_F32) {
        launch_generic<float>((const float *)x, (const float *)w, (float *)y, 1, M, N, K, trans_b != 0,
                              (const float *)bias, (const float *)residual, st);
        return launch_status("linear");
    }
    LLMIE_UNSUPPORTED("linear: dtype %d", (int)dtype);
}

extern "C" int llmie_linear_swiglu(const void *x, const void *w, void *y, int M, int K, int two_inter,
                                   llmie_dtype dtype, void *workspace, size_t workspace_bytes, llmie_stream stream) {
    LLMIE_REQUIRE(x && w && y, "linear_swiglu: NULL pointer");
    LLMIE_REQUIRE(M > 0 && K > 0 && two_inter > 0 && two_inter % 2 == 0, "linear_swiglu: bad shape");
    if (dtype != LLMIE_F16) LLMIE_UNSUPPORTED("linear_swiglu: fp16 only (dtype %d)", (int)dtype);
    SlabWs ws;
    LLMIE_REQUIRE(slab_ws_of(workspace, workspace_bytes, &ws), "linear_swiglu: workspace must be 16-byte aligned");
    return linear_f16_nk(LinearOperands{x, w, nullptr, y, M, K, two_inter, EPI_SWIGLU}, LinearScratch{ws}, as_stream(stream));
}

extern "C" const char *llmie_linear_route(llmie_weight_format fmt, const void *x, const void *w, const void *scale, const void *y, int M,
                                          int K, int N, int swiglu, int group, const void *bias, const void *residual,
                                          const void *workspace, size_t workspace_bytes) {
    const int bits = fmt == LLMIE_W_F16 ? 16 : (fmt == LLMIE_W_INT8 ? 8 : (fmt == LLMIE_W_INT4 ? 4 : (fmt == LLMIE_W_MXFP4 ? WF_MXFP4 : (fmt == LLMIE_W_FP8 ? WF_FP8 : 0))));
    const int epi = swiglu ? EPI_SWIGLU : EPI_NONE;
    static thread_local char name[48];
    auto fail = [](const char *what) -> const char * {
        set_error("linear_route: %s", what);
        return nullptr;
    };
    if (!bits) return fail("fp16, int8, int4, fp8 and MXFP4 weights only");
    if (!x || !w || !y || (bits != 16 && !scale)) return fail("NULL pointer");
    if (M <= 0 || K <= 0 || N <= 0 || (swiglu && (N % 2 || bias || residual))) return fail("bad shape or epilogue");
    if (bits == 4 && !(group > 0 && group % 32 == 0 && K % group == 0)) return fail("group must be a multiple of 32 dividing K");
    if (mis16(workspace)) return fail("workspace must be 16-byte aligned");
    void *wsp = const_cast<void *>(workspace);
    const LinearOperands o{x, w, bits == 16 ? nullptr : scale, const_cast<void *>(y), M, K, N, epi, bits == 4 ? group : 0, bias, residual};
    LinearScratch s{};
    if (bits == 16) {
        s.slabs = SlabWs{static_cast<float *>(wsp), workspace_bytes / sizeof(float)};
    } else if (bits == WF_FP8) {
        // as llmie_linear_fp8 splits its workspace: the activation part, which has to be there, then the slabs
        const size_t act = fp8_act_bytes(M, K);
        if (!wsp) return fail("fp8 weights need a workspace (llmie_linear_fp8_workspace_bytes)");
        if (workspace_bytes < act) return fail("fp8 workspace too small for the quantised activations (llmie_linear_fp8_workspace_bytes)");
        s = LinearScratch{SlabWs{reinterpret_cast<float *>(static_cast<char *>(wsp) + act), (workspace_bytes - act) / sizeof(float)}, nullptr, 0, wsp, act};
    } else {
        const WqWorkspace ws = wq_workspace(bits, M, K, N, wsp, workspace_bytes);
        s = LinearScratch{ws.slabs, ws.deq, ws.deq_bytes};
    }
    const LinearCall c = linear_call(bits, o, s);
    const LinearPlan p = bits == 16 ? plan_linear_f16(c) : (bits == WF_FP8 ? plan_linear_fp8(c) : plan_linear_wq(c));
    if (p.route == LR_REFUSED) {
        linear_refuse(c, p);
        return nullptr;
    }
    if (p.inner != LR_REFUSED) snprintf(name, sizeof(name), "%s+%s", linear_route_name(p.route), linear_route_name(p.inner));
    else snprintf(name, sizeof(name), "%s", linear_route_name(p.route));
    return name;
}

extern "C" const char *llmie_gemm256_tiles(int form, int operands, int M, int N, int K) {
    static thread_local char text[64];
    auto fail = [](const char *what) -> const char * {
        set_error("gemm256_tiles: %s", what);
        return nullptr;
    };
    if (form < G256_PLAIN || form > G256_QKV_ROPE || operands < G256_F16 || operands > G256_W8) return fail("unknown form or operand format");
    if (M <= 0 || N <= 0 || K <= 0) return fail("bad shape");
    if (form == G256_SWIGLU && N % 8 != 0) return fail("SwiGLU form: two_inter % 8 == 0");
    if (form == G256_QKV_ROPE && N % 128 != 0) return fail("QKV + RoPE form: N % 128 == 0");
    g256_plan_text(plan_gemm256(static_cast<G256Form>(form), static_cast<G256Operands>(operands), M, N, K), text, sizeof(text));
    return text;
}

extern "C" int llmie_batched_gemm(const void *a, const void *b, void *c, int batch, int m, int n, int k,
                                  int trans_b, llmie_dtype dtype, llmie_stream stream) {
    LLMIE_REQUIRE(a && b && c, "batched_gemm: NULL pointer");
    LLMIE_REQUIRE(batch > 0 && m > 0 && n > 0 && k > 0, "batched_gemm: bad shape");
    LLMIE_REQUIRE(batch <= 65535, "batched_gemm: batch > 65535");
    hipStream_t st = as_stream(stream);
    if (dtype == LLMIE_F16 && trans_b && k % 64 == 0 && m >= 32 &&
        ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) % 16 == 0) && reinterpret_cast<uintptr_t>(c) % 8 == 0 &&
        (static_cast<size_t>(m) * k) % 8 == 0 && (static_cast<size_t>(n) * k) % 8 == 0 && (static_cast<size_t>(m) * n) % 4 == 0) {
        dim3 grid((n + 127) / 128, (m + 127) / 128, batch);
        tiled_mfma_f16_kernel<false><<<grid, 256, 0, st>>>((const half_t *)a, (const half_t *)b, (half_t *)c, m, n, k,
                                                          static_cast<size_t>(m) * k, static_cast<size_t>(n) * k,
                                                          static_cast<size_t>(m) * n, nullptr, nullptr);
    } else if (dtype == LLMIE_F16)
        launch_generic<half_t>((const half_t *)a, (const half_t *)b, (half_t *)c, batch, m, n, k, trans_b != 0,
                               nullptr, nullptr, st);
    else if (dtype == LLMIE_F32)
        launch_generic<float>((const float *)a, (const float *)b, (float *)c, batch, m, n, k, trans_b != 0,
                              nullptr, nullptr, st);
    else
        LLMIE_UNSUPPORTED("batched_gemm: dtype %d", (int)dtype);
    return launch_status("batched_gemm");
}
