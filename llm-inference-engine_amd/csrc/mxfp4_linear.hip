// MXFP4 weights (OCP microscaling): e2m1 codes, two per byte (low nibble = even k), with one e8m0 scale byte per 32 elements
// along K (include/llmie.h states the format).  No reference counterpart.
//   llmie_quantize_mxfp4 / llmie_dequantize_mxfp4   fp16 [N, K] <-> codes [N, K/2] + scales [N, K/32]
//   llmie_linear_mxfp4                              weight-only projection under fp16 activations, what plan_linear_wq plans:
//     M <= 8   mxfp4_gemv_kernel: one, two or four waves per two weight rows, a lane's 16-byte load is one block of 32 codes; every
//              activation row is multiplied in the same pass, the block's 2^e scales the block's fp32 partial sum
//     M <= 64  mxfp4_mfma_kernel: one workgroup per 16 weight rows, 8 waves split K block-wise; v_mfma_f32_16x16x32_f16 of the
//              unscaled code fragments into a zeroed tile, the tile scaled per lane (a lane of the 16x16 C/D map owns one column =
//              one weight row) and added to the accumulator; the waves' accumulators are summed through LDS in wave order
//     M < 192  passes of <= 64 rows through the MFMA kernel;  from 192 rows: the fp16 image + the fp16 GEMM
// A code's magnitude {0, 0.5, 1, 1.5, 2, 3, 4, 6} is the fp16 whose bits are (code & 7) << 9, times 2^14: the expansion below
// builds two such halves per byte with shifts and masks and multiplies the pair by 16384 (exact, the subnormal 0.5 included).
#include "llmie_internal.h"

namespace llmie {

// mx4_expand / mx4_scale (device_utils.cuh): 8 codes of one word -> 8 unscaled fp16 weights; a scale byte -> 2^e as fp32

// ---- quantiser: one thread per block of 32 ----
__global__ __launch_bounds__(256) void mxfp4_quantize_kernel(const half_t *__restrict__ w, uint8_t *__restrict__ wq,
                                                             uint8_t *__restrict__ scale, size_t blocks, bool wq16) {
    const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= blocks) return;
    uint4_t v[4];   // the block as 16 words of two halves (even k in the low half)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const uint4_t *>(w + i * 32 + 8 * j);
    // fp16 magnitudes order as their bit patterns do.  The maximum runs on 32-bit words: written as a reduction over 16-bit lanes of
    // a half8, hipcc (ROCm 7.2) folded it to element 0 of each vector
    unsigned amax_bits = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const unsigned word = v[j / 4][j % 4], lo = word & 0x7fffu, hi = (word >> 16) & 0x7fffu;
        amax_bits = max(amax_bits, max(lo, hi));
    }
    int e = 0;
    unsigned sbyte = 127;
    if (amax_bits >= 0x7c00u) sbyte = 0xffu;   // inf or NaN in the block
    else if (amax_bits) {
        const float amax = to_f32(__builtin_bit_cast(half_t, static_cast<unsigned short>(amax_bits)));   // normal in fp32
        e = static_cast<int>((__builtin_bit_cast(unsigned, amax) >> 23) & 0xffu) - 127 - 2;
        e = e < -23 ? -23 : (e > 13 ? 13 : e);
        sbyte = static_cast<unsigned>(e + 127);
    }
    const float inv = __builtin_bit_cast(float, static_cast<unsigned>(127 - e) << 23);   // 2^-e, exact
    unsigned words[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned word = 0;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const unsigned short hb = static_cast<unsigned short>(v[j][t / 2] >> (16 * (t % 2)));
            const float r = fabsf(to_f32(__builtin_bit_cast(half_t, hb))) * inv;   // exact: a power-of-two multiple inside fp32's normal range
            // nearest magnitude of {0, .5, 1, 1.5, 2, 3, 4, 6}; a tie takes the even code; past 5: code 7 (saturation)
            const unsigned code = (r > 0.25f) + (r >= 0.75f) + (r > 1.25f) + (r >= 1.75f) + (r > 2.5f) + (r >= 3.5f) + (r > 5.f);
            const unsigned sign = (hb >> 12) & 0x8u;
            word |= (code | sign) << (4 * t);
        }
        words[j] = word;
    }
    scale[i] = static_cast<uint8_t>(sbyte);
    if (wq16) *reinterpret_cast<uint4_t *>(wq + i * 16) = uint4_t{words[0], words[1], words[2], words[3]};
    else {
#pragma unroll
        for (int j = 0; j < 16; ++j) wq[i * 16 + j] = static_cast<uint8_t>(words[j / 4] >> (8 * (j % 4)));
    }
}

// ---- fp16 image: one thread per 8 weights (one word in, 16 bytes out); magnitude x 2^e is exact in fp32 (or overflows to inf as
// the real value's fp16 does), rounded to fp16 once ----
__global__ __launch_bounds__(256) void mxfp4_dequant_kernel(const uint8_t *__restrict__ wq, const uint8_t *__restrict__ scale,
                                                            half_t *__restrict__ w16, size_t n8) {
    const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n8) return;
    const unsigned sb = scale[i / 4];
    const unsigned w = *reinterpret_cast<const unsigned *>(wq + i * 4);
    half8_t o;
    if (sb == 0xffu) {
        const half_t nan = __builtin_bit_cast(half_t, static_cast<unsigned short>(0x7e00u));
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = nan;
    } else {
        const float s = mx4_scale(sb);
        const half8_t m = mx4_expand(w);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = from_f32<half_t>(to_f32(m[j]) * s);
    }
    *reinterpret_cast<half8_t *>(w16 + i * 8) = o;
}

// ---- M <= 8: y[m, n] = sum over blocks of 2^e(n, b) * sum_{k in b} x[m, k] * code(n, k).  256 threads = 4 waves; KW of them share
// two weight rows and split the row's blocks: lane l of part p takes blocks 64 p + l, 64 (p + KW) + l, ... of both rows (one 16-byte
// load each).  A wave sums across its lanes; KW > 1: the parts' sums meet in LDS and are added in part order.  The launcher picks KW
// by K and the row count: at one row a lane then has one or two blocks and the launch N / 2 * KW waves of loads in flight (the down
// projection of a 7B layer, K = 11008 on N = 4096 rows, took 16.5 us with one wave per row pair and 12.9 us with four) ----
constexpr int kMx4GemvRowsPerWave = 2;
template <int MT, int KW>
__global__ __launch_bounds__(256) void mxfp4_gemv_kernel(const half_t *__restrict__ x, const uint8_t *__restrict__ wq,
                                                         const uint8_t *__restrict__ scale, half_t *y, int K, int N,
                                                         const half_t *__restrict__ bias, const half_t *residual) {
    constexpr int R = kMx4GemvRowsPerWave, GROUPS = 4 / KW;
    __shared__ float red[4][R * MT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int group = wave / KW, part = wave % KW;
    const int n0 = (blockIdx.x * GROUPS + group) * R;   // (rows past N: clamped loads, no store)
    const int nb = K >> 5;
    const uint8_t *wrow[R], *srow[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const size_t n = static_cast<size_t>(min(n0 + r, N - 1));
        wrow[r] = wq + n * (static_cast<size_t>(K) >> 1);
        srow[r] = scale + n * nb;
    }
    float acc[R][MT];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;
    for (int b = part * 64 + lane; b < nb; b += 64 * KW) {
        half8_t wv[R][4];
        float s[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint4_t c = load_nt(reinterpret_cast<const uint4_t *>(wrow[r] + 16 * static_cast<size_t>(b)));
            s[r] = mx4_scale(srow[r][b]);
#pragma unroll
            for (int i = 0; i < 4; ++i) wv[r][i] = mx4_expand(c[i]);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const half_t *xp = x + static_cast<size_t>(m) * K + 32 * static_cast<size_t>(b);
            half8_t xv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[i] = *reinterpret_cast<const half8_t *>(xp + 8 * i);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float p = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) p = dot8(wv[r][i], xv[i], p);
                acc[r][m] += p * s[r];
            }
        }
    }
    float sum[R][MT];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) sum[r][m] = wave_sum(acc[r][m]);
    if constexpr (KW > 1) {
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int m = 0; m < MT; ++m) red[wave][r * MT + m] = sum[r][m];
        }
        __syncthreads();
        if (part != 0) return;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                float v = red[wave][r * MT + m];
#pragma unroll
                for (int p = 1; p < KW; ++p) v += red[wave + p][r * MT + m];
                sum[r][m] = v;
            }
    }
    if (lane != 0) return;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int n = n0 + r;
        if (n >= N) continue;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            float v = sum[r][m];
            if (bias) v += to_f32(bias[n]);
            if (residual) v += to_f32(residual[static_cast<size_t>(m) * N + n]);
            y[static_cast<size_t>(m) * N + n] = from_f32<half_t>(v);
        }
    }
}

// ---- 8 < M <= 64: one workgroup = one tile of 16 weight rows, NW waves take the 32-deep blocks in groups of U.  A operand = the
// activations (lane (r, q): row m = 16 j + r, k = 8 q .. 8 q + 7 of the block), B operand = the expanded codes (weight row r, the
// same k), so lane (r, q) of the C/D tile holds D[m = 16 j + 4 q + e][n = r], e = 0..3: one weight row, one scale, per lane ----
template <int MT, int NW>
__global__ __launch_bounds__(NW * 64) void mxfp4_mfma_kernel(const half_t *__restrict__ x, const uint8_t *__restrict__ wq,
                                                             const uint8_t *__restrict__ scale, half_t *y, int M, int K, int N,
                                                             const half_t *__restrict__ bias, const half_t *residual) {
    __shared__ floatx4 red[NW][MT][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int nb = K >> 5;
    const size_t nrow = static_cast<size_t>(min(static_cast<int>(blockIdx.x) * 16 + r, N - 1));
    const uint8_t *wp = wq + nrow * (static_cast<size_t>(K) >> 1) + 4 * q;
    const uint8_t *sp = scale + nrow * nb;
    const half_t *xp[MT];
    bool xok[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        xok[j] = (16 * j + r) < M;
        xp[j] = x + static_cast<size_t>(xok[j] ? 16 * j + r : 0) * K + 8 * q;
    }
    floatx4 acc[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
    constexpr int U = 4;
    for (int b0 = wave * U; b0 < nb; b0 += NW * U) {
        unsigned c[U], sb[U];
        half8_t a[U][MT];
#pragma unroll
        for (int u = 0; u < U; ++u) {   // unconditional loads (clamped block / row 0 for rows past M), zeroed by the selects below
            const size_t b = static_cast<size_t>(min(b0 + u, nb - 1));
            c[u] = load_nt(reinterpret_cast<const unsigned *>(wp + 16 * b));
            sb[u] = sp[b];
#pragma unroll
            for (int j = 0; j < MT; ++j) a[u][j] = *reinterpret_cast<const half8_t *>(xp[j] + 32 * b);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool live = b0 + u < nb;
            const half8_t bw = mx4_expand(c[u]);
            const float s = live ? mx4_scale(sb[u]) : 0.f;
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const half8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
                const floatx4 t = __builtin_amdgcn_mfma_f32_16x16x32_f16((live && xok[j]) ? a[u][j] : z, bw,
                                                                         floatx4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                acc[j] += t * s;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < MT; ++j) red[wave][j][lane] = acc[j];
    __syncthreads();
    for (int j = wave; j < MT; j += NW) {
        floatx4 sum = red[0][j][lane];
#pragma unroll
        for (int w = 1; w < NW; ++w) sum += red[w][j][lane];
        const int n = blockIdx.x * 16 + r;
        if (n < N) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int m = 16 * j + 4 * q + e;
                if (m < M) {
                    float v = sum[e];
                    if (bias) v += to_f32(bias[n]);
                    if (residual) v += to_f32(residual[static_cast<size_t>(m) * N + n]);
                    y[static_cast<size_t>(m) * N + n] = from_f32<half_t>(v);
                }
            }
        }
    }
}

static void mxfp4_gemv_launch(const half_t *x, const uint8_t *wq, const uint8_t *scale, half_t *y, int M, int K, int N,
                              const half_t *bias, const half_t *residual, hipStream_t st) {
    // waves per row pair, up to 4 activation rows: one or two blocks per lane (K = 4096: 2, from K = 8192: 4).  More rows: one wave
    // (measured at 8 rows on the 7B shapes: the split costs 5 .. 40 % there, where the dot products, not the loads, set the time)
    const int nb = K / 32, kw = M > 4 ? 1 : (nb >= 256 ? 4 : (nb >= 128 ? 2 : 1));
    const int rows = kMx4GemvRowsPerWave * (4 / kw);   // weight rows per workgroup
    const unsigned grid = static_cast<unsigned>((N + rows - 1) / rows);
#define LLMIE_MX4_GEMV(MT)                                                                                                  \
    case MT:                                                                                                                \
        if (kw == 4) mxfp4_gemv_kernel<MT, 4><<<grid, 256, 0, st>>>(x, wq, scale, y, K, N, bias, residual);                \
        else if (kw == 2) mxfp4_gemv_kernel<MT, 2><<<grid, 256, 0, st>>>(x, wq, scale, y, K, N, bias, residual);           \
        else mxfp4_gemv_kernel<MT, 1><<<grid, 256, 0, st>>>(x, wq, scale, y, K, N, bias, residual);                        \
        break
    switch (M) {
        LLMIE_MX4_GEMV(1); LLMIE_MX4_GEMV(2); LLMIE_MX4_GEMV(3); LLMIE_MX4_GEMV(4);
        LLMIE_MX4_GEMV(5); LLMIE_MX4_GEMV(6); LLMIE_MX4_GEMV(7); LLMIE_MX4_GEMV(8);
    }
#undef LLMIE_MX4_GEMV
}

// 1 <= M <= 64 rows
static void mxfp4_mfma_launch(const half_t *x, const uint8_t *wq, const uint8_t *scale, half_t *y, int M, int K, int N,
                              const half_t *bias, const half_t *residual, hipStream_t st) {
    const unsigned tiles = static_cast<unsigned>((N + 15) / 16);
    switch ((M + 15) / 16) {
        case 1: mxfp4_mfma_kernel<1, 8><<<tiles, 512, 0, st>>>(x, wq, scale, y, M, K, N, bias, residual); break;
        case 2: mxfp4_mfma_kernel<2, 8><<<tiles, 512, 0, st>>>(x, wq, scale, y, M, K, N, bias, residual); break;
        case 3: mxfp4_mfma_kernel<3, 8><<<tiles, 512, 0, st>>>(x, wq, scale, y, M, K, N, bias, residual); break;
        default: mxfp4_mfma_kernel<4, 8><<<tiles, 512, 0, st>>>(x, wq, scale, y, M, K, N, bias, residual); break;
    }
}

int dequantize_mxfp4_f16(const uint8_t *wq, const uint8_t *scale, half_t *w16, int N, int K, hipStream_t st) {
    if (K % 32 != 0 || reinterpret_cast<uintptr_t>(wq) % 4 != 0 || reinterpret_cast<uintptr_t>(w16) % 16 != 0) {
        set_error("dequantize_mxfp4: needs K %% 32 == 0 (K=%d), wq 4-byte and w16 16-byte aligned", K);
        return LLMIE_ERR_UNSUPPORTED;
    }
    const size_t n8 = static_cast<size_t>(N) * K / 8;
    mxfp4_dequant_kernel<<<static_cast<unsigned>((n8 + 255) / 256), 256, 0, st>>>(wq, scale, w16, n8);
    return launch_status("dequantize_mxfp4");
}

int linear_mxfp4(const LinearOperands &o, const LinearScratch &s, hipStream_t st) {
    const LinearCall c = linear_call(WF_MXFP4, o, s);
    const LinearPlan p = plan_linear_wq(c);
    const half_t *x = static_cast<const half_t *>(o.x), *bias = static_cast<const half_t *>(o.bias), *residual = static_cast<const half_t *>(o.residual);
    const uint8_t *wq = static_cast<const uint8_t *>(o.w), *scale = static_cast<const uint8_t *>(o.scale);
    half_t *y = static_cast<half_t *>(o.y);
    const int M = o.M, K = o.K, N = o.N;
    switch (p.route) {
        case LR_MX4_GEMV:
            mxfp4_gemv_launch(x, wq, scale, y, M, K, N, bias, residual, st);
            return launch_status("linear_mxfp4(gemv)");
        case LR_MX4_MFMA:
            mxfp4_mfma_launch(x, wq, scale, y, M, K, N, bias, residual, st);
            return launch_status("linear_mxfp4(mfma)");
        case LR_MX4_CHUNKS:
            for (int m0 = 0; m0 < M; m0 += p.pass_rows) {
                const int m = M - m0 < p.pass_rows ? M - m0 : p.pass_rows;
                mxfp4_mfma_launch(x + static_cast<size_t>(m0) * K, wq, scale, y + static_cast<size_t>(m0) * N, m, K, N, bias,
                                  residual ? residual + static_cast<size_t>(m0) * N : nullptr, st);
            }
            return launch_status("linear_mxfp4(row chunks)");
        case LR_WQ_IMAGE_PREFILL: {
            const int rc = dequantize_mxfp4_f16(wq, scale, static_cast<half_t *>(s.image), N, K, st);
            if (rc) return rc;
            LinearOperands f = o;   // the fp16 GEMM on the image, without slabs
            f.w = s.image, f.scale = nullptr;
            return linear_f16_nk(f, LinearScratch{}, st);
        }
        default:
            return linear_refuse(c, p);
    }
}

}  // namespace llmie

using namespace llmie;

extern "C" int llmie_quantize_mxfp4(const void *w, uint8_t *wq, uint8_t *scale, int N, int K, llmie_stream stream) {
    LLMIE_REQUIRE(w && wq && scale, "quantize_mxfp4: NULL pointer");
    LLMIE_REQUIRE(N > 0 && K > 0, "quantize_mxfp4: bad shape N=%d K=%d", N, K);
    if (K % 32 != 0 || reinterpret_cast<uintptr_t>(w) % 16 != 0)
        LLMIE_UNSUPPORTED("quantize_mxfp4: needs K %% 32 == 0 (K=%d) and a 16-byte aligned w", K);
    const size_t blocks = static_cast<size_t>(N) * (K / 32);
    mxfp4_quantize_kernel<<<static_cast<unsigned>((blocks + 255) / 256), 256, 0, as_stream(stream)>>>(
        static_cast<const half_t *>(w), wq, scale, blocks, reinterpret_cast<uintptr_t>(wq) % 16 == 0);
    return launch_status("quantize_mxfp4");
}

extern "C" int llmie_dequantize_mxfp4(const uint8_t *wq, const uint8_t *scale, void *w16, int N, int K, llmie_stream stream) {
    LLMIE_REQUIRE(wq && scale && w16, "dequantize_mxfp4: NULL pointer");
    LLMIE_REQUIRE(N > 0 && K > 0, "dequantize_mxfp4: bad shape N=%d K=%d", N, K);
    return dequantize_mxfp4_f16(wq, scale, static_cast<half_t *>(w16), N, K, as_stream(stream));
}

extern "C" int llmie_linear_mxfp4(const void *x, const uint8_t *wq, const uint8_t *scale, void *y, int M, int K, int N,
                                  const void *bias, const void *residual, void *workspace, size_t workspace_bytes,
                                  llmie_stream stream) {
    LLMIE_REQUIRE(x && wq && scale && y, "linear_mxfp4: NULL pointer");
    LLMIE_REQUIRE(M > 0 && K > 0 && N > 0, "linear_mxfp4: bad shape M=%d K=%d N=%d", M, K, N);
    LLMIE_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "linear_mxfp4: workspace must be 16-byte aligned");
    // workspace = the fp16 image of W from kWqPrefillRows rows on, as llmie_linear_workspace_bytes sizes it; too small for it: row chunks
    const WqWorkspace w = wq_workspace(WF_MXFP4, M, K, N, workspace, workspace_bytes);
    return linear_mxfp4(LinearOperands{x, wq, scale, y, M, K, N, EPI_NONE_, 0, bias, residual}, LinearScratch{SlabWs{nullptr, 0}, w.deq, w.deq_bytes},
                        as_stream(stream));
}
