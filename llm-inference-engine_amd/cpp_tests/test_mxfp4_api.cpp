// launchQuantizeMxfp4 / launchDequantizeMxfp4 / launchLinearMxfp4 (api/kernels.hpp): a host restatement of the format (plain loops)
// against the device quantiser and de-quantiser, bit for bit, and the projection on integer-times-power-of-two operands whose fp16
// answer is exactly known (computed in double, rounded once) at one row count per route: 3 (GEMV), 20 (MFMA), 70 (row chunks) and
// 200 (the fp16 image).  Run on the GPU by tests/test_mxfp4_engine_gpu.py; exit code != 0 on any failure.
#include <cstdint>

#include "../src/kernels/includes/linear.cuh"   // all launchers arrive through api/kernels.hpp
#include "test_common.hpp"

namespace {
const double kMag[8] = {0, 0.5, 1, 1.5, 2, 3, 4, 6};
double code_value(unsigned code, int e) { return (code & 8 ? -1.0 : 1.0) * kMag[code & 7] * std::ldexp(1.0, e); }
unsigned code_at(const std::vector<uint8_t> &wq, size_t i) { return (wq[i / 2] >> (4 * (i % 2))) & 0xF; }

// the quantiser of include/llmie.h on finite inputs
void quantize_host(const std::vector<float> &w, int N, int K, std::vector<uint8_t> &wq, std::vector<uint8_t> &scale) {
    wq.assign(static_cast<size_t>(N) * K / 2, 0);
    scale.assign(static_cast<size_t>(N) * K / 32, 0);
    for (size_t b = 0; b < scale.size(); ++b) {
        float amax = 0.f;
        for (int t = 0; t < 32; ++t) amax = std::fmax(amax, std::fabs(w[b * 32 + t]));
        int e = 0;
        if (amax > 0.f) {
            int ex;
            std::frexp(amax, &ex);   // amax = f * 2^ex, f in [0.5, 1): floor(log2(amax)) = ex - 1
            e = ex - 1 - 2;
            e = e < -23 ? -23 : (e > 13 ? 13 : e);
        }
        scale[b] = static_cast<uint8_t>(e + 127);
        for (int t = 0; t < 32; ++t) {
            const float v = w[b * 32 + t], r = std::ldexp(std::fabs(v), -e);
            const unsigned code = (r > 0.25f) + (r >= 0.75f) + (r > 1.25f) + (r >= 1.75f) + (r > 2.5f) + (r >= 3.5f) + (r > 5.f);
            const size_t i = b * 32 + t;
            wq[i / 2] |= static_cast<uint8_t>((code | (std::signbit(v) ? 8u : 0u)) << (4 * (i % 2)));
        }
    }
}
}  // namespace

int main() {
    std::mt19937_64 rng(5);
    {   // quantiser and de-quantiser against the host restatement
        const int N = 19, K = 96;
        std::vector<float> w = storage_round<half>(randn(rng, static_cast<size_t>(N) * K, 0.3f));
        const float ties[7] = {0.25f, 0.75f, 1.25f, 1.75f, 2.5f, 3.5f, 5.f};
        for (int t = 0; t < 7; ++t) w[t + 1] = ties[t] * 0.125f, w[40 + t] = -ties[t] * 4.f;
        w[0] = 4.f * 0.125f, w[39] = 7.f * 4.f;                          // the blocks' maxima: e = -3 and e = 2 (7 saturates at 6)
        for (int t = 0; t < 32; ++t) w[64 + t] = t % 3 ? 0.f : -0.f;      // an all-zero block
        std::vector<uint8_t> eq, es;
        quantize_host(w, N, K, eq, es);
        DeviceArray<half> d_w(to_half(w));
        DeviceArray<uint8_t> d_q(eq.size()), d_s(es.size());
        TensorWrapper<half> t_w(Device::GPU, getTensorType<half>(), {N, K}, d_w.d);
        launchQuantizeMxfp4(&t_w, d_q.d, d_s.d);
        CHECK(hipStreamSynchronize(llmie_api::st()));
        check_equal("QuantizeMxfp4 scales", d_s.download(), es);
        check_equal("QuantizeMxfp4 codes", d_q.download(), eq);
        std::vector<half> ew(w.size());
        for (size_t i = 0; i < w.size(); ++i) ew[i] = __float2half(static_cast<float>(code_value(code_at(eq, i), int(es[i / 32]) - 127)));
        DeviceArray<half> d_o(w.size());
        TensorWrapper<half> t_o(Device::GPU, getTensorType<half>(), {N, K}, d_o.d);
        launchDequantizeMxfp4(d_q.d, d_s.d, &t_o);
        CHECK(hipStreamSynchronize(llmie_api::st()));
        check_equal("DequantizeMxfp4", d_o.download(), ew);
    }
    // the projection: x = i * 2^(m % 4), |i| <= 3; codes over all 16 values; block exponents -6 .. -4 inside a row, shifted by the row:
    // every product and partial sum is a multiple of 2^-9 and the sum of |terms| at most 2080 * 24 * 192 = 9.6e6 < 2^24 of them: the
    // answer is the fp16 rounding of an exact number
    const int K = 2080, N = 50;
    std::vector<uint8_t> wq(static_cast<size_t>(N) * K / 2), sc(static_cast<size_t>(N) * K / 32);
    for (auto &b : wq) b = static_cast<uint8_t>(rng() & 0xFF);
    for (int n = 0; n < N; ++n)
        for (int b = 0; b < K / 32; ++b) sc[static_cast<size_t>(n) * (K / 32) + b] = static_cast<uint8_t>(127 - 6 + (b * 7 + n) % 3 - n % 3);
    DeviceArray<uint8_t> d_q(wq), d_s(sc);
    const std::vector<float> biasf = storage_round<half>(randu(rng, N, 4.f));
    std::vector<float> bias(N);
    for (int n = 0; n < N; ++n) bias[n] = std::nearbyint(biasf[n]) * 0.25f;
    DeviceArray<half> d_bias(to_half(bias));
    for (int M : {3, 20, 70, 200}) {
        std::vector<float> x(static_cast<size_t>(M) * K), res(static_cast<size_t>(M) * N);
        for (int m = 0; m < M; ++m)
            for (int k = 0; k < K; ++k) x[static_cast<size_t>(m) * K + k] = std::ldexp(static_cast<float>(int(rng() % 7) - 3), m % 4);
        for (auto &r : res) r = static_cast<float>(int(rng() % 33) - 16) * 0.5f;
        std::vector<half> expect(static_cast<size_t>(M) * N), expect_epi(expect.size());
        for (int m = 0; m < M; ++m)
            for (int n = 0; n < N; ++n) {
                double acc = 0.0;
                for (int k = 0; k < K; ++k)
                    acc += static_cast<double>(x[static_cast<size_t>(m) * K + k]) *
                           code_value(code_at(wq, static_cast<size_t>(n) * K + k), int(sc[static_cast<size_t>(n) * (K / 32) + k / 32]) - 127);
                expect[static_cast<size_t>(m) * N + n] = __float2half(static_cast<float>(acc));   // (exact in float: < 2^24 units)
                expect_epi[static_cast<size_t>(m) * N + n] = __float2half(static_cast<float>(acc + bias[n] + res[static_cast<size_t>(m) * N + n]));
            }
        DeviceArray<half> d_x(to_half(x)), d_y(expect.size()), d_r(to_half(res));
        TensorWrapper<half> t_x(Device::GPU, getTensorType<half>(), {M, K}, d_x.d), t_y(Device::GPU, getTensorType<half>(), {M, N}, d_y.d);
        TensorWrapper<half> t_b(Device::GPU, getTensorType<half>(), {N}, d_bias.d), t_r(Device::GPU, getTensorType<half>(), {M, N}, d_r.d);
        char what[96];
        launchLinearMxfp4(&t_x, d_q.d, d_s.d, &t_y);
        CHECK(hipStreamSynchronize(llmie_api::st()));
        std::snprintf(what, sizeof(what), "LinearMxfp4 M=%d", M);
        check_equal(what, d_y.download(), expect);
        launchLinearMxfp4(&t_x, d_q.d, d_s.d, &t_r, &t_b, &t_r);   // bias + residual in place
        CHECK(hipStreamSynchronize(llmie_api::st()));
        std::snprintf(what, sizeof(what), "LinearMxfp4 M=%d bias + residual in place", M);
        check_equal(what, d_r.download(), expect_epi);
    }
    std::printf(g_failures ? "%d FAILED\n" : "all passed (%d failures)\n", g_failures);
    return g_failures ? 1 : 0;
}
