// Driver of the sanitizer build of the MSE weight observer (make asan_wq_mse): fqss_wq_observe_mse and fqss_wq_error of fqss_cpu.cpp on
// both weight layouts ([C][inner] and [outer][C][inner] with outer, inner > 1), channel lengths 1, 65 and 1536, an all-zero channel and a
// bad width, buffers sized exactly.  The contract's own identities are checked; AddressSanitizer / UBSan do the rest.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fqss.h"
#define CHECK(x) do { if (!(x)) { printf("FAILED: %s (line %d): %s\n", #x, __LINE__, fqss_last_error()); return 1; } } while (0)

static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

// one weight [outer][C][inner]; channel `zero_ch` (or none: -1) is all zero
static int run(int64_t outer, int64_t C, int64_t inner, int n_bits, int64_t zero_ch) {
    std::vector<float> w((size_t)(outer * C * inner));
    for (auto& x : w) {          // a bell-ish shape: the sum of four uniforms
        float s = 0.0f;
        for (int j = 0; j < 4; ++j) s += (float)rand() / (float)RAND_MAX - 0.5f;
        x = 0.1f * s;
    }
    if (zero_ch >= 0)
        for (int64_t o = 0; o < outer; ++o)
            for (int64_t i = 0; i < inner; ++i) w[(size_t)((o * C + zero_ch) * inner + i)] = 0.0f;
    std::vector<float> lo0((size_t)C), hi0((size_t)C), lo((size_t)C, -0.5f), hi((size_t)C, 0.5f), lo2((size_t)C), hi2((size_t)C);
    std::vector<int> k((size_t)C, -1);
    std::vector<double> err((size_t)(2 * C), -1.0), e0((size_t)C), ek((size_t)C), p0((size_t)C), pk((size_t)C);
    CHECK(fqss_wq_observe(w.data(), outer, C, inner, lo0.data(), hi0.data(), nullptr) == 0);
    CHECK(fqss_wq_observe_mse(w.data(), outer, C, inner, lo.data(), hi.data(), n_bits, k.data(), err.data(), nullptr) == 0);
    CHECK(fqss_wq_observe_mse(w.data(), outer, C, inner, lo2.data(), hi2.data(), n_bits, nullptr, nullptr, nullptr) == 0);   // optional outputs absent
    CHECK(fqss_wq_error(w.data(), outer, C, inner, lo0.data(), hi0.data(), n_bits, e0.data(), p0.data(), nullptr) == 0);
    CHECK(fqss_wq_error(w.data(), outer, C, inner, lo.data(), hi.data(), n_bits, ek.data(), pk.data(), nullptr) == 0);
    for (int64_t c = 0; c < C; ++c) {
        CHECK(k[c] >= 0 && k[c] < FQSS_WQ_MSE_STEPS);
        const float r = (float)(FQSS_WQ_MSE_DEN - k[c]) / (float)FQSS_WQ_MSE_DEN;
        CHECK(same_bits(lo[c], r * lo0[c]) && same_bits(hi[c], r * hi0[c]));
        CHECK(same_bits(lo[c], lo2[c]) && same_bits(hi[c], hi2[c]));
        CHECK(err[2 * c] == e0[c] && err[2 * c + 1] == ek[c]);          // the same sums in the same order
        CHECK(ek[c] <= e0[c] && p0[c] == pk[c]);
        if (c == zero_ch) CHECK(k[c] == 0 && lo[c] == 0.0f && hi[c] == 0.0f && e0[c] == 0.0 && p0[c] == 0.0);
    }
    return 0;
}

int main() {
    const int64_t lengths[3][2] = {{1, 1}, {13, 5}, {96, 16}};           // (outer or Ci, inner): channel lengths 1, 65, 1536
    for (const auto& l : lengths)
        for (int n_bits : {2, 4, 8}) {
            if (run(1, 3, l[0] * l[1], n_bits, 1)) return 1;             // [C][length]
            if (run(l[0], 3, l[1], n_bits, 2)) return 1;                 // [outer][C][inner]
        }
    std::vector<float> w(12, 0.25f), lo(3, -1.0f), hi(3, 1.0f);
    std::vector<double> e(3), p(3);
    CHECK(fqss_wq_observe_mse(w.data(), 1, 3, 4, lo.data(), hi.data(), 1, nullptr, nullptr, nullptr) == FQSS_EINVAL);
    CHECK(fqss_wq_observe_mse(w.data(), 1, 3, 4, lo.data(), hi.data(), 9, nullptr, nullptr, nullptr) == FQSS_EINVAL);
    CHECK(fqss_wq_error(w.data(), 1, 3, 4, lo.data(), hi.data(), 9, e.data(), p.data(), nullptr) == FQSS_EINVAL);
    CHECK(fqss_wq_error(w.data(), 1, 3, 4, lo.data(), hi.data(), 4, nullptr, p.data(), nullptr) == FQSS_EINVAL);
    CHECK(fqss_wq_observe_mse(nullptr, 1, 3, 4, lo.data(), hi.data(), 4, nullptr, nullptr, nullptr) == FQSS_EINVAL);
    CHECK(fqss_wq_observe_mse(w.data(), 1, 0, 4, lo.data(), hi.data(), 4, nullptr, nullptr, nullptr) == FQSS_EINVAL);
    CHECK(lo[0] == -1.0f && hi[2] == 1.0f);                              // a refused call writes nothing
    printf("selftest_wq_mse ok\n");
    return 0;
}
