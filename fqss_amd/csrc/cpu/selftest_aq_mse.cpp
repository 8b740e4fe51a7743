// Driver of the sanitizer build of the histogram-MSE activation observer (make asan_aq_mse): fqss_aq_hist and fqss_aq_mse_search of
// fqss_cpu.cpp on tensors of 1, 513 and 4099 values (one constant, one read from an address that is no multiple of 16), a void row, rows of
// very different ranges (the capped grid) and bad arguments, every buffer sized exactly.  The contract's own identities are checked;
// AddressSanitizer / UBSan do the rest.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fqss.h"
#define CHECK(x) do { if (!(x)) { printf("FAILED: %s (line %d): %s\n", #x, __LINE__, fqss_last_error()); return 1; } } while (0)

static uint32_t ordered(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// one observation of n values at scale s into row t; returns non-zero on a failed identity
static int observe(std::vector<uint32_t>& hist, std::vector<float>& rng, int t, int64_t n, float s, bool constant, int64_t offset) {
    std::vector<float> buf((size_t)(n + offset));
    float* x = buf.data() + offset;
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t i = 0; i < n; ++i) {
        float v = 0.0f;
        for (int j = 0; j < 4; ++j) v += (float)rand() / (float)RAND_MAX - 0.5f;
        x[i] = constant ? 1.5f : s * v;
        lo = fminf(lo, x[i]);
        hi = fmaxf(hi, x[i]);
    }
    uint32_t obs[2] = {ordered(lo), ordered(hi)};
    CHECK(fqss_aq_hist(x, n, obs, hist.data() + (size_t)t * FQSS_AQ_HIST_BINS, rng.data() + 2 * t, nullptr) == 0);
    CHECK(obs[0] == 0xFFFFFFFFu && obs[1] == 0u && rng[2 * t] == lo && rng[2 * t + 1] == hi);
    uint64_t total = 0;
    for (int k = 0; k < FQSS_AQ_HIST_BINS; ++k) total += hist[(size_t)t * FQSS_AQ_HIST_BINS + k];
    CHECK(total == (uint64_t)n);
    return 0;
}

static int search(const std::vector<uint32_t>& hist, const std::vector<float>& rng, int T, bool expect_cap) {
    std::vector<double> ws((size_t)(fqss_aq_mse_ws_bytes(T) / 8));
    CHECK(!ws.empty());
    float qmin = -0.5f, qmax = 0.5f;
    int ij[2] = {-7, -7};
    double err = -1.0;
    CHECK(fqss_aq_mse_search(hist.data(), rng.data(), T, 8, ws.data(), &qmin, &qmax, ij, &err, nullptr) == 0);
    CHECK(ij[0] >= 0 && ij[0] < FQSS_AQ_MSE_N && ij[1] >= 0 && ij[1] < FQSS_AQ_MSE_N && err >= 0.0 && qmin < qmax);
    CHECK(!expect_cap || ws[3] == (double)FQSS_AQ_MSE_MAX_BINS);
    float qmin2 = -0.5f, qmax2 = 0.5f;
    CHECK(fqss_aq_mse_search(hist.data(), rng.data(), T, 8, ws.data(), &qmin2, &qmax2, nullptr, nullptr, nullptr) == 0);   // optional outputs absent
    CHECK(qmin2 == qmin && qmax2 == qmax);
    return 0;
}

int main() {
    {   // five rows of growing scale, sizes 1 / 513 / 4099, one constant, one off 16-byte alignment, and a void row among them
        const int T = 6;
        std::vector<uint32_t> hist((size_t)T * FQSS_AQ_HIST_BINS, 0u);
        std::vector<float> rng((size_t)2 * T, 0.0f);
        if (observe(hist, rng, 0, 1, 1.0f, false, 0)) return 1;
        if (observe(hist, rng, 1, 513, 1.0f, false, 0)) return 1;
        if (observe(hist, rng, 2, 4099, 2.0f, false, 1)) return 1;
        if (observe(hist, rng, 3, 300, 1.0f, true, 3)) return 1;
        if (observe(hist, rng, 5, 4099, 3.0f, false, 0)) return 1;
        float x = 1.0f;
        uint32_t obs[2] = {0xFFFFFFFFu, 0u};                              // nothing observed: row 4 is void
        CHECK(fqss_aq_hist(&x, 1, obs, hist.data() + 4 * FQSS_AQ_HIST_BINS, rng.data() + 8, nullptr) == 0);
        CHECK(std::isnan(rng[8]) && std::isnan(rng[9]) && hist[4 * FQSS_AQ_HIST_BINS] == 0u);
        if (search(hist, rng, T, false)) return 1;
        if (search(hist, rng, 1, false)) return 1;
        float qmin = -0.5f, qmax = 0.5f;                                  // only the void row: the ranges stay
        int ij[2] = {0, 0};
        std::vector<double> ws((size_t)(fqss_aq_mse_ws_bytes(1) / 8));
        CHECK(fqss_aq_mse_search(hist.data() + 4 * FQSS_AQ_HIST_BINS, rng.data() + 8, 1, 8, ws.data(), &qmin, &qmax, ij, nullptr, nullptr) == 0);
        CHECK(qmin == -0.5f && qmax == 0.5f && ij[0] == -1 && ij[1] == -1);
    }
    {   // a range of 1e-3 beside one of 100: the capped grid
        std::vector<uint32_t> hist((size_t)2 * FQSS_AQ_HIST_BINS, 0u);
        std::vector<float> rng(4, 0.0f);
        if (observe(hist, rng, 0, 513, 1e-3f, false, 0)) return 1;
        if (observe(hist, rng, 1, 513, 50.0f, false, 0)) return 1;
        if (search(hist, rng, 2, true)) return 1;
    }
    {   // padded rows read in place: 5 rows of 37 values, 48 apart, the last row ending with the buffer
        std::vector<float> m((size_t)(4 * 48 + 37), 1e30f);
        for (int r = 0; r < 5; ++r)
            for (int c = 0; c < 37; ++c) m[(size_t)(r * 48 + c)] = (float)((r * 37 + c) % 11) - 5.0f;
        std::vector<uint32_t> hr(FQSS_AQ_HIST_BINS, 0u);
        float rr[2];
        uint32_t ob[2] = {ordered(-5.0f), ordered(5.0f)};
        CHECK(fqss_aq_hist_rows(m.data(), 5, 37, 48, ob, hr.data(), rr, nullptr) == 0);
        uint64_t total = 0;
        for (uint32_t v : hr) total += v;
        CHECK(total == 5 * 37 && rr[0] == -5.0f && rr[1] == 5.0f && hr[0] > 0 && hr[FQSS_AQ_HIST_BINS - 1] > 0);
        CHECK(fqss_aq_hist_rows(m.data(), 5, 37, 36, ob, hr.data(), rr, nullptr) == FQSS_EINVAL);
        CHECK(fqss_aq_mse_ws_offset(1, FQSS_AQ_WS_HDR) == 0 && fqss_aq_mse_ws_offset(1, 6) == -1 && fqss_aq_mse_ws_offset(0, 0) == -1);
        CHECK((fqss_aq_mse_ws_offset(3, FQSS_AQ_WS_ERR) + FQSS_AQ_MSE_N * FQSS_AQ_MSE_N) * 8 == fqss_aq_mse_ws_bytes(3));
    }
    std::vector<uint32_t> h(FQSS_AQ_HIST_BINS, 0u);
    std::vector<double> ws((size_t)(fqss_aq_mse_ws_bytes(1) / 8));
    float r[2] = {0.0f, 1.0f}, x = 0.5f, qmin = -1.0f, qmax = 1.0f;
    uint32_t obs[2] = {ordered(0.0f), ordered(1.0f)};
    CHECK(fqss_aq_mse_ws_bytes(0) == 0 && fqss_aq_mse_ws_bytes(FQSS_AQ_MSE_MAX_ROWS + 1) == 0);
    CHECK(fqss_aq_hist(nullptr, 1, obs, h.data(), r, nullptr) == FQSS_EINVAL);
    CHECK(fqss_aq_hist(&x, 0, obs, h.data(), r, nullptr) == FQSS_EINVAL);
    CHECK(fqss_aq_hist(&x, (int64_t)1 << 32, obs, h.data(), r, nullptr) == FQSS_EINVAL);
    CHECK(fqss_aq_mse_search(h.data(), r, 1, 4, ws.data(), &qmin, &qmax, nullptr, nullptr, nullptr) == FQSS_EINVAL);
    CHECK(fqss_aq_mse_search(h.data(), r, 0, 8, ws.data(), &qmin, &qmax, nullptr, nullptr, nullptr) == FQSS_EINVAL);
    CHECK(fqss_aq_mse_search(h.data(), r, 65, 8, ws.data(), &qmin, &qmax, nullptr, nullptr, nullptr) == FQSS_EINVAL);
    CHECK(qmin == -1.0f && qmax == 1.0f && obs[0] == ordered(0.0f));      // a refused call writes nothing
    printf("selftest_aq_mse ok\n");
    return 0;
}
