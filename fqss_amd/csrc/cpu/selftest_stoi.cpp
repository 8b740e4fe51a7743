// Driver of the sanitizer build of the short-time objective intelligibility (make asan_stoi): fqss_stoi of fqss_cpu.cpp at the three
// ratios served (1 / 1, 5 / 4, 5 / 8), on pitched rows, lengths around the frame rule (256 + 128 k and one more), fewer than 30 frames, no
// frame at all and a silent stretch, buffers sized exactly.  The contract's own identities are checked (estimate = reference gives 1,
// noise lowers d, too few frames give 1e-5, refusals write nothing); AddressSanitizer / UBSan do the rest.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fqss.h"
#define CHECK(x) do { if (!(x)) { printf("FAILED: %s (line %d): %s\n", #x, __LINE__, fqss_last_error()); return 1; } } while (0)

static const double kPi = 3.14159265358979323846;

// the taps of include/fqss.h, step 1 (kaiser through the power series of I0)
static double bessel_i0(double x) {
    double s = 1.0, t = 1.0;
    for (int k = 1; k < 64; ++k) {
        t *= (x / (2.0 * k)) * (x / (2.0 * k));
        s += t;
    }
    return s;
}
static std::vector<double> make_taps(int up, int down) {
    if (up == down) return {1.0};
    const double fc = 1.0 / (2.0 * (up > down ? up : down)), beta = 0.1102 * (60.0 - 8.7);
    const int half = (int)ceil((60.0 - 8.0) / (28.714 * fc / 10.0));
    std::vector<double> h((size_t)(2 * half + 1));
    double sum = 0.0;
    for (int t = -half; t <= half; ++t) {
        const double r = (double)t / half, a = 2.0 * fc * t;
        const double sinc = t == 0 ? 1.0 : sin(kPi * a) / (kPi * a);
        h[(size_t)(t + half)] = bessel_i0(beta * sqrt(1.0 - r * r)) / bessel_i0(beta) * 2.0 * up * fc * sinc;
        sum += h[(size_t)(t + half)];
    }
    for (auto& v : h) v *= up / sum;
    return h;
}

// P pairs of L samples at fs = 10000 down / up: a harmonic stack under a slow envelope, quiet from 40 % to 55 % of the length
static int run(int up, int down, int64_t L, int P, bool expect_number) {
    const double fs = 10000.0 * down / up;
    const int64_t ld = L + 3;
    std::vector<float> ref((size_t)(P * ld)), est((size_t)(P * ld)), same((size_t)(P * ld));
    for (int p = 0; p < P; ++p)
        for (int64_t i = 0; i < L; ++i) {
            const double t = (double)i / fs;
            double v = 0.0;
            for (int h = 1; h <= 12; ++h) v += sin(2.0 * kPi * (180.0 + 7.0 * p) * h * t + h) / h;
            v *= 0.05 * (0.6 + 0.4 * sin(2.0 * kPi * 3.0 * t));
            if (i > 2 * L / 5 && i < 11 * L / 20) v *= 1e-4;
            ref[(size_t)(p * ld + i)] = same[(size_t)(p * ld + i)] = (float)v;
            est[(size_t)(p * ld + i)] = (float)(v + 0.02 * ((double)rand() / RAND_MAX - 0.5));
        }
    const std::vector<double> taps = make_taps(up, down);
    const int64_t need = fqss_stoi_ws_doubles(P, L, up, down);
    CHECK(need > 0);
    std::vector<double> ws((size_t)need), d((size_t)P, -7.0), d1((size_t)P, -7.0);
    CHECK(fqss_stoi(est.data(), ref.data(), taps.data(), (int)taps.size(), ws.data(), need, d.data(), P, L, ld, ld, up, down, nullptr) == 0);
    CHECK(fqss_stoi(same.data(), ref.data(), taps.data(), (int)taps.size(), ws.data(), need, d1.data(), P, L, ld, ld, up, down, nullptr) == 0);
    for (int p = 0; p < P; ++p) {
        if (expect_number) {
            CHECK(fabs(d1[(size_t)p] - 1.0) < 1e-12);
            CHECK(d[(size_t)p] > 0.2 && d[(size_t)p] < 0.9999);
        } else {
            CHECK(d[(size_t)p] == 1e-5 && d1[(size_t)p] == 1e-5);
        }
    }
    CHECK(fqss_stoi(est.data(), ref.data(), taps.data(), (int)taps.size(), ws.data(), need - 1, d.data(), P, L, ld, ld, up, down, nullptr) == FQSS_EINVAL);
    CHECK(fqss_stoi(est.data(), ref.data(), taps.data(), (int)taps.size(), ws.data(), need, d.data(), P, L, L - 1, ld, up, down, nullptr) == FQSS_EINVAL);
    return 0;
}

int main() {
    const int ratios[3][2] = {{1, 1}, {5, 4}, {5, 8}};
    CHECK(make_taps(5, 4).size() == 365 && make_taps(5, 8).size() == 581);
    for (const auto& r : ratios) {
        const int64_t edge = ((256 + 128 * 44) * (int64_t)r[1] + r[0] - 1) / r[0];      // about 256 + 128 * 44 samples at 10 kHz
        if (run(r[0], r[1], edge, 2, true)) return 1;
        if (run(r[0], r[1], edge + 1, 1, true)) return 1;
        if (run(r[0], r[1], edge + 3, 3, true)) return 1;
        if (run(r[0], r[1], 9000, 1, true)) return 1;
        if (run(r[0], r[1], 2000, 2, false)) return 1;       // fewer than 30 frames
        if (run(r[0], r[1], 100, 1, false)) return 1;        // no frame at all
        if (run(r[0], r[1], 1, 1, false)) return 1;
    }
    std::vector<float> x(600, 0.25f);
    std::vector<double> taps = make_taps(5, 4), ws(8192), d(1, -7.0), even(364, 1.0);
    const int n = (int)taps.size();
    CHECK(fqss_stoi(x.data(), x.data(), taps.data(), n, ws.data(), 8192, d.data(), 0, 600, 600, 600, 5, 4, nullptr) == FQSS_EINVAL);
    CHECK(fqss_stoi(x.data(), x.data(), taps.data(), n, ws.data(), 8192, d.data(), 1, 0, 600, 600, 5, 4, nullptr) == FQSS_EINVAL);
    CHECK(fqss_stoi(nullptr, x.data(), taps.data(), n, ws.data(), 8192, d.data(), 1, 600, 600, 600, 5, 4, nullptr) == FQSS_EINVAL);
    CHECK(fqss_stoi(x.data(), x.data(), nullptr, n, ws.data(), 8192, d.data(), 1, 600, 600, 600, 5, 4, nullptr) == FQSS_EINVAL);
    CHECK(fqss_stoi(x.data(), x.data(), taps.data(), n, ws.data(), 8192, d.data(), 1, 600, 600, 600, 10, 8, nullptr) == FQSS_EINVAL);
    CHECK(fqss_stoi(x.data(), x.data(), taps.data(), n, ws.data(), 8192, d.data(), 1, 600, 600, 600, 0, 4, nullptr) == FQSS_EINVAL);
    CHECK(fqss_stoi(x.data(), x.data(), taps.data(), n, ws.data(), 8192, d.data(), 1, 600, 600, 600, 5, -4, nullptr) == FQSS_EINVAL);
    CHECK(fqss_stoi(x.data(), x.data(), even.data(), 364, ws.data(), 8192, d.data(), 1, 600, 600, 600, 5, 4, nullptr) == FQSS_EINVAL);
    CHECK(fqss_stoi(x.data(), x.data(), taps.data(), n, ws.data(), 8192, d.data(), 1, 600, 600, 600, 1, 1, nullptr) == FQSS_EINVAL);
    CHECK(fqss_stoi_ws_doubles(0, 600, 5, 4) == 0 && fqss_stoi_ws_doubles(1, 0, 5, 4) == 0 && fqss_stoi_ws_doubles(1, 600, 10, 8) == 0);
    CHECK(d[0] == -7.0);                                     // a refused call writes nothing
    // 750 samples at 10 kHz: four frames
    CHECK(fqss_stoi(x.data(), x.data(), taps.data(), n, ws.data(), 8192, d.data(), 1, 600, 600, 600, 5, 4, nullptr) == 0 && d[0] == 1e-5);
    printf("selftest_stoi ok\n");
    return 0;
}
