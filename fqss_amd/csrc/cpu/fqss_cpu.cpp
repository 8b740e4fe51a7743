// fqss_cpu.cpp -- the CPU backend behind include/fqss.h for cfg 1 of BASELINE.json ("convtasnet_2spks_8k.yaml on asteroid env, CPU,
// batch 2, 1 s ... plumbing, no GPU"; reference train.py:31: device = "cpu" if use_cpu).  Plain C++ (g++, OpenMP), host pointers, the
// `stream` argument is ignored, every call is synchronous.  It serves the entry points the UN-FUSED ConvTasNet QAT step uses (the
// per-layer kernels that the G1 layer fixtures pin: KDTrainStep(coded=False, batched_quantizers=False) with the module-path teacher)
// and, of the evaluation side, the SDR (fqss_sdr), the STOI (fqss_stoi) and the batched chunked path (fqss_splitter2_rows, fqss_chunk_gather,
// fqss_sisnr_chunks, fqss_infer_ola_chunks);
// anything else is absent from this library and fqss_amd/_lib.py raises.  Arithmetic: the same op sequences as the HIP kernels
// (fp32, one IEEE operation per operator: built with -ffp-contract=off; IEEE division; round-half-even), reductions in fp64.
// NOT the oracle: oracle/ is test infrastructure and is never loaded by the product; this file is product code selected by --use_cpu.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fqss.h"

namespace {
thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
#define REQUIRE(cond, msg)                          \
    do {                                            \
        if (!(cond)) {                              \
            set_error("%s: %s", __func__, msg);     \
            return FQSS_EINVAL;                     \
        }                                           \
    } while (0)

inline uint32_t f2ord(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float ord2f(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
inline float act_neg_scale(int act, float slope) { return act == FQSS_ACT_PRELU ? slope : (act == FQSS_ACT_RELU ? 0.0f : 1.0f); }
inline float act_apply(float z, int act, float slope) { return z > 0.0f ? z : act_neg_scale(act, slope) * z; }
struct QRange {
    float lo, delta;
};
inline QRange load_qrange(const float* qmin, const float* qmax) { return QRange{*qmin, (*qmax - *qmin) / 255.0f}; }
// qat_quant.py:139-146 op for op; c = clamped index, u = pre-round coordinate
inline float fq_asym(float t, const QRange& r, float& c, float& u, bool& inr) {
    u = (t - r.lo) / r.delta;
    const float X = nearbyintf(u);   // round-half-to-even (default rounding mode) == torch.round
    inr = (X >= 0.0f) && (X <= 255.0f);
    c = fminf(fmaxf(X, 0.0f), 255.0f);
    return r.delta * c + r.lo;
}
// weight grid at width n in [2, 8]: L = 2^n - 1 levels, codes in [-2^(n-1), 2^(n-1) - 1] (exact floats)
inline float wq_levels(int n_bits) { return (float)((1 << n_bits) - 1); }
inline float wq_qlo(int n_bits) { return -(float)(1 << (n_bits - 1)); }
inline float wq_qhi(int n_bits) { return (float)((1 << (n_bits - 1)) - 1); }
inline float wq_delta(float lo, float hi, float L) { return (2.0f * fmaxf(fabsf(lo), fabsf(hi))) / L; }
inline float wq_code(float w, float delta, float qlo, float qhi) { return fminf(fmaxf(nearbyintf(w / delta), qlo), qhi); }
inline float wq_mse_ratio(int k) { return (float)(FQSS_WQ_MSE_DEN - k) / (float)FQSS_WQ_MSE_DEN; }
}  // namespace

extern "C" {

int fqss_version(void) { return FQSS_VERSION; }
const char* fqss_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------------ activation quantizer
int fqss_actq_fwd(const float* z, float* out, uint8_t* idx, int64_t rows, int64_t cols, int64_t ld_z, int64_t ld_out, int64_t ld_idx,
                  int act, const float* slope_p, int qmode, const float* qmin, const float* qmax, uint32_t* obs_ws, fqss_stream_t) {
    if (rows == 0 || cols == 0) return FQSS_OK;
    REQUIRE(z && (out || idx) && rows >= 0 && cols >= 0 && ld_z >= cols, "bad args");
    REQUIRE(act >= 0 && act <= FQSS_ACT_RELU, "act not served by the CPU backend (NONE / PReLU / ReLU only)");
    REQUIRE(act != FQSS_ACT_PRELU || slope_p, "PReLU needs a slope");
    REQUIRE(qmode != FQSS_Q_QUANT || (qmin && qmax), "QUANT needs ranges");
    REQUIRE(qmode != FQSS_Q_OBSERVE || obs_ws, "OBSERVE needs obs_ws");
    const float slope = act == FQSS_ACT_PRELU ? *slope_p : 0.0f;
    QRange r{0.0f, 1.0f};
    if (qmode == FQSS_Q_QUANT) r = load_qrange(qmin, qmax);
    float vmin = INFINITY, vmax = -INFINITY;
#pragma omp parallel for reduction(min : vmin) reduction(max : vmax) schedule(static)
    for (int64_t row = 0; row < rows; ++row) {
        const float* zr = z + row * ld_z;
        for (int64_t c0 = 0; c0 < cols; ++c0) {
            const float t = act_apply(zr[c0], act, slope);
            float o = t;
            if (qmode == FQSS_Q_QUANT) {
                float c, u;
                bool inr;
                o = fq_asym(t, r, c, u, inr);
                if (idx) idx[row * ld_idx + c0] = (uint8_t)c;
            } else if (qmode == FQSS_Q_OBSERVE) {
                vmin = fminf(vmin, t);
                vmax = fmaxf(vmax, t);
            }
            if (out) out[row * ld_out + c0] = o;
        }
    }
    if (qmode == FQSS_Q_OBSERVE) {
        const uint32_t kmin = f2ord(vmin), kmax = f2ord(vmax);
        if (kmin < obs_ws[0]) obs_ws[0] = kmin;
        if (kmax > obs_ws[1]) obs_ws[1] = kmax;
    }
    return FQSS_OK;
}

int fqss_obs_reset(uint32_t* obs_ws, int64_t n_pairs, fqss_stream_t) {
    REQUIRE(obs_ws && n_pairs >= 0, "bad args");
    for (int64_t i = 0; i < n_pairs; ++i) {
        obs_ws[2 * i] = 0xFFFFFFFFu;
        obs_ws[2 * i + 1] = 0u;
    }
    return FQSS_OK;
}

int fqss_observer_ema(float* qmin, float* qmax, uint32_t* obs_ws, double alpha, fqss_stream_t) {
    REQUIRE(qmin && qmax && obs_ws, "null pointer");
    const float a = (float)alpha, oma = (float)(1.0 - alpha);
    const float tmin = ord2f(obs_ws[0]), tmax = ord2f(obs_ws[1]);
    *qmin = a * (*qmin) + oma * tmin;   // qat_quant.py:231-232
    *qmax = a * (*qmax) + oma * tmax;
    obs_ws[0] = 0xFFFFFFFFu;
    obs_ws[1] = 0u;
    return FQSS_OK;
}

int fqss_minmax(const float* x, int64_t rows, int64_t cols, int64_t ld, uint32_t* obs_ws, fqss_stream_t) {
    if (rows == 0 || cols == 0) return FQSS_OK;
    REQUIRE(x && obs_ws && ld >= cols, "bad args");
    float vmin = INFINITY, vmax = -INFINITY;
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t c = 0; c < cols; ++c) {
            vmin = fminf(vmin, x[r * ld + c]);
            vmax = fmaxf(vmax, x[r * ld + c]);
        }
    const uint32_t kmin = f2ord(vmin), kmax = f2ord(vmax);
    if (kmin < obs_ws[0]) obs_ws[0] = kmin;
    if (kmax > obs_ws[1]) obs_ws[1] = kmax;
    return FQSS_OK;
}

// backward of out = fq(act(z)): g_C = g*delta ; g_u = g_C*m ; g_t = g_u/delta ; d/dmax = sum g*(c - m*u)/255 ; d/dmin = sum g*(1-m) - d/dmax
int fqss_actq_bwd(const float* z, const float* g, float* gz, int64_t rows, int64_t cols, int64_t ld_z, int64_t ld_g, int64_t ld_gz, int act,
                  const float* slope_p, int qmode, const float* qmin, const float* qmax, double* gacc, float* gbias, int64_t C,
                  fqss_stream_t) {
    if (rows == 0 || cols == 0) return FQSS_OK;
    REQUIRE(z && g && gz && ld_z >= cols && ld_g >= cols && ld_gz >= cols, "bad args");
    REQUIRE(act >= 0 && act <= FQSS_ACT_RELU, "act not served by the CPU backend (NONE / PReLU / ReLU only)");
    REQUIRE(act != FQSS_ACT_PRELU || slope_p, "PReLU needs a slope");
    REQUIRE(qmode != FQSS_Q_QUANT || (qmin && qmax), "QUANT needs ranges");
    REQUIRE((qmode != FQSS_Q_QUANT && act != FQSS_ACT_PRELU) || gacc, "range/slope grads need gacc");
    REQUIRE(!gbias || (C > 0 && rows % C == 0), "gbias needs C dividing rows");
    if (!gbias || C <= 0) C = rows;
    const float slope = act == FQSS_ACT_PRELU ? *slope_p : 0.0f;
    QRange r{0.0f, 1.0f};
    if (qmode == FQSS_Q_QUANT) r = load_qrange(qmin, qmax);
    double p_du = 0.0, p_out = 0.0, p_slope = 0.0;
    std::vector<double> bias(gbias ? (size_t)C : 0, 0.0);
    for (int64_t row = 0; row < rows; ++row) {
        double pb = 0.0;
        for (int64_t c0 = 0; c0 < cols; ++c0) {
            const float zv = z[row * ld_z + c0], gj = g[row * ld_g + c0];
            const float t = act_apply(zv, act, slope);
            float gt = gj;
            if (qmode == FQSS_Q_QUANT) {
                float c, u;
                bool inr;
                (void)fq_asym(t, r, c, u, inr);
                gt = inr ? (gj * r.delta) / r.delta : 0.0f;
                p_du += (double)(gj * (inr ? (c - u) : c));
                p_out += inr ? 0.0 : (double)gj;
            }
            const bool neg = !(zv > 0.0f);
            if (act == FQSS_ACT_PRELU && neg) p_slope += (double)(zv * gt);
            const float gzj = neg ? act_neg_scale(act, slope) * gt : gt;
            gz[row * ld_gz + c0] = gzj;
            pb += (double)gzj;
        }
        if (gbias) bias[(size_t)(row % C)] += pb;
    }
    if (gbias)
        for (int64_t c = 0; c < C; ++c) gbias[c] += (float)bias[(size_t)c];
    if (qmode == FQSS_Q_QUANT || act == FQSS_ACT_PRELU) {
        const double dmax = p_du / 255.0;
        gacc[0] += qmode == FQSS_Q_QUANT ? p_out - dmax : 0.0;
        gacc[1] += qmode == FQSS_Q_QUANT ? dmax : 0.0;
        gacc[2] += p_slope;
    }
    return FQSS_OK;
}

int fqss_gacc_flush(double* gacc, float* gmin, float* gmax, float* gslope, fqss_stream_t) {
    REQUIRE(gacc, "null gacc");
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < FQSS_GACC_SLOTS; ++i)
        for (int k = 0; k < 3; ++k) {
            v[k] += gacc[3 * i + k];
            gacc[3 * i + k] = 0.0;
        }
    if (gmin) *gmin += (float)v[0];
    if (gmax) *gmax += (float)v[1];
    if (gslope) *gslope += (float)v[2];
    return FQSS_OK;
}

// ------------------------------------------------------------------------------------------------ weight quantizer (qat_quant.py:126-135)
int fqss_wq_observe(const float* w, int64_t outer, int64_t C, int64_t inner, float* qmin, float* qmax, fqss_stream_t) {
    REQUIRE(w && qmin && qmax && outer > 0 && C > 0 && inner > 0, "bad args");
    for (int64_t c = 0; c < C; ++c) {
        float vmin = INFINITY, vmax = -INFINITY;
        for (int64_t o = 0; o < outer; ++o)
            for (int64_t i = 0; i < inner; ++i) {
                const float v = w[(o * C + c) * inner + i];
                vmin = fminf(vmin, v);
                vmax = fmaxf(vmax, v);
            }
        qmin[c] = vmin;
        qmax[c] = vmax;
    }
    return FQSS_OK;
}

int fqss_wq_fwd_bits(const float* w, float* wq, int8_t* idx, int64_t outer, int64_t C, int64_t inner, const float* qmin, const float* qmax,
                     int n_bits, fqss_stream_t) {
    REQUIRE(w && wq && qmin && qmax && outer > 0 && C > 0 && inner > 0, "bad args");
    REQUIRE(n_bits >= FQSS_WQ_MIN_BITS && n_bits <= FQSS_WQ_MAX_BITS, "weight width outside 2..8 bits");
    const float L = wq_levels(n_bits), qlo = wq_qlo(n_bits), qhi = wq_qhi(n_bits);
    const int64_t n = outer * C * inner;
    for (int64_t e = 0; e < n; ++e) {
        const int64_t c = (e / inner) % C;
        const float delta = wq_delta(qmin[c], qmax[c], L);
        const float q = wq_code(w[e], delta, qlo, qhi);
        wq[e] = delta * q;
        if (idx) idx[e] = (int8_t)q;
    }
    return FQSS_OK;
}

int fqss_wq_fwd(const float* w, float* wq, int8_t* idx, int64_t outer, int64_t C, int64_t inner, const float* qmin, const float* qmax,
                fqss_stream_t s) {
    return fqss_wq_fwd_bits(w, wq, idx, outer, C, inner, qmin, qmax, 8, s);
}

int fqss_wq_bwd_bits(const float* w, const float* g, float* gw, float* gmin, float* gmax, int64_t outer, int64_t C, int64_t inner,
                     const float* qmin, const float* qmax, int accumulate, int n_bits, fqss_stream_t) {
    REQUIRE(w && g && gw && gmin && gmax && qmin && qmax && outer > 0 && C > 0 && inner > 0, "bad args");
    REQUIRE(n_bits >= FQSS_WQ_MIN_BITS && n_bits <= FQSS_WQ_MAX_BITS, "weight width outside 2..8 bits");
    const float L = wq_levels(n_bits), qlo = wq_qlo(n_bits), qhi = wq_qhi(n_bits);
    for (int64_t c = 0; c < C; ++c) {
        const float lo = qmin[c], hi = qmax[c];
        const float delta = wq_delta(lo, hi, L);
        double p = 0.0;
        for (int64_t o = 0; o < outer; ++o)
            for (int64_t i = 0; i < inner; ++i) {
                const int64_t k = (o * C + c) * inner + i;
                const float u = w[k] / delta;
                const float X = nearbyintf(u);
                const bool inr = (X >= qlo) && (X <= qhi);
                const float q = fminf(fmaxf(X, qlo), qhi);
                const float gk = g[k];
                const float gwk = inr ? (gk * delta) / delta : 0.0f;
                gw[k] = accumulate ? gw[k] + gwk : gwk;
                p += (double)(gk * (inr ? (q - u) : q));
            }
        const double D = p * (2.0 / (double)L);
        const float al = fabsf(lo), ah = fabsf(hi);
        const double wl = al > ah ? 1.0 : (al == ah ? 0.5 : 0.0), wh = ah > al ? 1.0 : (al == ah ? 0.5 : 0.0);
        const double sl = lo > 0.0f ? 1.0 : (lo < 0.0f ? -1.0 : 0.0), sh = hi > 0.0f ? 1.0 : (hi < 0.0f ? -1.0 : 0.0);
        const float dmin = (float)(D * wl * sl), dmax = (float)(D * wh * sh);
        gmin[c] = accumulate ? gmin[c] + dmin : dmin;
        gmax[c] = accumulate ? gmax[c] + dmax : dmax;
    }
    return FQSS_OK;
}

int fqss_wq_bwd(const float* w, const float* g, float* gw, float* gmin, float* gmax, int64_t outer, int64_t C, int64_t inner,
                const float* qmin, const float* qmax, int accumulate, fqss_stream_t s) {
    return fqss_wq_bwd_bits(w, g, gw, gmin, gmax, outer, C, inner, qmin, qmax, accumulate, 8, s);
}

// MSE observer (include/fqss.h): candidate 0 is fqss_wq_observe's pair; e_k summed in fp64 in element order, candidates in order
int fqss_wq_observe_mse(const float* w, int64_t outer, int64_t C, int64_t inner, float* qmin, float* qmax, int n_bits, int* k_out,
                        double* err, fqss_stream_t) {
    REQUIRE(w && qmin && qmax && outer > 0 && C > 0 && inner > 0, "bad args");
    REQUIRE(n_bits >= FQSS_WQ_MIN_BITS && n_bits <= FQSS_WQ_MAX_BITS, "weight width outside 2..8 bits");
    const float L = wq_levels(n_bits), qlo = wq_qlo(n_bits), qhi = wq_qhi(n_bits);
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < C; ++c) {
        float lo = INFINITY, hi = -INFINITY;
        for (int64_t o = 0; o < outer; ++o)
            for (int64_t i = 0; i < inner; ++i) {
                const float v = w[(o * C + c) * inner + i];
                lo = fminf(lo, v);
                hi = fmaxf(hi, v);
            }
        const float amax = fmaxf(fabsf(lo), fabsf(hi));
        const int nk = (amax > 0.0f && amax < INFINITY) ? FQSS_WQ_MSE_STEPS : 1;
        double e0 = 0.0, ebest = 0.0;
        int kbest = 0;
        for (int k = 0; k < nk; ++k) {
            const float r = wq_mse_ratio(k);
            const float delta = wq_delta(r * lo, r * hi, L);
            double e = 0.0;
            for (int64_t o = 0; o < outer; ++o)
                for (int64_t i = 0; i < inner; ++i) {
                    const float v = w[(o * C + c) * inner + i];
                    const double d = (double)v - (double)(delta * wq_code(v, delta, qlo, qhi));
                    e += d * d;
                }
            if (k == 0) {
                e0 = ebest = e;
            } else if (e < ebest) {      // strict: ties go to the wider range
                ebest = e;
                kbest = k;
            }
        }
        const float r = wq_mse_ratio(kbest);
        qmin[c] = r * lo;
        qmax[c] = r * hi;
        if (k_out) k_out[c] = kbest;
        if (err) {
            err[2 * c] = e0;
            err[2 * c + 1] = ebest;
        }
    }
    return FQSS_OK;
}

int fqss_wq_error(const float* w, int64_t outer, int64_t C, int64_t inner, const float* qmin, const float* qmax, int n_bits, double* err,
                  double* pow, fqss_stream_t) {
    REQUIRE(w && qmin && qmax && err && pow && outer > 0 && C > 0 && inner > 0, "bad args");
    REQUIRE(n_bits >= FQSS_WQ_MIN_BITS && n_bits <= FQSS_WQ_MAX_BITS, "weight width outside 2..8 bits");
    const float L = wq_levels(n_bits), qlo = wq_qlo(n_bits), qhi = wq_qhi(n_bits);
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < C; ++c) {
        const float delta = wq_delta(qmin[c], qmax[c], L);
        double e = 0.0, p = 0.0;
        for (int64_t o = 0; o < outer; ++o)
            for (int64_t i = 0; i < inner; ++i) {
                const float v = w[(o * C + c) * inner + i];
                const double d = (double)v - (double)(delta * wq_code(v, delta, qlo, qhi));
                e += d * d;
                p += (double)v * (double)v;
            }
        err[c] = e;
        pow[c] = p;
    }
    return FQSS_OK;
}

// ------------------------------------------------------------------------------------------------ pointwise conv (qat_layers.py:137-146)
int fqss_pwconv_fwd(const float* x, const float* w, const float* bias, float* z, int B, int Ci, int Co, int M, int64_t ld_x, int64_t ld_z,
                    fqss_stream_t) {
    if (B == 0 || M == 0) return FQSS_OK;
    REQUIRE(x && w && z && Ci > 0 && Co > 0 && ld_x >= M && ld_z >= M, "bad args");
#pragma omp parallel for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b)
        for (int co = 0; co < Co; ++co) {
            float* zr = z + ((int64_t)b * Co + co) * ld_z;
            const float bv = bias ? bias[co] : 0.0f;
            for (int m = 0; m < M; ++m) zr[m] = bv;
            for (int ci = 0; ci < Ci; ++ci) {
                const float wv = w[(int64_t)co * Ci + ci];
                const float* xr = x + ((int64_t)b * Ci + ci) * ld_x;
                for (int m = 0; m < M; ++m) zr[m] += wv * xr[m];
            }
        }
    return FQSS_OK;
}
int fqss_pwconv_fwd_x3(const float* x, const float* w, const float* bias, float* z, int B, int Ci, int Co, int M, int64_t ld_x,
                       int64_t ld_z, fqss_stream_t s) {
    return fqss_pwconv_fwd(x, w, bias, z, B, Ci, Co, M, ld_x, ld_z, s);
}
int fqss_pwconv_bwd_x(const float* gz, const float* w, float* gx, int B, int Ci, int Co, int M, int64_t ld_gz, int64_t ld_gx, fqss_stream_t) {
    if (B == 0 || M == 0) return FQSS_OK;
    REQUIRE(gz && w && gx && Ci > 0 && Co > 0 && ld_gz >= M && ld_gx >= M, "bad args");
#pragma omp parallel for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b)
        for (int ci = 0; ci < Ci; ++ci) {
            float* gr = gx + ((int64_t)b * Ci + ci) * ld_gx;
            for (int m = 0; m < M; ++m) gr[m] = 0.0f;
            for (int co = 0; co < Co; ++co) {
                const float wv = w[(int64_t)co * Ci + ci];
                const float* zr = gz + ((int64_t)b * Co + co) * ld_gz;
                for (int m = 0; m < M; ++m) gr[m] += wv * zr[m];
            }
        }
    return FQSS_OK;
}
int fqss_pwconv_bwd_w(const float* gz, const float* x, float* gw, int B, int Ci, int Co, int M, int64_t ld_gz, int64_t ld_x, fqss_stream_t) {
    if (B == 0 || M == 0) return FQSS_OK;
    REQUIRE(gz && x && gw && Ci > 0 && Co > 0 && ld_gz >= M && ld_x >= M, "bad args");
#pragma omp parallel for collapse(2) schedule(static)
    for (int co = 0; co < Co; ++co)
        for (int ci = 0; ci < Ci; ++ci) {
            double s = 0.0;
            for (int b = 0; b < B; ++b) {
                const float* zr = gz + ((int64_t)b * Co + co) * ld_gz;
                const float* xr = x + ((int64_t)b * Ci + ci) * ld_x;
                float p = 0.0f;
                for (int m = 0; m < M; ++m) p += zr[m] * xr[m];
                s += (double)p;
            }
            gw[(int64_t)co * Ci + ci] += (float)s;
        }
    return FQSS_OK;
}

// ------------------------------------------------------------------------------------------------ depthwise conv (convtasnetq.py:28-30)
int fqss_dwconv_fwd(const float* x, const float* w, const float* bias, float* z, int B, int C, int M, int K, int dil, int pad, int64_t ld_x,
                    int64_t ld_z, fqss_stream_t) {
    if (B == 0 || M == 0) return FQSS_OK;
    REQUIRE(x && w && z && C > 0 && K > 0 && dil > 0 && 2 * pad == dil * (K - 1), "bad args");
#pragma omp parallel for schedule(static)
    for (int64_t row = 0; row < (int64_t)B * C; ++row) {
        const int c = (int)(row % C);
        const float* xr = x + row * ld_x;
        float* zr = z + row * ld_z;
        for (int m = 0; m < M; ++m) {
            float acc = bias ? bias[c] : 0.0f;
            for (int k = 0; k < K; ++k) {
                const int j = m + k * dil - pad;
                if (j >= 0 && j < M) acc += w[c * K + k] * xr[j];
            }
            zr[m] = acc;
        }
    }
    return FQSS_OK;
}
int fqss_dwconv_bwd_x(const float* gz, const float* w, float* gx, int B, int C, int M, int K, int dil, int pad, int64_t ld_gz, int64_t ld_gx,
                      fqss_stream_t) {
    if (B == 0 || M == 0) return FQSS_OK;
    REQUIRE(gz && w && gx && C > 0 && K > 0 && dil > 0, "bad args");
#pragma omp parallel for schedule(static)
    for (int64_t row = 0; row < (int64_t)B * C; ++row) {
        const int c = (int)(row % C);
        const float* gr = gz + row * ld_gz;
        float* xr = gx + row * ld_gx;
        for (int j = 0; j < M; ++j) {
            float acc = 0.0f;
            for (int k = 0; k < K; ++k) {
                const int m = j - k * dil + pad;
                if (m >= 0 && m < M) acc += w[c * K + k] * gr[m];
            }
            xr[j] = acc;
        }
    }
    return FQSS_OK;
}
int fqss_dwconv_bwd_w(const float* gz, const float* x, float* gw, int B, int C, int M, int K, int dil, int pad, int64_t ld_gz, int64_t ld_x,
                      fqss_stream_t) {
    if (B == 0 || M == 0) return FQSS_OK;
    REQUIRE(gz && x && gw && C > 0 && K > 0 && dil > 0, "bad args");
#pragma omp parallel for schedule(static)
    for (int c = 0; c < C; ++c)
        for (int k = 0; k < K; ++k) {
            double s = 0.0;
            for (int b = 0; b < B; ++b) {
                const float* gr = gz + ((int64_t)b * C + c) * ld_gz;
                const float* xr = x + ((int64_t)b * C + c) * ld_x;
                for (int m = 0; m < M; ++m) {
                    const int j = m + k * dil - pad;
                    if (j >= 0 && j < M) s += (double)(gr[m] * xr[j]);
                }
            }
            gw[c * K + k] += (float)s;
        }
    return FQSS_OK;
}

// ------------------------------------------------------------------------------------------------ GroupNorm(1, C) (qat_layers.py:445-448)
int fqss_gn_fwd(const float* x, const float* gamma, const float* beta, float* z, float* mean_rstd, int B, int C, int M, int64_t ld_x,
                int64_t ld_z, float eps, double* ws, fqss_stream_t) {
    if (B == 0) return FQSS_OK;
    REQUIRE(x && gamma && beta && z && mean_rstd && C > 0 && M > 0 && ld_x >= M && ld_z >= M, "bad args");
    (void)ws;
    for (int b = 0; b < B; ++b) {
        double s = 0.0, ss = 0.0;
        for (int c = 0; c < C; ++c) {
            const float* xr = x + ((int64_t)b * C + c) * ld_x;
            for (int m = 0; m < M; ++m) {
                s += (double)xr[m];
                ss += (double)xr[m] * (double)xr[m];
            }
        }
        const double n = (double)C * M, mu = s / n;
        double var = ss / n - mu * mu;
        if (var < 0.0) var = 0.0;
        const float mean = (float)mu, rstd = (float)(1.0 / sqrt(var + (double)eps));
        mean_rstd[2 * b] = mean;
        mean_rstd[2 * b + 1] = rstd;
        for (int c = 0; c < C; ++c) {
            const float scale = rstd * gamma[c], shift = fmaf(-scale, mean, beta[c]);
            const float* xr = x + ((int64_t)b * C + c) * ld_x;
            float* zr = z + ((int64_t)b * C + c) * ld_z;
            for (int m = 0; m < M; ++m) zr[m] = fmaf(xr[m], scale, shift);
        }
    }
    return FQSS_OK;
}
int fqss_gn_bwd(const float* gz, const float* x, const float* gamma, const float* mean_rstd, float* gx, float* ggamma, float* gbeta, int B,
                int C, int M, int64_t ld_gz, int64_t ld_x, int64_t ld_gx, double* ws, fqss_stream_t) {
    if (B == 0) return FQSS_OK;
    REQUIRE(gz && x && gamma && mean_rstd && gx && ggamma && gbeta && C > 0 && M > 0, "bad args");
    (void)ws;
    std::vector<double> gg((size_t)C, 0.0), gb((size_t)C, 0.0);
    for (int b = 0; b < B; ++b) {
        const float mean = mean_rstd[2 * b], rstd = mean_rstd[2 * b + 1];
        double s1 = 0.0, s2 = 0.0;      // sum gamma*g, sum gamma*g*xhat over the sample
        for (int c = 0; c < C; ++c) {
            const float* gr = gz + ((int64_t)b * C + c) * ld_gz;
            const float* xr = x + ((int64_t)b * C + c) * ld_x;
            double a = 0.0, d = 0.0;
            for (int m = 0; m < M; ++m) {
                const float xh = (xr[m] - mean) * rstd;
                a += (double)gr[m];
                d += (double)(gr[m] * xh);
            }
            gb[(size_t)c] += a;
            gg[(size_t)c] += d;
            s1 += (double)gamma[c] * a;
            s2 += (double)gamma[c] * d;
        }
        const double n = (double)C * M;
        const float m1 = (float)(s1 / n), m2 = (float)(s2 / n);
        for (int c = 0; c < C; ++c) {
            const float* gr = gz + ((int64_t)b * C + c) * ld_gz;
            const float* xr = x + ((int64_t)b * C + c) * ld_x;
            float* or_ = gx + ((int64_t)b * C + c) * ld_gx;
            for (int m = 0; m < M; ++m) {
                const float xh = (xr[m] - mean) * rstd;
                or_[m] = rstd * ((gamma[c] * gr[m] - m1) - xh * m2);
            }
        }
    }
    for (int c = 0; c < C; ++c) {
        ggamma[c] += (float)gg[(size_t)c];
        gbeta[c] += (float)gb[(size_t)c];
    }
    return FQSS_OK;
}

// ------------------------------------------------------------------------------------------------ element-wise producers
int fqss_axpby(const float* a, const float* b, float sa, float sb, float* z, int64_t rows, int64_t cols, int64_t ld_a, int64_t ld_b,
               int64_t ld_z, fqss_stream_t) {
    if (rows == 0 || cols == 0) return FQSS_OK;
    REQUIRE(a && b && z, "null tensor");
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t c = 0; c < cols; ++c) z[r * ld_z + c] = sa * a[r * ld_a + c] + sb * b[r * ld_b + c];
    return FQSS_OK;
}
int fqss_mul_bcast_fwd(const float* mask, const float* feat, float* z, int B, int S, int C, int M, int64_t ld_mask, int64_t ld_feat,
                       int64_t ld_z, fqss_stream_t) {
    if (B == 0 || M == 0) return FQSS_OK;
    REQUIRE(mask && feat && z, "null tensor");
    for (int b = 0; b < B; ++b)
        for (int s = 0; s < S; ++s)
            for (int c = 0; c < C; ++c) {
                const int64_t r = ((int64_t)b * S + s) * C + c;
                const float* fr = feat + ((int64_t)b * C + c) * ld_feat;
                for (int m = 0; m < M; ++m) z[r * ld_z + m] = mask[r * ld_mask + m] * fr[m];
            }
    return FQSS_OK;
}
int fqss_mul_bcast_bwd(const float* gz, const float* mask, const float* feat, float* gmask, float* gfeat, int B, int S, int C, int M,
                       int64_t ld_gz, int64_t ld_mask, int64_t ld_feat, int64_t ld_gmask, int64_t ld_gfeat, fqss_stream_t) {
    if (B == 0 || M == 0) return FQSS_OK;
    REQUIRE(gz && mask && feat && gmask && gfeat, "null tensor");
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c) {
            const float* fr = feat + ((int64_t)b * C + c) * ld_feat;
            float* gf = gfeat + ((int64_t)b * C + c) * ld_gfeat;
            for (int m = 0; m < M; ++m) gf[m] = 0.0f;
            for (int s = 0; s < S; ++s) {      // ascending s, like the kernel
                const int64_t r = ((int64_t)b * S + s) * C + c;
                for (int m = 0; m < M; ++m) {
                    const float gv = gz[r * ld_gz + m];
                    gmask[r * ld_gmask + m] = gv * fr[m];
                    gf[m] += gv * mask[r * ld_mask + m];
                }
            }
        }
    return FQSS_OK;
}

// ------------------------------------------------------------------------------------------------ splitter, framing conv, overlap-add
static inline float split_clip(float v) {   // torch.clip(v, -128, 127): a NaN (the 0 / 0 of a silent row) stays NaN
    v = v < -128.0f ? -128.0f : v;
    return v > 127.0f ? 127.0f : v;
}
static inline float split_q(float x) {      // process.py:10-14 with threshold = 1, n_bits = 8, sign = True
    const float delta = 0.0078125f;
    return split_clip(floorf(x / delta)) * delta;
}
static inline void split2(float x, float thr, float& msb, float& lsb) {      // process.py:22-36
    const float delta = 0.0078125f;
    const float v = x / thr;
    const float q0 = split_q(v);
    const float r = ((2.0f * (v - q0)) * 1.0f) / delta - 1.0f;          // process.py:35 op order
    msb = q0;
    lsb = split_q(r);
}
int fqss_splitter2(const float* x, float* out, int B, int64_t T, const uint32_t* obs_ws, fqss_stream_t) {
    if (B == 0 || T == 0) return FQSS_OK;
    REQUIRE(x && out && obs_ws, "null pointer");
    const float thr = fmaxf(fabsf(ord2f(obs_ws[0])), fabsf(ord2f(obs_ws[1])));   // process.py:24
    for (int64_t b = 0; b < B; ++b)
        for (int64_t t = 0; t < T; ++t) split2(x[b * T + t], thr, out[(b * 2 + 0) * T + t], out[(b * 2 + 1) * T + t]);
    return FQSS_OK;
}
// one threshold per row (the reference calls the model chunk by chunk); row_max: B words zeroed by the caller, left holding the bit
// images of max|x[b][:]| as the HIP library leaves them
int fqss_splitter2_rows(const float* x, float* out, int B, int64_t T, uint32_t* row_max, fqss_stream_t) {
    REQUIRE(x && out && row_max, "null pointer");
    REQUIRE(B > 0 && T > 0, "bad shape");
    for (int64_t b = 0; b < B; ++b) {
        float thr;
        memcpy(&thr, &row_max[b], 4);
        for (int64_t t = 0; t < T; ++t) thr = fmaxf(thr, fabsf(x[b * T + t]));
        memcpy(&row_max[b], &thr, 4);
        for (int64_t t = 0; t < T; ++t) split2(x[b * T + t], thr, out[(b * 2 + 0) * T + t], out[(b * 2 + 1) * T + t]);
    }
    return FQSS_OK;
}
int fqss_frames_conv_fwd(const float* x, const float* w, float* z, int N, int Ci, int Co, int64_t T, int K, int stride, int M, int64_t ld_z,
                         fqss_stream_t) {
    if (N == 0 || M == 0) return FQSS_OK;
    REQUIRE(x && w && z && Ci > 0 && Co > 0 && K > 0 && stride > 0 && (int64_t)(M - 1) * stride + K <= T && ld_z >= M, "bad args");
#pragma omp parallel for collapse(2) schedule(static)
    for (int n = 0; n < N; ++n)
        for (int co = 0; co < Co; ++co)
            for (int m = 0; m < M; ++m) {
                float acc = 0.0f;
                for (int ci = 0; ci < Ci; ++ci) {
                    const float* xp = x + ((int64_t)n * Ci + ci) * T + (int64_t)m * stride;
                    const float* wr = w + ((int64_t)co * Ci + ci) * K;
                    for (int k = 0; k < K; ++k) acc = fmaf(xp[k], wr[k], acc);      // the kernel's j-ordered fmaf chain
                }
                z[((int64_t)n * Co + co) * ld_z + m] = acc;
            }
    return FQSS_OK;
}
int fqss_ola_convtr_fwd(const float* x, const float* w, float* out, int N, int C, int M, int64_t ld_x, int K, int stride, int64_t T,
                        fqss_stream_t) {
    if (N == 0 || M == 0) return FQSS_OK;
    REQUIRE(x && w && out && C > 0 && K > 0 && stride > 0 && T == (int64_t)(M - 1) * stride + K && ld_x >= M, "T must equal (M-1)*stride + K");
#pragma omp parallel for schedule(static)
    for (int n = 0; n < N; ++n) {
        std::vector<double> acc((size_t)T, 0.0);
        for (int c = 0; c < C; ++c) {
            const float* xr = x + ((int64_t)n * C + c) * ld_x;
            for (int m = 0; m < M; ++m)
                for (int k = 0; k < K; ++k) acc[(size_t)((int64_t)m * stride + k)] += (double)(xr[m] * w[c * K + k]);
        }
        for (int64_t t = 0; t < T; ++t) out[(int64_t)n * T + t] = (float)acc[(size_t)t];
    }
    return FQSS_OK;
}
int fqss_frames_wgrad1s(const float* a, const float* sig, int64_t sig_ns, float* gw, int64_t ld_gw, int N, int C, int M, int64_t ld_a,
                        int64_t T, int K, int stride, fqss_stream_t) {
    if (N == 0 || M == 0) return FQSS_OK;
    REQUIRE(a && sig && gw && C > 0 && K > 0 && stride > 0 && ld_a >= M && (int64_t)(M - 1) * stride + K <= T && sig_ns >= T && ld_gw >= K,
            "bad args");
#pragma omp parallel for schedule(static)
    for (int c = 0; c < C; ++c)
        for (int k = 0; k < K; ++k) {
            double s = 0.0;
            for (int n = 0; n < N; ++n) {
                const float* ar = a + ((int64_t)n * C + c) * ld_a;
                const float* sr = sig + (int64_t)n * sig_ns + k;
                for (int m = 0; m < M; ++m) s += (double)(ar[m] * sr[(int64_t)m * stride]);
            }
            gw[(int64_t)c * ld_gw + k] += (float)s;
        }
    return FQSS_OK;
}
int fqss_frames_wgrad1(const float* a, const float* sig, float* gw, int N, int C, int M, int64_t ld_a, int64_t T, int K, int stride,
                       fqss_stream_t s) {
    return fqss_frames_wgrad1s(a, sig, T, gw, K, N, C, M, ld_a, T, K, stride, s);
}
int fqss_frames_wgrad(const float* a, const float* x, float* gw, int N, int C, int Ci, int M, int64_t ld_a, int64_t T, int K, int stride,
                      fqss_stream_t s) {
    for (int ci = 0; ci < Ci; ++ci) {
        const int rc = fqss_frames_wgrad1s(a, x + (int64_t)ci * T, (int64_t)Ci * T, gw + (int64_t)ci * K, (int64_t)Ci * K, N, C, M, ld_a, T, K,
                                           stride, s);
        if (rc) return rc;
    }
    return FQSS_OK;
}

// ------------------------------------------------------------------------------------------------ KD loss (mysystem.py:124-151, wsdr.py:56-95)
namespace {
constexpr double kEps = 1e-8;
struct PairSdr {
    double sdr, cx, cy;
};
PairSdr pair_sdr(double Sx, double Sy, double Sxx, double Syy, double Sxy, double T) {
    const double X2 = Sxx - Sx * Sx / T, Y2 = Syy - Sy * Sy / T, D = Sxy - Sx * Sy / T;
    const double E = Y2 + kEps, alpha = D / E, P = alpha * alpha * Y2;
    double Nn = X2 - 2.0 * alpha * D + alpha * alpha * Y2;
    if (Nn < 0.0) Nn = 0.0;
    const double den = Nn + kEps;
    PairSdr r;
    r.sdr = P / den;
    r.cx = -2.0 * P / (den * den);
    r.cy = 2.0 * alpha * Y2 / (E * den) + P * (2.0 * alpha + 2.0 * D * kEps / (E * E)) / (den * den);
    return r;
}
}  // namespace

int fqss_kd_loss(const float* est, const float* fest, const float* tgt, int B, int64_t T, float kd_lambda, double* stats, float* out,
                 float* w_out, float* sisdr_out, float* gest, fqss_stream_t) {
    REQUIRE(est && fest && tgt && out && w_out && sisdr_out && B > 0 && T > 0, "bad args");
    (void)stats;
    struct Smp {
        double m[24];
        PairSdr st[2][2], sf[2][2];
        int pt, pf;
        double task, kd, w;
    };
    std::vector<Smp> S((size_t)B);
    double task = 0.0, kd = 0.0;
    const double Td = (double)T;
    for (int b = 0; b < B; ++b) {
        Smp& q = S[(size_t)b];
        for (int i = 0; i < 24; ++i) q.m[i] = 0.0;
        const float* sig[6] = {est + (int64_t)b * 2 * T,  est + (int64_t)b * 2 * T + T, fest + (int64_t)b * 2 * T, fest + (int64_t)b * 2 * T + T,
                               tgt + (int64_t)b * 2 * T,  tgt + (int64_t)b * 2 * T + T};
        for (int64_t t = 0; t < T; ++t) {
            double s[6];
            for (int i = 0; i < 6; ++i) s[i] = (double)sig[i][t];
            for (int i = 0; i < 6; ++i) {
                q.m[i] += s[i];
                q.m[6 + i] += s[i] * s[i];
            }
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) {
                    q.m[12 + i * 2 + j] += s[i] * s[4 + j];
                    q.m[16 + i * 2 + j] += s[i] * s[2 + j];
                    q.m[20 + i * 2 + j] += s[2 + i] * s[4 + j];
                }
        }
        const double* m = q.m;
        double nl_ft[2][2], nl_et[2][2];
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) {
                q.st[i][j] = pair_sdr(m[i], m[4 + j], m[6 + i], m[10 + j], m[12 + i * 2 + j], Td);
                q.sf[i][j] = pair_sdr(m[i], m[2 + j], m[6 + i], m[8 + j], m[16 + i * 2 + j], Td);
                const PairSdr ft = pair_sdr(m[2 + i], m[4 + j], m[8 + i], m[10 + j], m[20 + i * 2 + j], Td);
                nl_ft[i][j] = -10.0 * log10(ft.sdr + kEps);
                nl_et[i][j] = -10.0 * log10(q.st[i][j].sdr + kEps);
            }
        // PIT (pw_mtx): p0 = (0,1), p1 = (1,0); torch.min keeps the first on ties
        const double lf0 = 0.5 * (nl_ft[0][0] + nl_ft[1][1]), lf1 = 0.5 * (nl_ft[1][0] + nl_ft[0][1]);
        const double le0 = 0.5 * (nl_et[0][0] + nl_et[1][1]), le1 = 0.5 * (nl_et[1][0] + nl_et[0][1]);
        const double sdrs = lf1 < lf0 ? lf1 : lf0, sdrqs = le1 < le0 ? le1 : le0;
        q.w = pow(10.0, (sdrs - sdrqs) / 10.0);     // mysystem.py:141
        const double t0 = -0.5 * (q.st[0][0].sdr + q.st[1][1].sdr), t1 = -0.5 * (q.st[1][0].sdr + q.st[0][1].sdr);
        q.pt = t1 < t0 ? 1 : 0;
        q.task = -(q.pt ? t1 : t0);
        const double k0 = -0.5 * q.w * (q.sf[0][0].sdr + q.sf[1][1].sdr), k1 = -0.5 * q.w * (q.sf[1][0].sdr + q.sf[0][1].sdr);
        q.pf = k1 < k0 ? 1 : 0;
        q.kd = -(q.pf ? k1 : k0);
        w_out[b] = (float)q.w;
        sisdr_out[b] = (float)(-sdrqs);
        task += q.task;
        kd += q.kd;
    }
    task /= (double)B;
    kd /= (double)B;
    const double lam = (double)kd_lambda, arg = (1.0 - lam) * task + lam * kd + kEps;
    out[0] = (float)(-10.0 * log10(arg));
    out[1] = (float)(-10.0 * log10(kd + kEps));
    out[2] = (float)task;
    out[3] = (float)kd;
    if (gest) {
        const double dL = -10.0 / (log(10.0) * arg);
        for (int b = 0; b < B; ++b) {
            const Smp& q = S[(size_t)b];
            const double gt = dL * (1.0 - lam) / (2.0 * (double)B), gk = dL * lam * q.w / (2.0 * (double)B);
            for (int i = 0; i < 2; ++i) {
                const int jt = q.pt ? 1 - i : i, jf = q.pf ? 1 - i : i;
                const float A = (float)(gt * q.st[i][jt].cx + gk * q.sf[i][jf].cx), Bt = (float)(gt * q.st[i][jt].cy),
                            Bf = (float)(gk * q.sf[i][jf].cy);
                const float me = (float)(q.m[i] / Td), mt = (float)(q.m[4 + jt] / Td), mf = (float)(q.m[2 + jf] / Td);
                const float* e = est + ((int64_t)b * 2 + i) * T;
                const float* tt = tgt + ((int64_t)b * 2 + jt) * T;
                const float* ff = fest + ((int64_t)b * 2 + jf) * T;
                float* g = gest + ((int64_t)b * 2 + i) * T;
                for (int64_t t = 0; t < T; ++t) g[t] = A * (e[t] - me) + Bt * (tt[t] - mt) + Bf * (ff[t] - mf);
            }
        }
    }
    return FQSS_OK;
}

// the loss for n_src = S in 1..3 (include/fqss.h: fqss_kd_loss_n), a plain fp64 restatement of csrc/train_ops.hip's k_kd_*_n: the
// moment row, the four PIT reductions over itertools.permutations order (first wins ties), the three modes, the gradient map
namespace {
void kd_moments_row(const float* est, const float* fest, const float* tgt, int b, int S, int64_t T, double* m) {
    const int NM = 6 * S + 3 * S * S;
    for (int i = 0; i < NM; ++i) m[i] = 0.0;
    const float* sig[9];
    for (int i = 0; i < S; ++i) {
        sig[i] = est + ((int64_t)b * S + i) * T;
        sig[S + i] = fest + ((int64_t)b * S + i) * T;
        sig[2 * S + i] = tgt + ((int64_t)b * S + i) * T;
    }
    for (int64_t t = 0; t < T; ++t) {
        double s[9];
        for (int i = 0; i < 3 * S; ++i) s[i] = (double)sig[i][t];
        for (int i = 0; i < 3 * S; ++i) {
            m[i] += s[i];
            m[3 * S + i] += s[i] * s[i];
        }
        for (int i = 0; i < S; ++i)
            for (int j = 0; j < S; ++j) {
                m[6 * S + i * S + j] += s[i] * s[2 * S + j];
                m[6 * S + S * S + i * S + j] += s[i] * s[S + j];
                m[6 * S + 2 * S * S + i * S + j] += s[S + i] * s[2 * S + j];
            }
    }
}
}  // namespace

int fqss_kd_moments_n(const float* est, const float* fest, const float* tgt, int B, int S, int64_t T, double* stats, fqss_stream_t) {
    REQUIRE(est && fest && tgt && stats, "null tensor");
    REQUIRE(S >= 1 && S <= 3, "n_src must be in 1..3");
    REQUIRE(B > 0 && B <= 1024 && T > 0, "B must be in 1..1024");
    for (int b = 0; b < B; ++b) {
        double* m = stats + (int64_t)b * FQSS_KD_STATS_STRIDE_N;
        for (int i = 0; i < FQSS_KD_STATS_STRIDE_N; ++i) m[i] = 0.0;
        kd_moments_row(est, fest, tgt, b, S, T, m);
    }
    return FQSS_OK;
}

int fqss_kd_loss_n(const float* est, const float* fest, const float* tgt, int B, int S, int64_t T, float kd_lambda, int mode,
                   int use_threshold, float threshold, double* stats, float* out, float* w_out, float* sisdr_out, float* gest,
                   fqss_stream_t) {
    REQUIRE(est && fest && tgt && stats && out && w_out && sisdr_out, "null tensor");
    REQUIRE(S >= 1 && S <= 3, "n_src must be in 1..3");
    REQUIRE(B > 0 && B <= 1024 && T > 0, "B must be in 1..1024");
    REQUIRE(mode >= 0 && mode <= 2, "mode must be 0 (asteroid), 1 (per sample) or 2 (teacher-free PIT SI-SDR)");
    REQUIRE(mode != 1 || B == 1 || B == S,
            "the per-sample KD weights broadcast [1, n_src, n_src] * [1, B]: B must be 1 or n_src (the reference raises otherwise)");
    std::vector<std::vector<int>> perms;
    {
        std::vector<int> p((size_t)S);
        for (int i = 0; i < S; ++i) p[(size_t)i] = i;
        do perms.push_back(p);
        while (std::next_permutation(p.begin(), p.end()));      // lexicographic = itertools.permutations(range(S))
    }
    const int oET = 6 * S, oEF = 6 * S + S * S, oFT = 6 * S + 2 * S * S;
    const double Td = (double)T, lam = (double)kd_lambda;
    struct Smp {
        double rt[3][3], rf[3][3], w, task, kd, pit_db;
        int pt, pf;
    };
    std::vector<Smp> smp((size_t)B);
    for (int b = 0; b < B; ++b) {
        double* m = stats + (int64_t)b * FQSS_KD_STATS_STRIDE_N;
        for (int i = 0; i < FQSS_KD_STATS_STRIDE_N; ++i) m[i] = 0.0;
        kd_moments_row(est, fest, tgt, b, S, T, m);
        Smp& q = smp[(size_t)b];
        double nl_ft[3][3], nl_et[3][3];
        for (int i = 0; i < S; ++i)
            for (int j = 0; j < S; ++j) {
                q.rt[i][j] = pair_sdr(m[i], m[2 * S + j], m[3 * S + i], m[5 * S + j], m[oET + i * S + j], Td).sdr;
                q.rf[i][j] = pair_sdr(m[i], m[S + j], m[3 * S + i], m[4 * S + j], m[oEF + i * S + j], Td).sdr;
                const double ft = pair_sdr(m[S + i], m[2 * S + j], m[4 * S + i], m[5 * S + j], m[oFT + i * S + j], Td).sdr;
                nl_ft[i][j] = -10.0 * log10(ft + kEps);
                nl_et[i][j] = -10.0 * log10(q.rt[i][j] + kEps);
            }
        double sdrs = 0.0, sdrqs = 0.0, tbest = 0.0;
        int pe = 0;
        q.pt = 0;
        for (size_t k = 0; k < perms.size(); ++k) {
            const std::vector<int>& p = perms[k];
            double lf = 0.0, le = 0.0, tq = 0.0;
            for (int i = 0; i < S; ++i) {
                lf += nl_ft[p[(size_t)i]][i];
                le += nl_et[p[(size_t)i]][i];
                tq += q.rt[p[(size_t)i]][i];
            }
            lf /= (double)S;
            le /= (double)S;
            tq = -tq / (double)S;
            if (k == 0 || lf < sdrs) sdrs = lf;
            if (k == 0 || le < sdrqs) sdrqs = le, pe = (int)k;
            if (k == 0 || tq < tbest) tbest = tq, q.pt = (int)k;
        }
        q.w = pow(10.0, (sdrs - sdrqs) / 10.0);
        q.task = -tbest;
        q.pit_db = sdrqs;
        if (mode == 2) q.pt = pe;
        w_out[b] = (float)q.w;
        sisdr_out[b] = (float)(-sdrqs);
    }
    double task = 0.0, kd = 0.0;
    for (int b = 0; b < B; ++b) {
        Smp& q = smp[(size_t)b];
        double kbest = 0.0;
        q.pf = 0;
        for (size_t k = 0; k < perms.size(); ++k) {
            const std::vector<int>& p = perms[k];
            double kq = 0.0;
            for (int i = 0; i < S; ++i) {
                const int j = p[(size_t)i];     // student source j on teacher source i
                kq += ((mode == 1 && B == S) ? smp[(size_t)j].w : q.w) * q.rf[j][i];
            }
            kq = -kq / (double)S;
            if (k == 0 || kq < kbest) kbest = kq, q.pf = (int)k;
        }
        q.kd = -kbest;
        task += q.task;
        kd += q.kd;
    }
    task /= (double)B;
    kd /= (double)B;
    std::vector<double> gt((size_t)B, 0.0), gkw((size_t)B, 0.0);     // the KD coefficient of student source j is gkw * (its weight)
    if (mode == 2) {
        double l = 0.0;
        for (int b = 0; b < B; ++b) l += smp[(size_t)b].pit_db;
        out[0] = (float)(l / (double)B);
        out[1] = 0.0f;
        out[2] = (float)task;
        out[3] = 0.0f;
    } else if (mode == 0) {
        const double arg = (1.0 - lam) * task + lam * kd + kEps, dL = -10.0 / (log(10.0) * arg);
        out[0] = (float)(-10.0 * log10(arg));
        out[1] = (float)(-10.0 * log10(kd + kEps));
        out[2] = (float)task;
        out[3] = (float)kd;
        for (int b = 0; b < B; ++b) {
            gt[(size_t)b] = dL * (1.0 - lam) / ((double)S * (double)B);
            gkw[(size_t)b] = dL * lam / ((double)S * (double)B);
        }
    } else {
        std::vector<double> arg_b((size_t)B), loss_b((size_t)B);
        int nkeep = 0;
        for (int b = 0; b < B; ++b) {
            arg_b[(size_t)b] = (1.0 - lam) * smp[(size_t)b].task + lam * smp[(size_t)b].kd + kEps;
            loss_b[(size_t)b] = -10.0 * log10(arg_b[(size_t)b]);
            if (!use_threshold || loss_b[(size_t)b] > (double)threshold) ++nkeep;
        }
        const double cnt = (double)(nkeep == 0 ? B : nkeep);
        double l = 0.0;
        for (int b = 0; b < B; ++b) {
            const bool keep = nkeep == 0 || !use_threshold || loss_b[(size_t)b] > (double)threshold;
            if (!keep) continue;
            l += loss_b[(size_t)b];
            const double dL = -10.0 / (log(10.0) * arg_b[(size_t)b]) / cnt;
            gt[(size_t)b] = dL * (1.0 - lam) / (double)S;
            gkw[(size_t)b] = dL * lam / (double)S;
        }
        out[0] = (float)(l / cnt);
        out[1] = (float)(-10.0 * log10(kd + kEps));
        out[2] = (float)task;
        out[3] = (float)kd;
    }
    for (int b = 0; b < B; ++b) {
        const Smp& q = smp[(size_t)b];
        double* m = stats + (int64_t)b * FQSS_KD_STATS_STRIDE_N;
        for (int i = 0; i < 3 * S; ++i) m[48 + i] = m[i] / Td;
        for (int i = 0; i < S; ++i) {
            int jt = 0, jf = 0;     // estimate i sits on signal j with p[j] == i (the inverse map)
            for (int j = 0; j < S; ++j) {
                if (perms[(size_t)q.pt][(size_t)j] == i) jt = j;
                if (perms[(size_t)q.pf][(size_t)j] == i) jf = j;
            }
            const PairSdr a = pair_sdr(m[i], m[2 * S + jt], m[3 * S + i], m[5 * S + jt], m[oET + i * S + jt], Td);
            const PairSdr c = pair_sdr(m[i], m[S + jf], m[3 * S + i], m[4 * S + jf], m[oEF + i * S + jf], Td);
            const double gti = (mode == 2) ? -10.0 / (log(10.0) * (a.sdr + kEps)) / (double)S / (double)B : gt[(size_t)b];
            const double gki = gkw[(size_t)b] * ((mode == 1 && B == S) ? smp[(size_t)i].w : q.w);
            double* cf = m + 57 + 5 * i;
            cf[0] = gti * a.cx + gki * c.cx;
            cf[1] = gti * a.cy;
            cf[2] = (double)jt;
            cf[3] = gki * c.cy;
            cf[4] = (double)jf;
            if (!gest) continue;
            const float A = (float)cf[0], Bt = (float)cf[1], Bf = (float)cf[3];
            const float me = (float)m[48 + i], mt = (float)m[48 + 2 * S + jt], mf = (float)m[48 + S + jf];
            const float* e = est + ((int64_t)b * S + i) * T;
            const float* tt = tgt + ((int64_t)b * S + jt) * T;
            const float* ff = fest + ((int64_t)b * S + jf) * T;
            float* g = gest + ((int64_t)b * S + i) * T;
            for (int64_t t = 0; t < T; ++t) g[t] = A * (e[t] - me) + Bt * (tt[t] - mt) + Bf * (ff[t] - mf);
        }
    }
    return FQSS_OK;
}

// ------------------------------------------------------------------------------------------------ clip + Adam (torch.optim.Adam, clip_grad_norm_)
int fqss_sumsq(const float* g, int64_t n, double* sumsq, fqss_stream_t) {
    REQUIRE(g && sumsq && n >= 0, "bad args");
    double s = 0.0;
#pragma omp parallel for reduction(+ : s) schedule(static)
    for (int64_t i = 0; i < n; ++i) s += (double)g[i] * (double)g[i];
    *sumsq += s;
    return FQSS_OK;
}
int fqss_adam_clip(float* p, const float* g, float* m, float* v, int64_t n, const double* sumsq, float max_norm, float grad_scale, float lr,
                   float beta1, float beta2, float eps, int32_t* step_t, const int32_t* t0, float* gnorm_out, fqss_stream_t) {
    REQUIRE(p && g && m && v && sumsq && step_t && n >= 0, "bad args");
    const int tg = *step_t + 1;
    const double norm = sqrt(*sumsq) * (double)grad_scale;
    double coef = (double)max_norm / (norm + 1e-6);
    if (coef > 1.0) coef = 1.0;
    if (max_norm <= 0.0f) coef = 1.0;
    const float gs = (float)((double)grad_scale * coef);
    const float omb1 = (float)(1.0 - (double)beta1), omb2 = (float)(1.0 - (double)beta2);
    int cached = -1;
    float step_size = 0.0f, bc2_sqrt = 1.0f;
    for (int64_t i = 0; i < n; ++i) {
        const int t = tg - (t0 ? t0[i] : 0);
        if (t <= 0) continue;
        if (t != cached) {
            const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
            step_size = (float)((double)lr / bc1);
            bc2_sqrt = (float)sqrt(bc2);
            cached = t;
        }
        const float gi = g[i] * gs;
        const float mi = m[i] + omb1 * (gi - m[i]);
        const float vi = v[i] * beta2 + (omb2 * gi) * gi;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] = p[i] + ((-step_size) * mi) / denom;
    }
    *step_t = tg;
    if (gnorm_out) *gnorm_out = (float)norm;
    return FQSS_OK;
}
// the optimizer family on the same clip and clocks (fqss.h: fqss_optim_clip; the op sequence of csrc/train_ops.hip k_optim_clip)
int fqss_optim_clip(float* p, const float* g, float* m, float* v, int64_t n, const double* sumsq, float max_norm, float grad_scale, float lr,
                    float beta1, float beta2, float eps, int32_t* step_t, const int32_t* t0, float* gnorm_out, int kind, float weight_decay,
                    const float* wd_slot, float momentum, int nesterov, fqss_stream_t) {
    REQUIRE(kind == FQSS_OPT_ADAM || kind == FQSS_OPT_ADAMW || kind == FQSS_OPT_SGD, "kind: FQSS_OPT_ADAM, FQSS_OPT_ADAMW or FQSS_OPT_SGD");
    REQUIRE(p && g && sumsq && step_t && n >= 0, "bad args");
    REQUIRE(weight_decay >= 0.0f, "weight_decay must be >= 0");
    REQUIRE(momentum >= 0.0f && momentum < 1.0f, "momentum must lie in [0, 1)");
    REQUIRE(nesterov == 0 || (nesterov == 1 && momentum > 0.0f), "nesterov: 0 or 1, and 1 needs a momentum > 0");
    REQUIRE(kind == FQSS_OPT_SGD ? (m || momentum == 0.0f) : (m && v), "null moment buffer");
    REQUIRE(!wd_slot || n % 64 == 0, "a decay table needs n to be a multiple of 64 floats");
    const bool adam = kind != FQSS_OPT_SGD, use_buf = !adam && momentum != 0.0f;
    const float mu = momentum;
    const int tg = *step_t + 1;
    const double norm = sqrt(*sumsq) * (double)grad_scale;
    double coef = (double)max_norm / (norm + 1e-6);
    if (coef > 1.0) coef = 1.0;
    if (max_norm <= 0.0f) coef = 1.0;
    const float gs = (float)((double)grad_scale * coef);
    const float omb1 = (float)(1.0 - (double)beta1), omb2 = (float)(1.0 - (double)beta2);
    int cached = -1;
    float step_size = 0.0f, bc2_sqrt = 1.0f;
    for (int64_t i = 0; i < n; ++i) {
        const int t = tg - (t0 ? t0[i] : 0);
        if (t <= 0) continue;
        const float wd = wd_slot ? wd_slot[i >> 6] : weight_decay;
        float gi = g[i] * gs, pi = p[i];
        if (kind == FQSS_OPT_ADAMW) {
            if (wd != 0.0f) pi = pi * (float)(1.0 - (double)lr * (double)wd);
        } else if (wd != 0.0f) {
            gi = fmaf(wd, pi, gi);      // add(alpha=): one rounding in torch's kernels
        }
        if (adam) {
            if (t != cached) {
                const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
                step_size = (float)((double)lr / bc1);
                bc2_sqrt = (float)sqrt(bc2);
                cached = t;
            }
            const float mi = m[i] + omb1 * (gi - m[i]);
            const float vi = v[i] * beta2 + (omb2 * gi) * gi;
            m[i] = mi;
            v[i] = vi;
            const float denom = sqrtf(vi) / bc2_sqrt + eps;
            p[i] = pi + ((-step_size) * mi) / denom;
        } else {
            float d = gi;
            if (use_buf) {
                const float buf = (t == 1) ? gi : m[i] * mu + gi;
                m[i] = buf;
                d = nesterov ? fmaf(mu, buf, gi) : buf;
            }
            p[i] = fmaf(-lr, d, pi);
        }
    }
    *step_t = tg;
    if (gnorm_out) *gnorm_out = (float)norm;
    return FQSS_OK;
}
// EMA copies (fqss.h: fqss_ema_update / fqss_ema_update_dev; `count` is host memory on this backend)
static void ema_apply(float* ema, const float* p, int64_t n, double wd) {
    const float w = (float)wd, omw = (float)(1.0 - wd);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i) ema[i] = ema[i] * omw + w * p[i];
}
int fqss_ema_update(float* ema, const float* p, int64_t n, float w, fqss_stream_t) {
    REQUIRE(ema && p && n >= 0, "null pointer");
    REQUIRE(w >= 0.0f && w <= 1.0f, "w must lie in [0, 1]");
    REQUIRE(ema + n <= p || p + n <= ema, "ema and p overlap");
    ema_apply(ema, p, n, (double)w);
    return FQSS_OK;
}
int fqss_ema_update_dev(float* ema, const float* p, int64_t n, double decay, double* count, fqss_stream_t) {
    REQUIRE(ema && p && count && n >= 0, "null pointer");
    REQUIRE(decay >= 0.0 && decay < 1.0, "decay must lie in [0, 1)");
    REQUIRE(ema + n <= p || p + n <= ema, "ema and p overlap");
    if (n == 0) return FQSS_OK;
    *count = *count * decay + 1.0;
    ema_apply(ema, p, n, 1.0 / *count);
    return FQSS_OK;
}
// gradient accumulation: the moves between the gradient arena and the window's accumulator (same contract as the HIP entry point)
int fqss_grad_accum(float* acc, float* g, int64_t n, int mode, fqss_stream_t) {
    REQUIRE(acc && g, "null pointer");
    REQUIRE(mode >= 0 && mode <= 3, "mode: 0 (acc = g), 1 (acc += g), 2 (g += acc) or 3 (g = acc)");
    REQUIRE(n >= 0 && n % 4 == 0 && ((uintptr_t)acc & 15u) == 0 && ((uintptr_t)g & 15u) == 0,
            "n must be a multiple of 4 floats and both pointers 16-B aligned");
    REQUIRE(acc + n <= g || g + n <= acc, "acc and g overlap");
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i) {
        if (mode == 0) acc[i] = g[i];
        else if (mode == 1) acc[i] = acc[i] + g[i];
        else if (mode == 2) g[i] = acc[i] + g[i];
        else g[i] = acc[i];
    }
    return FQSS_OK;
}

// ------------------------------------------------------------------------------------------------ data side (LibriMix dataset, librimix_dataset.py:54, 139-153)
// the op sequences of csrc/data_ops.hip: energies in fp64, gains in fp32 (process.py:77-103), max_clip(0.9) (process.py:57-62)
int fqss_snr_mix(const float* a, const float* b, const float* snr, double* ws, uint32_t* peak, float* out, int64_t B, int64_t T, int64_t ld_a,
                 int64_t ld_b, int64_t ld_o, int mode, int clip, fqss_stream_t) {
    REQUIRE(a && b && snr && ws && peak && out, "null pointer");
    REQUIRE(B > 0 && T > 0 && ld_a >= T && ld_b >= T && ld_o >= T && (mode == 0 || mode == 1), "bad shape");
#pragma omp parallel for schedule(static)
    for (int64_t r = 0; r < B; ++r) {
        double ea = 0.0, eb = 0.0;
        for (int64_t i = 0; i < T; ++i) {
            const double x = a[r * ld_a + i], y = b[r * ld_b + i];
            ea += x * x;
            eb += y * y;
        }
        ws[2 * r] += ea;
        ws[2 * r + 1] += eb;
        const float Ea = (float)(ws[2 * r] / (double)T), Eb = (float)(ws[2 * r + 1] / (double)T);
        float ga = 1.0f, gb = 1.0f;
        if (mode == 0) {
            if (Ea > 0.0f && Eb > 0.0f) {
                const float now = 10.0f * log10f(Ea / Eb);
                if (now < snr[r]) gb = sqrtf((Ea / Eb) * powf(10.0f, -snr[r] / 10.0f));
                else ga = sqrtf((Eb / Ea) * powf(10.0f, snr[r] / 10.0f));
            }
        } else if (Ea > 0.0f) {
            gb = sqrtf((Ea / Eb) / powf(10.0f, snr[r] / 10.0f));
        }
        float mx = 0.0f;
        for (int64_t i = 0; i < T; ++i) {
            const float m = a[r * ld_a + i] * ga + b[r * ld_b + i] * gb;
            out[r * ld_o + i] = m;
            mx = fmaxf(mx, fabsf(m));
        }
        memcpy(&peak[r], &mx, 4);
        if (clip && mx >= 0.9f) {
            const float gain = 0.9f / mx;
            for (int64_t i = 0; i < T; ++i) out[r * ld_o + i] *= gain;
        }
    }
    return FQSS_OK;
}

// y[r][n * newf + p] = sum_k h[p][k] * xpad[r][n * orig + k]: one fma per tap, in tap order (the HIP kernel's chain)
int fqss_resample_fir(const float* x, const float* h, float* y, int64_t rows, int64_t L, int64_t Lout, int64_t ld_x, int64_t ld_y, int orig,
                      int newf, int width, fqss_stream_t) {
    if (rows == 0 || Lout == 0) return FQSS_OK;
    REQUIRE(x && h && y, "null pointer");
    REQUIRE(rows > 0 && L > 0 && Lout > 0 && ld_x >= L && ld_y >= Lout && orig > 0 && newf > 0 && width >= 0, "bad shape");
    REQUIRE(Lout <= ((int64_t)newf * L + orig - 1) / orig, "output longer than ceil(new * L / orig)");
    const int K = 2 * width + orig;
#pragma omp parallel for collapse(2) schedule(static)
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t o = 0; o < Lout; ++o) {
            const int64_t n = o / newf, base = n * orig - width;
            const int p = (int)(o - n * newf);
            float acc = 0.0f;
            for (int k = 0; k < K; ++k) {
                const int64_t i = base + k;
                acc = fmaf(h[p * K + k], (i >= 0 && i < L) ? x[r * ld_x + i] : 0.0f, acc);
            }
            y[r * ld_y + o] = acc;
        }
    return FQSS_OK;
}

// ------------------------------------------------------------------------------------------------ signal-to-distortion ratio
// include/fqss.h, fqss_sdr: the definition in straight fp64 loops (means subtracted and signals normalised first, direct lag sums,
// Levinson-Durbin); the workspace has the HIP library's size rule and is not used
int64_t fqss_sdr_ws_doubles(int P, int64_t L, int filter_length) {
    if (P < 1 || L < 1 || filter_length < 1 || filter_length > 512) return 0;
    return (int64_t)P * ((L + 1023) / 1024) * (2 * (int64_t)filter_length + 4);
}

int fqss_sdr(const float* est, const float* ref, double* ws, int64_t ws_doubles, double* db, int P, int64_t L, int64_t ld_e, int64_t ld_r,
             int filter_length, int zero_mean, double load_diag, fqss_stream_t) {
    REQUIRE(est && ref && ws && db, "null pointer");
    REQUIRE(P >= 1 && P <= 65535 && L >= 1 && ld_e >= L && ld_r >= L, "bad shape (1 <= P <= 65535, L >= 1, ld >= L)");
    REQUIRE(filter_length >= 1 && filter_length <= 512, "filter_length outside 1..512");
    REQUIRE(ws_doubles >= fqss_sdr_ws_doubles(P, L, filter_length), "workspace shorter than fqss_sdr_ws_doubles");
    const int F = filter_length;
    for (int p = 0; p < P; ++p) {
        std::vector<double> t(L), e(L), r(F, 0.0), b(F, 0.0), a(F, 0.0), an(F, 0.0), x(F, 0.0);
        double st = 0.0, se = 0.0;
        for (int64_t i = 0; i < L; ++i) {
            t[i] = ref[p * ld_r + i];
            e[i] = est[p * ld_e + i];
            st += t[i];
            se += e[i];
        }
        const double mt = zero_mean ? st / (double)L : 0.0, me = zero_mean ? se / (double)L : 0.0;
        double tt = 0.0, ee = 0.0;
        for (int64_t i = 0; i < L; ++i) {
            t[i] -= mt;
            e[i] -= me;
            tt += t[i] * t[i];
            ee += e[i] * e[i];
        }
        const double nt = fmax(sqrt(tt), 1e-6), ne = fmax(sqrt(ee), 1e-6);
        for (int64_t i = 0; i < L; ++i) {
            t[i] /= nt;
            e[i] /= ne;
        }
#pragma omp parallel for schedule(static)
        for (int k = 0; k < F; ++k) {
            double rk = 0.0, bk = 0.0;
            for (int64_t i = 0; i + k < L; ++i) {
                rk += t[i] * t[i + k];
                bk += t[i] * e[i + k];
            }
            r[k] = rk;
            b[k] = bk;
        }
        if (load_diag >= 0.0) r[0] += load_diag;      // (a negative or NaN load_diag: none)
        double E = r[0];
        bool ok = E > 0.0;
        a[0] = 1.0;
        x[0] = b[0] / E;
        for (int m = 1; m < F; ++m) {
            double acc = 0.0, q = 0.0;
            for (int i = 0; i < m; ++i) {
                acc += a[i] * r[m - i];
                q += x[i] * r[m - i];
            }
            const double k = -acc / E;
            E = E * (1.0 - k * k);
            ok = ok && E > 0.0;
            const double lam = (b[m] - q) / E;
            for (int i = 0; i <= m; ++i) an[i] = a[i] + k * a[m - i];
            a.swap(an);
            for (int i = 0; i <= m; ++i) x[i] += lam * a[m - i];
        }
        double coh = 0.0;
        for (int i = 0; i < F; ++i) coh += b[i] * x[i];
        db[p] = (ok && std::isfinite(coh)) ? 10.0 * log10(coh / (1.0 - coh)) : (double)NAN;
    }
    return FQSS_OK;
}

// ------------------------------------------------------------------------------------------------ short-time objective intelligibility
// include/fqss.h, fqss_stoi: the six steps in straight fp64 loops (a direct DFT over the 256 non-zero samples of a frame); the workspace
// has the HIP library's size rule and is not used
static int64_t stoi_gcd(int64_t a, int64_t b) { return b == 0 ? a : stoi_gcd(b, a % b); }
static bool stoi_ratio_ok(int up, int down) { return up >= 1 && down >= 1 && up <= 65536 && down <= 65536 && stoi_gcd(up, down) == 1; }
static bool stoi_shape_ok(int P, int64_t L, int up, int down) {
    return P >= 1 && P <= 32767 && L >= 1 && stoi_ratio_ok(up, down) && L <= ((int64_t)1 << 37) / up;
}
static const int kStoiLo[16] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

int64_t fqss_stoi_ws_doubles(int P, int64_t L, int up, int down) {
    if (!stoi_shape_ok(P, L, up, down)) return 0;
    const int64_t Lp = (L * up + down - 1) / down, NF = Lp > 256 ? (Lp - 256 + 127) / 128 : 0;
    const int64_t Tmax = NF > 1 ? NF - 1 : 0, Smax = NF > 30 ? NF - 30 : 0;
    return (int64_t)P * ((up == down ? 0 : 2 * Lp) + NF + (NF + 2) / 2 + 2 * 15 * Tmax + Smax);
}

int fqss_stoi(const float* est, const float* ref, const double* taps, int n_taps, double* ws, int64_t ws_doubles, double* d, int P,
              int64_t L, int64_t ld_e, int64_t ld_r, int up, int down, fqss_stream_t) {
    REQUIRE(est && ref && taps && ws && d, "null pointer");
    REQUIRE(stoi_ratio_ok(up, down), "up / down not in 1..65536 or not reduced");
    REQUIRE(stoi_shape_ok(P, L, up, down) && ld_e >= L && ld_r >= L, "bad shape (1 <= P <= 32767, 1 <= L <= 2^37 / up, ld >= L)");
    REQUIRE(n_taps >= 1 && (n_taps & 1) && (up != down || n_taps == 1), "n_taps even, or not 1 at up = down = 1");
    REQUIRE(n_taps <= 1023 && 255 * (int64_t)down + n_taps <= 1022 * (int64_t)up, "resampler outside what one workgroup stages");
    REQUIRE(ws_doubles >= fqss_stoi_ws_doubles(P, L, up, down), "workspace shorter than fqss_stoi_ws_doubles");
    const double EPS = 2.220446049250313e-16, PI = 3.14159265358979323846, CLIP = 1.0 + pow(10.0, 15.0 / 20.0);
    const int64_t Lp = (L * up + down - 1) / down, NF = Lp > 256 ? (Lp - 256 + 127) / 128 : 0, Lh = (n_taps - 1) / 2;
    std::vector<double> w(256), cs(512), sn(512);
    for (int t = 0; t < 256; ++t) w[t] = 0.5 - 0.5 * cos(2.0 * PI * (double)(t + 1) / 257.0);
    for (int j = 0; j < 512; ++j) {
        cs[j] = cos(2.0 * PI * (double)j / 512.0);
        sn[j] = sin(2.0 * PI * (double)j / 512.0);
    }
    for (int p = 0; p < P; ++p) {
        std::vector<double> sig[2];      // 0: clean, 1: estimate, at 10 kHz
        for (int s = 0; s < 2; ++s) {
            const float* src = s == 0 ? ref + p * ld_r : est + p * ld_e;
            sig[s].assign((size_t)Lp, 0.0);
            if (up == down) {
                for (int64_t i = 0; i < L; ++i) sig[s][i] = (double)src[i];
                continue;
            }
#pragma omp parallel for schedule(static)
            for (int64_t n = 0; n < Lp; ++n) {
                const int64_t m = n * down + Lh;
                double acc = 0.0;
                for (int64_t k = m % up; k < n_taps; k += up) {      // u[m - k] is a sample only where up divides m - k
                    const int64_t i = (m - k) / up;
                    if (k <= m && i < L) acc += taps[k] * (double)src[i];
                }
                sig[s][n] = acc;
            }
        }
        std::vector<double> e((size_t)NF);
        std::vector<int64_t> kept;
        double emax = -INFINITY;
        for (int64_t f = 0; f < NF; ++f) {
            double ss = 0.0;
            for (int t = 0; t < 256; ++t) {
                const double v = w[t] * sig[0][f * 128 + t];
                ss += v * v;
            }
            e[f] = 20.0 * log10(sqrt(ss) + EPS);
            emax = fmax(emax, e[f]);
        }
        for (int64_t f = 0; f < NF; ++f)
            if (emax - 40.0 - e[f] < 0.0) kept.push_back(f);
        const int64_t K = (int64_t)kept.size(), T = K > 0 ? K - 1 : 0;
        if (T < 30) {
            d[p] = 1e-5;
            continue;
        }
        std::vector<double> tob[2];
        for (int s = 0; s < 2; ++s) {
            std::vector<double> sil((size_t)((K - 1) * 128 + 256), 0.0);
            for (int64_t j = 0; j < K; ++j)
                for (int t = 0; t < 256; ++t) sil[j * 128 + t] += w[t] * sig[s][kept[j] * 128 + t];
            tob[s].assign((size_t)(15 * T), 0.0);
#pragma omp parallel for schedule(static)
            for (int64_t m = 0; m < T; ++m) {
                double fr[256], pw[257];
                for (int t = 0; t < 256; ++t) fr[t] = w[t] * sil[m * 128 + t];
                for (int b = kStoiLo[0]; b < kStoiLo[15]; ++b) {
                    double re = 0.0, im = 0.0;
                    for (int t = 0; t < 256; ++t) {
                        re += fr[t] * cs[(b * t) & 511];
                        im -= fr[t] * sn[(b * t) & 511];
                    }
                    pw[b] = re * re + im * im;
                }
                for (int k = 0; k < 15; ++k) {
                    double acc = 0.0;
                    for (int b = kStoiLo[k]; b < kStoiLo[k + 1]; ++b) acc += pw[b];
                    tob[s][k * T + m] = sqrt(acc);
                }
            }
        }
        double total = 0.0;
        for (int64_t m = 30; m <= T; ++m)
            for (int k = 0; k < 15; ++k) {
                const double *x = &tob[0][k * T + m - 30], *y = &tob[1][k * T + m - 30];
                double xx = 0.0, yy = 0.0, yp[30], xc[30], mx = 0.0, my = 0.0, nx = 0.0, ny = 0.0, dot = 0.0;
                for (int c = 0; c < 30; ++c) {
                    xx += x[c] * x[c];
                    yy += y[c] * y[c];
                }
                const double scale = sqrt(xx) / (sqrt(yy) + EPS);
                for (int c = 0; c < 30; ++c) {
                    yp[c] = fmin(y[c] * scale, x[c] * CLIP);
                    mx += x[c];
                    my += yp[c];
                }
                mx /= 30.0;
                my /= 30.0;
                for (int c = 0; c < 30; ++c) {
                    xc[c] = x[c] - mx;
                    yp[c] -= my;
                    nx += xc[c] * xc[c];
                    ny += yp[c] * yp[c];
                }
                nx = sqrt(nx) + EPS;
                ny = sqrt(ny) + EPS;
                for (int c = 0; c < 30; ++c) dot += (xc[c] / nx) * (yp[c] / ny);
                total += dot;
            }
        d[p] = total / (15.0 * (double)(T - 29));
    }
    return FQSS_OK;
}

// ------------------------------------------------------------------------------------------------ batched chunked inference
// include/fqss.h: chunk k covers [k * stride, k * stride + seg), N = ceil(L / stride) chunks, n_k = min(seg, L - k * stride)
static inline bool chunk_geometry_ok(int64_t L, int64_t seg, int64_t stride) { return L > 0 && seg > 0 && stride > 0 && stride <= seg; }
static inline int64_t chunk_count(int64_t L, int64_t stride) { return (L + stride - 1) / stride; }
static inline float tri_weight(int64_t t, int64_t seg) {      // process.py:166-168
    const int64_t h = seg / 2;
    const float mx = (float)(seg - h);
    return (t < h ? (float)(t + 1) : (float)(seg - t)) / mx;
}

int fqss_chunk_gather(const float* mix, float* out, int64_t L, int64_t seg, int64_t stride, int64_t k0, int G, fqss_stream_t) {
    REQUIRE(mix && out, "null pointer");
    REQUIRE(chunk_geometry_ok(L, seg, stride) && G > 0 && G <= 65535 && k0 >= 0 && k0 < chunk_count(L, stride),
            "bad shape (1 <= stride <= seg, 0 <= k0 < ceil(L / stride), 1 <= G <= 65535)");
    const int64_t N = chunk_count(L, stride);
    for (int64_t g = 0; g < G; ++g) {
        const int64_t k = k0 + g < N ? k0 + g : N - 1, n = L - k * stride;
        for (int64_t t = 0; t < seg; ++t) out[g * seg + t] = t < n ? mix[k * stride + t] : 0.0f;
    }
    return FQSS_OK;
}

int fqss_sisnr_chunks(const float* est, const float* ref, float* db, int* map, int G, int S, int64_t seg, int64_t stride, int64_t k0, int64_t L,
                      int64_t ld_r, fqss_stream_t) {
    REQUIRE(est && ref && db && map, "null pointer");
    REQUIRE(S > 0 && S <= 16 && ld_r >= L, "bad shape (S <= 16, ld_r >= L)");
    REQUIRE(chunk_geometry_ok(L, seg, stride) && G > 0 && k0 >= 0 && k0 < chunk_count(L, stride),
            "bad shape (1 <= stride <= seg, 0 <= k0 < ceil(L / stride), G >= 1)");
    const int64_t N = chunk_count(L, stride);
    const double eps = 1.1920928955078125e-07;      // torch.finfo(torch.float32).eps
    for (int64_t g = 0; g < G; ++g) {
        const int64_t k = k0 + g < N ? k0 + g : N - 1, start = k * stride, n = L - start < seg ? L - start : seg;
        float* dbg = db + g * S * S;
        for (int p = 0; p < S; ++p)
            for (int q = 0; q < S; ++q) {
                const float *e = est + (g * S + p) * seg, *r = ref + q * ld_r + start;
                double m[5] = {0, 0, 0, 0, 0};
                for (int64_t i = 0; i < n; ++i) {
                    const double a = e[i], b = r[i];
                    m[0] += a; m[1] += b; m[2] += a * b; m[3] += a * a; m[4] += b * b;
                }
                const double nn = (double)n;
                const double spt = m[2] - m[0] * m[1] / nn, spp = m[3] - m[0] * m[0] / nn, stt = m[4] - m[1] * m[1] / nn;
                const double alpha = (spt + eps) / (stt + eps);
                const double num = alpha * alpha * stt, den = alpha * alpha * stt - 2.0 * alpha * spt + spp;
                dbg[p * S + q] = (float)(10.0 * log10((num + eps) / ((den < 0.0 ? 0.0 : den) + eps)));
            }
        int* mp = map + g * S * 2;      // swap_channel_order (process.py:105-125): first maximum, later estimates override earlier claims
        for (int d = 0; d < S; ++d) { mp[2 * d] = d; mp[2 * d + 1] = 1; }
        for (int p = 0; p < S; ++p) {
            int best = 0;
            float bv = -INFINITY;
            for (int q = 0; q < S; ++q)
                if (dbg[p * S + q] > bv) { bv = dbg[p * S + q]; best = q; }
            mp[2 * best] = p;
            mp[2 * best + 1] = p == best ? 1 : -1;
        }
    }
    return FQSS_OK;
}

int fqss_infer_ola_chunks(const float* chunks, const int* map, float* out, int S, int C, int64_t L, int64_t seg, int64_t stride,
                          int64_t ld_chunk, int64_t ld_out, fqss_stream_t) {
    REQUIRE(chunks && out, "null pointer");
    REQUIRE(S > 0 && C > 0 && S * C <= 65535 && chunk_geometry_ok(L, seg, stride) && ld_chunk >= seg && ld_out >= L,
            "bad shape (1 <= stride <= seg, ld_chunk >= seg, ld_out >= L)");
    const int64_t N = chunk_count(L, stride);
#pragma omp parallel for collapse(2) schedule(static)
    for (int64_t d = 0; d < S; ++d)
        for (int64_t c = 0; c < C; ++c)
            for (int64_t t = 0; t < L; ++t) {
                const int64_t k_lo = t < seg ? 0 : (t - seg) / stride + 1;
                const int64_t k_hi = t / stride < N - 1 ? t / stride : N - 1;
                float acc = 0.0f, wsum = 0.0f;
                for (int64_t k = k_lo; k <= k_hi; ++k) {      // increasing k: the order of the chunk-by-chunk overlap-add
                    const int64_t src = map ? map[(k * S + d) * 2] : d, tt = t - k * stride;
                    const float sign = map ? (float)map[(k * S + d) * 2 + 1] : 1.0f, w = tri_weight(tt, seg);
                    acc = acc + w * (sign * chunks[((k * S + src) * C + c) * ld_chunk + tt]);
                    wsum += w;
                }
                out[(d * C + c) * ld_out + t] = acc / wsum;
            }
    return FQSS_OK;
}

// include/fqss.h, fqss_aq_hist / fqss_aq_mse_search: the histogram-MSE activation observer in straight fp64 loops.  The workspace has the
// layout of the HIP library's (csrc/aq_mse.hip AqLayout), so that kernels.aq_mse_search reads b, vals and e(i, j) from either.
namespace {
constexpr int kAqBins = FQSS_AQ_HIST_BINS, kAqRows = FQSS_AQ_MSE_MAX_ROWS, kAqMaxM = FQSS_AQ_MSE_MAX_BINS, kAqN = FQSS_AQ_MSE_N;
struct AqLayout {
    int64_t hdr, rows, cum, b, vals, err, total;
};
inline AqLayout aq_layout(int T) {
    AqLayout w;
    w.hdr = 0;
    w.rows = 16;
    w.cum = w.rows + 2 * kAqRows;
    w.b = w.cum + (int64_t)T * (kAqBins + 1);
    w.vals = w.b + kAqMaxM;
    w.err = w.vals + kAqMaxM;
    w.total = w.err + kAqN * kAqN;
    return w;
}
inline bool aq_finite(float v) { return std::isfinite(v); }
inline int aq_guess(double v, double lo, double span) {
    const double f = (v - lo) / span * (double)kAqBins;
    return f >= (double)kAqBins ? kAqBins - 1 : (f > 0.0 ? (int)f : 0);
}
inline int aq_bin(double v, double lo, double span, double step) {
    int k = aq_guess(v, lo, span);
    if (v < lo + (double)k * step) {
        k = k > 0 ? k - 1 : 0;
    } else if (k < kAqBins - 1 && v >= lo + (double)(k + 1) * step) {
        k += 1;
    }
    return k;
}
inline double aq_cum_at(double b, double lo, double hi, const double* c) {
    if (b < lo) return 0.0;
    if (b >= hi) return c[kAqBins];
    const double span = hi - lo, step = span / (double)kAqBins;
    int k = aq_guess(b, lo, span);
    for (int r = 0; r < 4 && k > 0 && b < lo + (double)k * step; ++r) k -= 1;
    for (int r = 0; r < 4 && k < kAqBins - 1 && b >= lo + (double)(k + 1) * step; ++r) k += 1;
    const double e0 = lo + (double)k * step, e1 = k == kAqBins - 1 ? hi : lo + (double)(k + 1) * step;
    const double slope = (c[k + 1] - c[k]) / (e1 - e0);
    return slope * (b - e0) + c[k];
}
}  // namespace

int64_t fqss_aq_mse_ws_bytes(int T) {
    if (T < 1 || T > kAqRows) return 0;
    return aq_layout(T).total * (int64_t)sizeof(double);
}

int64_t fqss_aq_mse_ws_offset(int T, int what) {
    if (T < 1 || T > kAqRows) return -1;
    const AqLayout L = aq_layout(T);
    switch (what) {
        case FQSS_AQ_WS_HDR: return L.hdr;
        case FQSS_AQ_WS_ROWS: return L.rows;
        case FQSS_AQ_WS_CUM: return L.cum;
        case FQSS_AQ_WS_B: return L.b;
        case FQSS_AQ_WS_VALS: return L.vals;
        case FQSS_AQ_WS_ERR: return L.err;
    }
    return -1;
}

int fqss_aq_hist_rows(const float* x, int64_t rows, int64_t cols, int64_t ld, uint32_t* obs_ws, uint32_t* hist_row, float* rng_row,
                      fqss_stream_t) {
    REQUIRE(x && obs_ws && hist_row && rng_row, "null pointer");
    REQUIRE(rows >= 1 && cols >= 1 && ld >= cols && rows < ((int64_t)1 << 32) && cols < ((int64_t)1 << 32) && rows * cols < ((int64_t)1 << 32),
            "bad shape (rows, cols >= 1, ld >= cols, rows * cols < 2^32)");
    const float lo32 = ord2f(obs_ws[0]), hi32 = ord2f(obs_ws[1]);
    obs_ws[0] = 0xFFFFFFFFu;
    obs_ws[1] = 0u;
    if (!aq_finite(lo32) || !aq_finite(hi32)) {
        rng_row[0] = rng_row[1] = NAN;
        return FQSS_OK;
    }
    rng_row[0] = lo32;
    rng_row[1] = hi32;
    double lo = (double)lo32, hi = (double)hi32;
    if (lo == hi) {
        lo -= 0.5;
        hi += 0.5;
    }
    const double span = hi - lo, step = span / (double)kAqBins;
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t i = 0; i < cols; ++i) hist_row[aq_bin((double)x[r * ld + i], lo, span, step)] += 1u;
    return FQSS_OK;
}

int fqss_aq_hist(const float* x, int64_t n, uint32_t* obs_ws, uint32_t* hist_row, float* rng_row, fqss_stream_t stream) {
    REQUIRE(x && obs_ws && hist_row && rng_row, "null pointer");
    REQUIRE(n >= 1 && n < ((int64_t)1 << 32), "n outside 1 .. 2^32 - 1");
    return fqss_aq_hist_rows(x, 1, n, n, obs_ws, hist_row, rng_row, stream);
}

int fqss_aq_mse_search(const uint32_t* hist, const float* rng, int T, int n_bits, double* ws, float* qmin, float* qmax, int* ij_out,
                       double* err_out, fqss_stream_t) {
    REQUIRE(hist && rng && ws && qmin && qmax, "null pointer");
    REQUIRE(T >= 1 && T <= kAqRows, "T outside 1 .. 64");
    REQUIRE(n_bits == 8, "n_bits must be 8 (the activation grid of the fused kernels)");
    const AqLayout L = aq_layout(T);
    double bmin = INFINITY, bmax = -INFINITY, w = INFINITY;
    int nv = 0;
    for (int t = 0; t < kAqRows; ++t) ws[L.rows + 2 * t] = ws[L.rows + 2 * t + 1] = NAN;
    for (int t = 0; t < T; ++t) {
        double* c = ws + L.cum + (int64_t)t * (kAqBins + 1);
        uint64_t s = 0;
        c[0] = 0.0;
        for (int k = 0; k < kAqBins; ++k) {
            s += hist[(int64_t)t * kAqBins + k];
            c[k + 1] = (double)s;
        }
        if (!aq_finite(rng[2 * t]) || !aq_finite(rng[2 * t + 1])) continue;
        double lo = (double)rng[2 * t], hi = (double)rng[2 * t + 1];
        if (lo == hi) {
            lo -= 0.5;
            hi += 0.5;
        }
        ws[L.rows + 2 * t] = lo;
        ws[L.rows + 2 * t + 1] = hi;
        nv += 1;
        bmin = std::fmin(bmin, lo);
        bmax = std::fmax(bmax, hi);
        w = std::fmin(w, (hi - lo) / (double)kAqBins);
    }
    double Md = std::ceil(((bmax + w) - bmin) / w);
    if (!(Md <= (double)kAqMaxM)) {
        w = (bmax - bmin) / (double)(kAqMaxM - 1);
        Md = std::fmin(std::ceil(((bmax + w) - bmin) / w), (double)kAqMaxM);
    }
    if (!(Md >= 2.0) || nv == 0) Md = 2.0;
    const int M = (int)Md, K = M - 1;
    ws[L.hdr + 0] = bmin;
    ws[L.hdr + 1] = bmax;
    ws[L.hdr + 2] = w;
    ws[L.hdr + 3] = Md;
    ws[L.hdr + 4] = (double)nv;
    double* b = ws + L.b;
    double* vals = ws + L.vals;
    double* err = ws + L.err;
#pragma omp parallel for
    for (int m = 0; m < M; ++m) {
        const double b0 = bmin + (double)m * w;
        b[m] = b0;
        if (m >= M - 1) continue;
        const double b1 = bmin + (double)(m + 1) * w;
        double acc = 0.0;
        for (int t = 0; t < T; ++t) {
            const double lo = ws[L.rows + 2 * t], hi = ws[L.rows + 2 * t + 1];
            if (lo != lo) continue;
            const double* c = ws + L.cum + (int64_t)t * (kAqBins + 1);
            acc += aq_cum_at(b1, lo, hi, c) - aq_cum_at(b0, lo, hi, c);
        }
        vals[m] = acc;
    }
    if (nv == 0) {
        if (ij_out) ij_out[0] = ij_out[1] = -1;
        if (err_out) *err_out = NAN;
        return FQSS_OK;
    }
    double sum = 0.0;
    for (int m = 0; m < K; ++m) sum += vals[m];
    const double b0 = b[0], bl = b[K - 1];
    const double delta = 0.5 * (bl - b0) / (double)kAqN;
#pragma omp parallel for
    for (int ij = 0; ij < kAqN * kAqN; ++ij) {
        const int i = ij / kAqN, j = ij % kAqN;
        const double mn = b0 + delta * (double)i, mx = bl - delta * (double)j;
        const double D = (mx - mn) / 255.0;
        double acc = 0.0;
        for (int m = 0; m < K; ++m) {
            const double c = std::fmin(std::fmax(std::nearbyint((b[m] - mn) / D), 0.0), 255.0);
            const double d = b[m] - (D * c + mn);
            acc += (d * d) * vals[m];
        }
        err[ij] = acc / sum;
    }
    double best = INFINITY;
    int idx = 0;
    for (int ij = 0; ij < kAqN * kAqN; ++ij)
        if (err[ij] < best) {
            best = err[ij];
            idx = ij;
        }
    *qmin = (float)(b0 + delta * (double)(idx / kAqN));
    *qmax = (float)(bl - delta * (double)(idx % kAqN));
    if (ij_out) {
        ij_out[0] = idx / kAqN;
        ij_out[1] = idx % kAqN;
    }
    if (err_out) *err_out = best;
    return FQSS_OK;
}

}  // extern "C"
