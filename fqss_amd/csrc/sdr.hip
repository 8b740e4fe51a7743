// sdr.hip -- signal-to-distortion ratio of the evaluation side (process.metric_evaluation, process.py:129-152 of the reference:
// torchmetrics' SignalDistortionRatio, which computes it with fast_bss_eval -- both third party, restated from the published definition).
// For one (estimate, target) pair of L samples and a distortion filter of F taps:
//   target /= max(||target||, 1e-6), preds /= max(||preds||, 1e-6)      (after subtracting the means when zero_mean)
//   r[k] = sum_t target[t] target[t + k],  b[k] = sum_t target[t] preds[t + k],  k < F, linear: terms with t + k >= L are absent
//   R sol = b with R the symmetric Toeplitz matrix of r (r[0] += load_diag first),  coh = b . sol,  SDR = 10 log10(coh / (1 - coh))
// Two kernels, all sums in fp64 (products of two fp32 values are exact there), no floating-point atomics -- the same bits every run:
//   k_sdr_corr    grid (time tiles, pairs): the tile's share of r, b and of the four moments, stored to ws[pair][tile][2F + 4]
//   k_sdr_finish  one workgroup per pair: tile partials summed in tile order, normalisation, Levinson-Durbin, the ratio in dB
#include "fqss_dev.h"

namespace fqss {

constexpr int kSdrTile = 1024;      // time samples per workgroup of k_sdr_corr (tests/test_gpu_sdr.py names it: TILE)
constexpr int kSdrMaxF = 512;       // filter_length <= 512: two adjacent lags per thread of a 256-thread workgroup
constexpr int kSdrMom = 4;          // sum t^2, sum p^2, sum t, sum p behind the 2F lag sums of a tile

__host__ __device__ static inline int64_t sdr_stride(int F) { return 2 * (int64_t)F + kSdrMom; }

// Thread j owns lags 2j and 2j + 1.  The tile of `ref` and its F - 1 samples of halo (and the same span of `est`) sit in LDS as fp64, zero
// past the end of the signal, so an absent term is an exact 0.  Per pair of time samples a wave reads the two samples (one address for
// all lanes: a broadcast) and, per array, the next two doubles of its sliding window (16 B per lane, consecutive across lanes: every
// bank once) for eight fp64 FMAs per lane.
__global__ __launch_bounds__(256) void k_sdr_corr(const float* __restrict__ est, const float* __restrict__ ref, double* __restrict__ ws, int F,
                                                  int64_t L, int64_t ld_e, int64_t ld_r) {
    __shared__ __attribute__((aligned(16))) double refh[kSdrTile + kSdrMaxF];
    __shared__ __attribute__((aligned(16))) double esth[kSdrTile + kSdrMaxF];
    __shared__ double smem[kSdrMom * 4];
    const int tid = threadIdx.x;
    const int64_t p = blockIdx.y, t0 = (int64_t)blockIdx.x * kSdrTile;
    const float *e = est + p * ld_e, *r = ref + p * ld_r;
    for (int i = tid; i < kSdrTile + kSdrMaxF; i += 256) {
        const int64_t g = t0 + i;
        refh[i] = g < L ? (double)r[g] : 0.0;
        esth[i] = g < L ? (double)e[g] : 0.0;
    }
    __syncthreads();
    double* out = ws + (p * gridDim.x + blockIdx.x) * sdr_stride(F);
    const int k0 = 2 * tid;
    if (k0 < F) {
        const double2* a2 = reinterpret_cast<const double2*>(refh);
        const double2* x2 = reinterpret_cast<const double2*>(refh + k0);
        const double2* y2 = reinterpret_cast<const double2*>(esth + k0);
        double r0 = 0.0, r1 = 0.0, b0 = 0.0, b1 = 0.0;
        double2 x = x2[0], y = y2[0];
#pragma unroll 4
        for (int t = 0; t < kSdrTile / 2; ++t) {
            const double2 a = a2[t], xn = x2[t + 1], yn = y2[t + 1];
            r0 = fma(a.x, x.x, r0);
            r1 = fma(a.x, x.y, r1);
            b0 = fma(a.x, y.x, b0);
            b1 = fma(a.x, y.y, b1);
            r0 = fma(a.y, x.y, r0);
            r1 = fma(a.y, xn.x, r1);
            b0 = fma(a.y, y.y, b0);
            b1 = fma(a.y, yn.x, b1);
            x = xn;
            y = yn;
        }
        out[k0] = r0;
        out[F + k0] = b0;
        if (k0 + 1 < F) {
            out[k0 + 1] = r1;
            out[F + k0 + 1] = b1;
        }
    }
    double m[kSdrMom] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < kSdrTile; i += 256) {
        const double a = refh[i], c = esth[i];
        m[0] = fma(a, a, m[0]);
        m[1] = fma(c, c, m[1]);
        m[2] += a;
        m[3] += c;
    }
    block_sum<double, kSdrMom>(m, smem);
    if (tid == 0)
        for (int i = 0; i < kSdrMom; ++i) out[2 * F + i] = m[i];
}

// sum of x[i0 .. i0 + n) in index order
__device__ __forceinline__ double sdr_span_sum(const float* __restrict__ x, int64_t i0, int64_t n) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += (double)x[i0 + i];
    return s;
}

// Levinson-Durbin on the normalised lag sums.  a^(n) is the prediction polynomial of order n (a[0] = 1) with error E_n = E_(n-1) (1 - k^2);
// its reverse y solves R_(n+1) y = E_n e_n, so the solution grows by x += (b[n] - sum_i x[i] r[n - i]) / E_n * y.  Thread j holds elements j and
// j + 256 of a and x in registers; a is mirrored in LDS (two buffers, written for step n + 1 while step n's is read) for the reversed reads.
// Per step: two dot products (DPP tree inside a wave, the four wave sums through LDS, added in wave order), two updates, two barriers.
__global__ __launch_bounds__(256) void k_sdr_finish(const float* __restrict__ est, const float* __restrict__ ref, const double* __restrict__ ws,
                                                    double* __restrict__ db, int F, int64_t L, int64_t ld_e, int64_t ld_r, int64_t ntiles,
                                                    int zero_mean, double load_diag) {
    __shared__ double r_s[kSdrMaxF], b_s[kSdrMaxF], a_s[2][kSdrMaxF], red[8], mom[kSdrMom];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t p = blockIdx.x, stride = sdr_stride(F);
    const double* part = ws + p * ntiles * stride;
    const float *e = est + p * ld_e, *r = ref + p * ld_r;
    double rr[2] = {0.0, 0.0}, bb[2] = {0.0, 0.0};
    for (int64_t tile = 0; tile < ntiles; ++tile)
        for (int s = 0; s < 2; ++s) {
            const int k = tid + 256 * s;
            if (k < F) {
                rr[s] += part[tile * stride + k];
                bb[s] += part[tile * stride + F + k];
            }
        }
    if (tid < kSdrMom) {
        double s = 0.0;
        for (int64_t tile = 0; tile < ntiles; ++tile) s += part[tile * stride + 2 * F + tid];
        mom[tid] = s;
    }
    a_s[0][tid] = tid == 0 ? 1.0 : 0.0;
    a_s[0][tid + 256] = 0.0;
    a_s[1][tid] = 0.0;
    a_s[1][tid + 256] = 0.0;
    __syncthreads();
    // normalisation; with zero_mean the lag sums of the centred signals follow from the raw ones, the totals and the sums of the first / last
    // k samples: sum_{t < L - k} (t[t] - mt)(p[t + k] - mp) = b[k] - mp (St - last_k(t)) - mt (Sp - first_k(p)) + (L - k) mt mp
    const double n = (double)L, St = mom[2], Sp = mom[3];
    const double mt = zero_mean ? St / n : 0.0, mp = zero_mean ? Sp / n : 0.0;
    const double tt = mom[0] - mt * St, pp = mom[1] - mp * Sp;
    const double nt = fmax(sqrt(fmax(tt, 0.0)), 1e-6), np = fmax(sqrt(fmax(pp, 0.0)), 1e-6);
    for (int s = 0; s < 2; ++s) {
        const int k = tid + 256 * s;
        if (k >= F) continue;
        double rv = 0.0, bv = 0.0;
        if (k < L) {
            rv = rr[s];
            bv = bb[s];
            if (zero_mean) {
                const double head_t = sdr_span_sum(r, 0, k), tail_t = sdr_span_sum(r, L - k, k), head_p = sdr_span_sum(e, 0, k);
                const double cnt = (double)(L - k);
                rv = rv - mt * ((St - tail_t) + (St - head_t)) + cnt * mt * mt;
                bv = bv - mp * (St - tail_t) - mt * (Sp - head_p) + cnt * mt * mp;
            }
            rv = rv / (nt * nt);
            bv = bv / (nt * np);
        }
        if (k == 0 && load_diag >= 0.0) rv += load_diag;      // (a negative or NaN load_diag: none)
        r_s[k] = rv;
        b_s[k] = bv;
    }
    __syncthreads();
    double E = r_s[0];
    bool ok = E > 0.0;
    double a[2] = {tid == 0 ? 1.0 : 0.0, 0.0}, x[2] = {tid == 0 ? b_s[0] / E : 0.0, 0.0};
    for (int m = 1; m < F; ++m) {
        const double* ac = a_s[(m - 1) & 1];
        double* an = a_s[m & 1];
        double acc = 0.0, q = 0.0;
        for (int s = 0; s < 2; ++s) {
            const int i = tid + 256 * s;
            if (i < m) {
                const double rv = r_s[m - i];
                acc = fma(a[s], rv, acc);
                q = fma(x[s], rv, q);
            }
        }
        acc = wave_sum63(acc);
        q = wave_sum63(q);
        if (lane == 63) {
            red[2 * w] = acc;
            red[2 * w + 1] = q;
        }
        __syncthreads();
        acc = ((red[0] + red[2]) + red[4]) + red[6];
        q = ((red[1] + red[3]) + red[5]) + red[7];
        const double k = -acc / E;
        E = E * (1.0 - k * k);
        ok = ok && E > 0.0;
        const double lam = (b_s[m] - q) / E;
        for (int s = 0; s < 2; ++s) {
            const int i = tid + 256 * s;
            if (i <= m) {
                const double arev = ac[m - i];
                const double ai = fma(k, arev, a[s]);         // a^(m)[i]
                x[s] = fma(lam, fma(k, a[s], arev), x[s]);    // + lam a^(m)[m - i]
                a[s] = ai;
                an[i] = ai;
            }
        }
        __syncthreads();
    }
    double coh = 0.0;
    for (int s = 0; s < 2; ++s) {
        const int i = tid + 256 * s;
        if (i < F) coh = fma(b_s[i], x[s], coh);
    }
    coh = wave_sum63(coh);
    if (lane == 63) red[w] = coh;
    __syncthreads();
    if (tid == 0) {
        coh = ((red[0] + red[1]) + red[2]) + red[3];
        db[p] = (ok && isfinite(coh)) ? 10.0 * log10(coh / (1.0 - coh)) : (double)NAN;
    }
}

}  // namespace fqss

using namespace fqss;

// doubles of workspace of fqss_sdr: P pairs x cdiv(L, 1024) time tiles x (2 filter_length + 4); 0 for arguments fqss_sdr refuses
extern "C" int64_t fqss_sdr_ws_doubles(int P, int64_t L, int filter_length) {
    if (P < 1 || L < 1 || filter_length < 1 || filter_length > kSdrMaxF) return 0;
    return (int64_t)P * cdiv(L, kSdrTile) * sdr_stride(filter_length);
}

extern "C" int fqss_sdr(const float* est, const float* ref, double* ws, int64_t ws_doubles, double* db, int P, int64_t L, int64_t ld_e,
                        int64_t ld_r, int filter_length, int zero_mean, double load_diag, fqss_stream_t stream) {
    FQSS_REQUIRE(est && ref && ws && db, "null pointer");
    FQSS_REQUIRE(P >= 1 && P <= 65535 && L >= 1 && ld_e >= L && ld_r >= L, "bad shape (1 <= P <= 65535, L >= 1, ld >= L)");
    FQSS_REQUIRE(filter_length >= 1 && filter_length <= kSdrMaxF, "filter_length outside 1..512");
    const int64_t ntiles = cdiv(L, kSdrTile);
    FQSS_REQUIRE(ntiles <= 0x7fffffff, "L too long");
    FQSS_REQUIRE(ws_doubles >= fqss_sdr_ws_doubles(P, L, filter_length), "workspace shorter than fqss_sdr_ws_doubles");
    hipLaunchKernelGGL(k_sdr_corr, dim3((unsigned)ntiles, (unsigned)P), dim3(256), 0, (hipStream_t)stream, est, ref, ws, filter_length, L, ld_e, ld_r);
    hipLaunchKernelGGL(k_sdr_finish, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, est, ref, (const double*)ws, db, filter_length, L, ld_e,
                       ld_r, ntiles, zero_mean, load_diag);
    return launch_status("fqss_sdr");
}
