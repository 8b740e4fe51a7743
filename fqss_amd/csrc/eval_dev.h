// eval_dev.h -- per-sample device functions that more than one kernel of the evaluation side computes through, so that the kernels that
// must agree bit for bit carry ONE operation sequence (contraction is off: every operator is one IEEE operation):
//   the weighted overlap-add of infer.hip (k_infer_ola, k_infer_ola_chunks),
//   the normalize=False splitter of codec.hip (k_splitter2_raw) and of track_eval.hip (k_splitter2_raw_rows),
//   the Levinson-Durbin recursion of sdr.hip (k_sdr_finish) and of bss_eval.hip (k_bss_tgt).
#pragma once
#include "fqss_dev.h"

namespace fqss {
#if defined(__HIPCC__)

// triangular chunk weight of model_infer (process.py:166-168): 1..h, (seg-h)..1 over max, h = seg / 2
__device__ __forceinline__ float tri_weight(int64_t t, int64_t seg) {
    const int64_t h = seg / 2;
    const float mx = (float)(seg - h);
    return (t < h ? (float)(t + 1) : (float)(seg - t)) / mx;
}

// one step of the weighted overlap-add, acc + w * (sign * v): k_infer_ola and the gather forms accumulate through this one expression,
// so they round alike (two multiplications and one addition, no fused multiply-add: the library is built with -ffp-contract=off)
__device__ __forceinline__ float ola_step(float acc, float w, float sign, float v) { return acc + w * (sign * v); }

// output sample t of source d, channel c of the overlap-add as a gather: the chunks that cover t in increasing k -- the order in which
// fqss_infer_ola is called chunk after chunk -- through ola_step / tri_weight, divided by the weight sum.  chunks [N][S][C][ld_chunk]
__device__ __forceinline__ float ola_chunks_sample(const float* __restrict__ chunks, const int* __restrict__ map, int S, int C, int d, int c,
                                                   int64_t t, int64_t seg, int64_t stride, int64_t N, int64_t ld_chunk) {
    const int64_t k_lo = t < seg ? 0 : (t - seg) / stride + 1;      // first k with t - k * stride < seg
    int64_t k_hi = t / stride;                                       // last k with k * stride <= t
    if (k_hi > N - 1) k_hi = N - 1;
    float acc = 0.0f, wsum = 0.0f;
    for (int64_t k = k_lo; k <= k_hi; ++k) {
        const int* mp = map != nullptr ? map + (k * S + d) * 2 : nullptr;
        const int src = mp != nullptr ? mp[0] : d;
        const float sign = mp != nullptr ? (float)mp[1] : 1.0f;
        const int64_t tt = t - k * stride;
        const float w = tri_weight(tt, seg);
        acc = ola_step(acc, w, sign, chunks[((k * S + src) * C + c) * ld_chunk + tt]);
        wsum += w;
    }
    return acc / wsum;
}

// p[i .. i + 3] clipped to [0, n): one 16-byte request when VEC (the caller vouches for the alignment) and the quad is whole; 0 past n.
// The tile sums of track_eval.hip and of hd_loss.hip (fqss_hd_loss_x) read through it: both load forms give the same samples
template <bool VEC>
__device__ __forceinline__ void load_quad(const float* __restrict__ p, int64_t i, int64_t n, float (&v)[4]) {
    if (VEC && i + 4 <= n) {
        const float4 q = *reinterpret_cast<const float4*>(p + i);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = i + e < n ? p[i + e] : 0.0f;
    }
}

// torch.clip(v, -128, 127) of process.py:14: a NaN stays NaN (fminf / fmaxf would return the bound, and the 0 / 0 of a silent row
// would come out as -1 where the reference -- and include/fqss.h -- say NaN)
__device__ __forceinline__ float split_clip(float v) {
    v = v < -128.0f ? -128.0f : v;
    return v > 127.0f ? 127.0f : v;
}

// the two channels of one sample of preprocess(x, n_splitter=2, normalize=False) (process.py:26-36) under threshold thr,
// delta = thr / 128: x is NOT divided by thr
__device__ __forceinline__ void split2_raw(float v, float thr, float delta, float& msb, float& lsb) {
    const float q0 = split_clip(floorf(v / delta)) * delta;
    const float r = ((2.0f * (v - q0)) * thr) / delta - thr;      // process.py:35 op order
    msb = q0;
    lsb = split_clip(floorf(r / delta)) * delta;
}

// Levinson-Durbin on normalised lag sums r_s, b_s [F] in LDS (csrc/sdr.hip k_sdr_finish; csrc/bss_eval.hip k_bss_tgt): coh = b . R^-1 b
// with R the symmetric Toeplitz matrix of r, valid in thread 0; ok: every prediction error was positive.  A 256-thread workgroup, all of
// it in the call; a_s [2][kLevMaxF] holds (1, 0, ...) and zeros on entry and the caller has synchronised; red: 8 doubles.
// a^(n) is the prediction polynomial of order n (a[0] = 1) with error E_n = E_(n-1) (1 - k^2); its reverse y solves R_(n+1) y = E_n e_n,
// so the solution grows by x += (b[n] - sum_i x[i] r[n - i]) / E_n * y.  Thread j holds elements j and j + 256 of a and x in registers; a
// is mirrored in LDS (two buffers, written for step n + 1 while step n's is read) for the reversed reads.  Per step: two dot products
// (DPP tree inside a wave, the four wave sums through LDS, added in wave order), two updates, two barriers.
constexpr int kLevMaxF = 512;
__device__ __forceinline__ double levinson_coh(const double* r_s, const double* b_s, double (*a_s)[kLevMaxF], double* red, int F, bool& ok) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double E = r_s[0];
    ok = E > 0.0;
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
    return ((red[0] + red[1]) + red[2]) + red[3];
}

#endif  // __HIPCC__
}  // namespace fqss
