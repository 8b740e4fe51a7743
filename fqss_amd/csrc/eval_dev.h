// eval_dev.h -- per-sample device functions that more than one kernel of the evaluation side computes through, so that the kernels that
// must agree bit for bit carry ONE operation sequence (contraction is off: every operator is one IEEE operation):
//   the weighted overlap-add of infer.hip (k_infer_ola, k_infer_ola_chunks),
//   the normalize=False splitter of codec.hip (k_splitter2_raw) and of track_eval.hip (k_splitter2_raw_rows).
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

#endif  // __HIPCC__
}  // namespace fqss
