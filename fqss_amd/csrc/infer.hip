// infer.hip -- the evaluation side of the path: `process.model_infer` chunked inference with triangular
// overlap-add and per-chunk source re-ordering (process.py:105-194) and the SI-SNR the re-ordering and `val.py` are built on
// (torchmetrics' ScaleInvariantSignalNoiseRatio, third party: restated from its published form, zero-mean SI-SDR with eps = 2^-23).
// All of it stays on the device: five fp64 moments per (estimate, target) pair, a one-wave finish that also takes the re-ordering
// decision of `swap_channel_order` (so no host round trip per chunk), and one stream for the weighted overlap-add.
#include "fqss_dev.h"

namespace fqss {

// mom[p][q][5] += (sum e, sum r, sum e r, sum e e, sum r r) of est[p][:], ref[q][:]
__global__ __launch_bounds__(256) void k_sisnr_moments(const float* __restrict__ est, const float* __restrict__ ref, double* __restrict__ mom,
                                                        int S, int64_t L, int64_t ld_e, int64_t ld_r) {
    __shared__ double smem[5 * 4];
    const int p = blockIdx.y / S, q = blockIdx.y % S;
    const float *e = est + p * ld_e, *r = ref + q * ld_r;
    double v[5] = {0, 0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < L; i += (int64_t)gridDim.x * 256) {
        const double a = e[i], b = r[i];
        v[0] += a; v[1] += b; v[2] += a * b; v[3] += a * a; v[4] += b * b;
    }
    block_sum<double, 5>(v, smem);
    if (threadIdx.x == 0)
        for (int k = 0; k < 5; ++k) atomicAdd(mom + ((int64_t)p * S + q) * 5 + k, v[k]);
}

// db[p][q] = SI-SNR(est_p, ref_q) in dB; map[d] = (source index, sign) of swap_channel_order (process.py:105-125):
// for every estimate p in order: d = argmax_q db[p][q] (first maximum), out[d] = est_p if p == d else -est_p; untouched d keep est_d
__global__ void k_sisnr_finish(const double* __restrict__ mom, float* __restrict__ db, int* __restrict__ map, int S, int64_t L, int do_map) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double eps = 1.1920928955078125e-07;      // torch.finfo(torch.float32).eps
    for (int p = 0; p < S; ++p)
        for (int q = 0; q < S; ++q) {
            const double* m = mom + ((int64_t)p * S + q) * 5;
            const double n = (double)L;
            const double spt = m[2] - m[0] * m[1] / n, spp = m[3] - m[0] * m[0] / n, stt = m[4] - m[1] * m[1] / n;
            const double alpha = (spt + eps) / (stt + eps);
            const double num = alpha * alpha * stt, den = alpha * alpha * stt - 2.0 * alpha * spt + spp;
            db[p * S + q] = (float)(10.0 * log10((num + eps) / ((den < 0.0 ? 0.0 : den) + eps)));
        }
    if (!do_map) return;
    for (int d = 0; d < S; ++d) { map[2 * d] = d; map[2 * d + 1] = 1; }
    for (int p = 0; p < S; ++p) {
        int best = 0;
        float bv = -INFINITY;
        for (int q = 0; q < S; ++q)
            if (db[p * S + q] > bv) { bv = db[p * S + q]; best = q; }
        map[2 * best] = p;
        map[2 * best + 1] = p == best ? 1 : -1;
    }
}

// triangular chunk weight of model_infer (process.py:166-168): 1..h, (seg-h)..1 over max, h = seg / 2
__device__ __forceinline__ float tri_weight(int64_t t, int64_t seg) {
    const int64_t h = seg / 2;
    const float mx = (float)(seg - h);
    return (t < h ? (float)(t + 1) : (float)(seg - t)) / mx;
}

// one step of the weighted overlap-add, acc + w * (sign * v): k_infer_ola and k_infer_ola_chunks both accumulate through this one
// expression, so the two round alike (two multiplications and one addition, no fused multiply-add: the library is built with
// -ffp-contract=off)
__device__ __forceinline__ float ola_step(float acc, float w, float sign, float v) { return acc + w * (sign * v); }

// out[d][c][start + t] += w[t] * sign_d * chunk[src_d][c][t];  sum_weight[start + t] += w[t]   (t < n)
__global__ __launch_bounds__(256) void k_infer_ola(const float* __restrict__ chunk, const int* __restrict__ map, float* __restrict__ out,
                                                    float* __restrict__ sum_weight, int S, int C, int64_t n, int64_t seg, int64_t start,
                                                    int64_t ld_chunk, int64_t ld_out) {
    const int dc = blockIdx.y, d = dc / C, c = dc % C;
    const int src = map != nullptr ? map[2 * d] : d;
    const float sign = map != nullptr ? (float)map[2 * d + 1] : 1.0f;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
        const float w = tri_weight(t, seg);
        float* o = out + ((int64_t)d * C + c) * ld_out + start + t;
        *o = ola_step(*o, w, sign, chunk[((int64_t)src * C + c) * ld_chunk + t]);
        if (dc == 0) sum_weight[start + t] += w;
    }
}

__global__ __launch_bounds__(256) void k_infer_normalize(float* __restrict__ out, const float* __restrict__ sum_weight, int64_t rows, int64_t L,
                                                          int64_t ld) {
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y)
        for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < L; t += (int64_t)gridDim.x * 256) out[r * ld + t] /= sum_weight[t];
}

// ---- the batched form of the chunked path: G chunks of one utterance per model call (process.model_infer(chunk_batch=G)) ----
// chunk k covers mix[k * stride : k * stride + seg]; N = ceil(L / stride) chunks; n_k = min(seg, L - k * stride)

// out[g][t] = mix[(k0 + g) * stride + t], zero past L; rows past the last chunk repeat it (one [G, 1, seg] shape serves every group)
__global__ __launch_bounds__(256) void k_chunk_gather(const float* __restrict__ mix, float* __restrict__ out, int64_t L, int64_t seg,
                                                       int64_t stride, int64_t k0, int64_t N) {
    int64_t k = k0 + blockIdx.y;
    if (k > N - 1) k = N - 1;
    const float* src = mix + k * stride;
    const int64_t n = L - k * stride;       // >= 1
    float* dst = out + (int64_t)blockIdx.y * seg;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < seg; t += (int64_t)gridDim.x * 256) dst[t] = t < n ? src[t] : 0.0f;
}

// SI-SNR matrix and re-ordering map of every chunk of a group in one launch: one workgroup per chunk, one wave per (estimate, target)
// pair (round robin), the five fp64 moments summed per lane in index order and over the lanes on the fixed DPP tree -- no atomics, the
// same bits every run.  Formula and first-maximum scan: k_sisnr_finish.
__global__ __launch_bounds__(256) void k_sisnr_chunks(const float* __restrict__ est, const float* __restrict__ ref, float* __restrict__ db,
                                                       int* __restrict__ map, int S, int64_t seg, int64_t stride, int64_t k0, int64_t N,
                                                       int64_t L, int64_t ld_r) {
    __shared__ float sdb[16 * 16];
    const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t k = k0 + g;
    if (k > N - 1) k = N - 1;
    const int64_t start = k * stride, n = L - start < seg ? L - start : seg;
    const double eps = 1.1920928955078125e-07;      // torch.finfo(torch.float32).eps
    for (int pq = wave; pq < S * S; pq += 4) {
        const int p = pq / S, q = pq % S;
        const float *e = est + ((int64_t)g * S + p) * seg, *r = ref + q * ld_r + start;
        double v[5] = {0, 0, 0, 0, 0};
        for (int64_t i = lane; i < n; i += 64) {
            const double a = e[i], b = r[i];
            v[0] += a; v[1] += b; v[2] += a * b; v[3] += a * a; v[4] += b * b;
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) v[j] = wave_sum63(v[j]);
        if (lane == 63) {
            const double nn = (double)n;
            const double spt = v[2] - v[0] * v[1] / nn, spp = v[3] - v[0] * v[0] / nn, stt = v[4] - v[1] * v[1] / nn;
            const double alpha = (spt + eps) / (stt + eps);
            const double num = alpha * alpha * stt, den = alpha * alpha * stt - 2.0 * alpha * spt + spp;
            const float d = (float)(10.0 * log10((num + eps) / ((den < 0.0 ? 0.0 : den) + eps)));
            sdb[pq] = d;
            db[(int64_t)g * S * S + pq] = d;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int* mp = map + (int64_t)g * S * 2;
    for (int d = 0; d < S; ++d) { mp[2 * d] = d; mp[2 * d + 1] = 1; }
    for (int p = 0; p < S; ++p) {
        int best = 0;
        float bv = -INFINITY;
        for (int q = 0; q < S; ++q)
            if (sdb[p * S + q] > bv) { bv = sdb[p * S + q]; best = q; }
        mp[2 * best] = p;
        mp[2 * best + 1] = p == best ? 1 : -1;
    }
}

// the overlap-add as a gather: every output sample walks the chunks that cover it in increasing k -- the order in which fqss_infer_ola
// is called chunk after chunk -- through the same ola_step / tri_weight, then divides by its weight sum: bit for bit fqss_infer_ola x N
// + fqss_infer_normalize, without the zeroed output, the weight buffer and the read-modify-write.  chunks [N][S][C][ld_chunk]
__global__ __launch_bounds__(256) void k_infer_ola_chunks(const float* __restrict__ chunks, const int* __restrict__ map, float* __restrict__ out,
                                                           int S, int C, int64_t L, int64_t seg, int64_t stride, int64_t N, int64_t ld_chunk,
                                                           int64_t ld_out) {
    const int dc = blockIdx.y, d = dc / C, c = dc % C;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < L; t += (int64_t)gridDim.x * 256) {
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
        out[((int64_t)d * C + c) * ld_out + t] = acc / wsum;
    }
}

}  // namespace fqss

using namespace fqss;

// est / ref: S rows of L samples; mom: S*S*5 doubles zeroed by the caller; db [S][S]; map (optional): 2*S ints
extern "C" int fqss_sisnr_matrix(const float* est, const float* ref, double* mom, float* db, int* map, int S, int64_t L, int64_t ld_e,
                                 int64_t ld_r, fqss_stream_t stream) {
    FQSS_REQUIRE(est && ref && mom && db, "null pointer");
    FQSS_REQUIRE(S > 0 && S <= 16 && L > 0 && ld_e >= L && ld_r >= L, "bad shape (S <= 16)");
    int64_t gx = cdiv(L, 4096);
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(k_sisnr_moments, dim3((unsigned)gx, (unsigned)(S * S)), dim3(256), 0, (hipStream_t)stream, est, ref, mom, S, L, ld_e, ld_r);
    hipLaunchKernelGGL(k_sisnr_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, mom, db, map, S, L, map != nullptr);
    return launch_status("fqss_sisnr_matrix");
}

extern "C" int fqss_infer_ola(const float* chunk, const int* map, float* out, float* sum_weight, int S, int C, int64_t n, int64_t seg,
                              int64_t start, int64_t ld_chunk, int64_t ld_out, fqss_stream_t stream) {
    FQSS_REQUIRE(chunk && out && sum_weight, "null pointer");
    FQSS_REQUIRE(S > 0 && C > 0 && S * C <= 65535 && n > 0 && n <= seg && start >= 0 && ld_chunk >= n && ld_out >= start + n, "bad shape");
    int64_t gx = cdiv(n, 1024);
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(k_infer_ola, dim3((unsigned)gx, (unsigned)(S * C)), dim3(256), 0, (hipStream_t)stream, chunk, map, out, sum_weight, S, C, n,
                       seg, start, ld_chunk, ld_out);
    return launch_status("fqss_infer_ola");
}

extern "C" int fqss_infer_normalize(float* out, const float* sum_weight, int64_t rows, int64_t L, int64_t ld, fqss_stream_t stream) {
    FQSS_REQUIRE(out && sum_weight, "null pointer");
    FQSS_REQUIRE(rows > 0 && L > 0 && ld >= L, "bad shape");
    int64_t gx = cdiv(L, 1024);
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(k_infer_normalize, dim3((unsigned)gx, (unsigned)(rows > 1024 ? 1024 : rows)), dim3(256), 0, (hipStream_t)stream, out,
                       sum_weight, rows, L, ld);
    return launch_status("fqss_infer_normalize");
}

// the chunk geometry shared by the three batched entry points: stride in [1, seg] (every sample is covered), N = ceil(L / stride)
static inline bool chunk_geometry_ok(int64_t L, int64_t seg, int64_t stride) { return L > 0 && seg > 0 && stride > 0 && stride <= seg; }

extern "C" int fqss_chunk_gather(const float* mix, float* out, int64_t L, int64_t seg, int64_t stride, int64_t k0, int G, fqss_stream_t stream) {
    FQSS_REQUIRE(mix && out, "null pointer");
    FQSS_REQUIRE(chunk_geometry_ok(L, seg, stride) && G > 0 && G <= 65535 && k0 >= 0 && k0 < cdiv(L, stride),
                 "bad shape (1 <= stride <= seg, 0 <= k0 < ceil(L / stride), 1 <= G <= 65535)");
    int64_t gx = cdiv(seg, 1024);
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(k_chunk_gather, dim3((unsigned)gx, (unsigned)G), dim3(256), 0, (hipStream_t)stream, mix, out, L, seg, stride, k0,
                       cdiv(L, stride));
    return launch_status("fqss_chunk_gather");
}

extern "C" int fqss_sisnr_chunks(const float* est, const float* ref, float* db, int* map, int G, int S, int64_t seg, int64_t stride, int64_t k0,
                                 int64_t L, int64_t ld_r, fqss_stream_t stream) {
    FQSS_REQUIRE(est && ref && db && map, "null pointer");
    FQSS_REQUIRE(S > 0 && S <= 16 && ld_r >= L, "bad shape (S <= 16, ld_r >= L)");
    FQSS_REQUIRE(chunk_geometry_ok(L, seg, stride) && G > 0 && k0 >= 0 && k0 < cdiv(L, stride),
                 "bad shape (1 <= stride <= seg, 0 <= k0 < ceil(L / stride), G >= 1)");
    hipLaunchKernelGGL(k_sisnr_chunks, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, est, ref, db, map, S, seg, stride, k0,
                       cdiv(L, stride), L, ld_r);
    return launch_status("fqss_sisnr_chunks");
}

extern "C" int fqss_infer_ola_chunks(const float* chunks, const int* map, float* out, int S, int C, int64_t L, int64_t seg, int64_t stride,
                                     int64_t ld_chunk, int64_t ld_out, fqss_stream_t stream) {
    FQSS_REQUIRE(chunks && out, "null pointer");
    FQSS_REQUIRE(S > 0 && C > 0 && S * C <= 65535 && chunk_geometry_ok(L, seg, stride) && ld_chunk >= seg && ld_out >= L,
                 "bad shape (1 <= stride <= seg, ld_chunk >= seg, ld_out >= L)");
    int64_t gx = cdiv(L, 1024);
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(k_infer_ola_chunks, dim3((unsigned)gx, (unsigned)(S * C)), dim3(256), 0, (hipStream_t)stream, chunks, map, out, S, C, L,
                       seg, stride, cdiv(L, stride), ld_chunk, ld_out);
    return launch_status("fqss_infer_ola_chunks");
}
