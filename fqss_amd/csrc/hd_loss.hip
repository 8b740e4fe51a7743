// hd_loss.hip -- the losses of the htdemucs environment (train_env/htdemucs_musdbhq/solver.py:333-390).  l1 with a teacher:
//   task_s = mean_b mean_{c,t} |est - src| ;  kd_s = mean_b ( w_bs * mean_{c,t} |est - fest| ) ,
//   w_bs = exp((sdr(src, fest) - sdr(src, est)) / 10) with demucs' new_sdr (third party, demucs~=4.0.0:
//   10 log10((sum src^2 + 1e-7) / (sum (src - x)^2 + 1e-7)) over channels and time), detached;
//   loss = sum_s wt_s ((1 - lambda) task_s + lambda kd_s) / sum_s wt_s,
//   d loss / d est = ct_s sign(est - src) + ck_bs sign(est - fest).
// fqss_hd_loss_x is the family around it: l1 | mse (solver.py:364-368), with or without the teacher, the nSDR of validation
// (solver.py:384-390) beside every loss.  No host synchronisation.
#include "eval_dev.h"

namespace fqss {

__device__ __forceinline__ float sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// ---- fqss_hd_loss_x: the loss family (l1 | mse, with or without a teacher, nSDR beside every one) ----
// Statement: include/fqss.h.  Three launches on the caller's stream, no atomics, no buffer the caller has to clear:
//   tiles   grid (tiles of the row, B*S).  A tile is kHdTile = 4096 samples = 256 lanes x 4 visits x 4 consecutive samples; a lane
//           reads one quad of every operand per visit (16-byte requests when the row bases allow it, one sample per request otherwise
//           -- the same samples in the same order either way), forms the differences in fp64 (exact) and adds its 16 samples in
//           (visit, sample) order; the workgroup adds its lanes on the DPP tree (block_sum) and STORES the tile's NS partials:
//           ws[(bs * NS + k) * ntiles + tile], k = A, Q, P (, K, F).  No teacher: NS = 3 and the fest stream is not compiled in.
//   finish  one workgroup.  Wave w adds the tile partials of the sums r = w, w + 4, ..: lane l takes tiles l, l + 64, .. in tile order,
//           then the DPP tree -- no barrier per sum, and the order is a function of the shape alone.  Thread s then forms source s
//           (the items in b order), thread 0 the weighted means over the sources; everything stays fp64 until it is stored.
//   grad    grid as tiles: one stream over est, src (, fest) with the per-(b, s) coefficients of the finish.
constexpr int kHdTile = FQSS_HD_LOSS_TILE;
static_assert(kHdTile == 256 * 4 * 4, "a tile is 256 lanes x 4 visits x 4 samples");

template <bool VEC, bool TEACHER>
__global__ __launch_bounds__(256) void k_hdx_tiles(const float* __restrict__ est, const float* __restrict__ fest, const float* __restrict__ src,
                                                    double* __restrict__ ws, int64_t N, int64_t ntiles) {
    constexpr int NS = TEACHER ? 5 : 3;
    __shared__ double smem[NS * 4];
    const int64_t bs = blockIdx.y;
    const float *e = est + bs * N, *s = src + bs * N, *f = TEACHER ? fest + bs * N : nullptr;
    double acc[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t i = (int64_t)blockIdx.x * kHdTile + (int64_t)(j * 256 + (int)threadIdx.x) * 4;
        if (i >= N) break;
        float ve[4], vs[4], vf[4];
        load_quad<VEC>(e, i, N, ve);        // past N: zeros in every operand, which add nothing to any sum
        load_quad<VEC>(s, i, N, vs);
        if (TEACHER) load_quad<VEC>(f, i, N, vf);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double sv = (double)vs[q], d = (double)ve[q] - sv;
            acc[0] += fabs(d);
            acc[1] += d * d;
            acc[2] += sv * sv;
            if (TEACHER) {
                const double fv = (double)vf[q], df = sv - fv;
                acc[3] += fabs((double)ve[q] - fv);
                acc[4] += df * df;
            }
        }
    }
    block_sum<double, NS>(acc, smem);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) ws[(bs * NS + k) * ntiles + blockIdx.x] = acc[k];
    }
}

// ws behind the tile partials: tot [B*S][NS] (the sums of an item), then per [3][S] = (loss_s, reco_s, nsdr_s) in fp64.
// out: [0] loss, [1] reco, [2] nsdr, then loss_s, reco_s, nsdr_s, kd_s [S] each, then w [B][S];  coef [B][S][2] = (c0, c1):
// gest = c0 * sign(est - src) + c1 * sign(est - fest) for l1, c0 * (est - src) for mse
template <bool TEACHER>
__global__ __launch_bounds__(256) void k_hdx_finish(double* __restrict__ ws, const float* __restrict__ wt, float* __restrict__ out,
                                                     float* __restrict__ coef, int B, int S, int64_t N, int64_t ntiles, float lambda, int kind) {
    constexpr int NS = TEACHER ? 5 : 3;
    const int64_t nsums = (int64_t)B * S * NS;
    double* tot = ws + nsums * ntiles;
    double* per = tot + nsums;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t r = wave; r < nsums; r += 4) {     // wave-uniform bounds: all 64 lanes reach the DPP tree
        const double* p = ws + r * ntiles;
        double v = 0.0;
        for (int64_t t = lane; t < ntiles; t += 64) v += p[t];
        v = wave_sum63(v);
        if (lane == 63) tot[r] = v;
    }
    __threadfence_block();
    __syncthreads();
    double wsum = 0.0;
    for (int s = 0; s < S; ++s) wsum += wt[s];
    const double dn = (double)N, lam = (double)lambda;
    for (int s = threadIdx.x; s < S; s += 256) {
        double ls = 0.0, rs = 0.0, ns = 0.0, ks = 0.0;
        for (int b = 0; b < B; ++b) {
            const int64_t bs = (int64_t)b * S + s;
            const double* q = tot + bs * NS;
            const double A = q[0], Q = q[1], P = q[2];
            ns += 10.0 * log10((P + 1e-7) / (Q + 1e-7));
            float w = 1.0f;
            if (TEACHER) {      // the two SDRs and the weight in fp32 (include/fqss.h)
                const float sdr_t = 10.0f * log10f((float)((P + 1e-7) / (q[4] + 1e-7)));
                const float sdr_q = 10.0f * log10f((float)((P + 1e-7) / (Q + 1e-7)));
                w = expf((sdr_t - sdr_q) / 10.0f);
                ks += (double)w * (q[3] / dn);
            }
            out[3 + 4 * S + bs] = w;
            if (kind == 0) {
                ls += A / dn;
                rs += A / dn;
            } else {
                ls += Q / dn;
                rs += sqrt(Q / dn);
            }
            const double c = (double)wt[s] / wsum;
            float c0, c1 = 0.0f;
            if (TEACHER) {
                c0 = (float)(c * (1.0 - lam) / ((double)B * dn));
                c1 = (float)(c * lam * (double)w / ((double)B * dn));
            } else {
                c0 = (float)(c * (kind == 0 ? 1.0 : 2.0) / ((double)B * dn));
            }
            coef[bs * 2 + 0] = c0;
            coef[bs * 2 + 1] = c1;
        }
        ls /= B;
        rs /= B;
        ns /= B;
        ks /= B;
        if (TEACHER) ls = (1.0 - lam) * ls + lam * ks;      // reco_s stays the task term
        per[s] = ls;
        per[S + s] = rs;
        per[2 * S + s] = ns;
        out[3 + s] = (float)ls;
        out[3 + S + s] = (float)rs;
        out[3 + 2 * S + s] = (float)ns;
        out[3 + 3 * S + s] = (float)ks;
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x < 3) {
        double v = 0.0;
        for (int s = 0; s < S; ++s) v += (double)wt[s] * per[threadIdx.x * S + s];
        out[threadIdx.x] = (float)(v / wsum);
    }
}

// MODE 0: l1 without a teacher, 1: mse, 2: l1 with a teacher
template <bool VEC, int MODE>
__global__ __launch_bounds__(256) void k_hdx_grad(const float* __restrict__ est, const float* __restrict__ fest, const float* __restrict__ src,
                                                   const float* __restrict__ coef, float* __restrict__ gest, int64_t N) {
    const int64_t bs = blockIdx.y;
    const float c0 = coef[bs * 2], c1 = coef[bs * 2 + 1];
    const float *e = est + bs * N, *s = src + bs * N, *f = MODE == 2 ? fest + bs * N : nullptr;
    float* g = gest + bs * N;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t i = (int64_t)blockIdx.x * kHdTile + (int64_t)(j * 256 + (int)threadIdx.x) * 4;
        if (i >= N) break;
        float ve[4], vs[4], vf[4], r[4];
        load_quad<VEC>(e, i, N, ve);
        load_quad<VEC>(s, i, N, vs);
        if (MODE == 2) load_quad<VEC>(f, i, N, vf);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float d = ve[q] - vs[q];
            r[q] = MODE == 1 ? c0 * d : c0 * sgn(d);
            if (MODE == 2) r[q] += c1 * sgn(ve[q] - vf[q]);
        }
        if (VEC && i + 4 <= N) {
            *reinterpret_cast<float4*>(g + i) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (i + q < N) g[i + q] = r[q];
        }
    }
}

template <bool TEACHER>
static void hdx_launch(const float* est, const float* fest, const float* src, const float* wt, double* ws, float* out, float* coef, float* gest,
                       int B, int S, int64_t N, float lambda, int kind, hipStream_t st) {
    const int64_t ntiles = cdiv(N, kHdTile);
    const bool rows16 = (N & 3) == 0 || B * S == 1;     // every row base is as aligned as the tensor's
    const bool vec = rows16 && aligned16(est) && aligned16(src) && (!TEACHER || aligned16(fest));
    const dim3 grid((unsigned)ntiles, (unsigned)(B * S)), block(256);
    if (vec)
        hipLaunchKernelGGL((k_hdx_tiles<true, TEACHER>), grid, block, 0, st, est, fest, src, ws, N, ntiles);
    else
        hipLaunchKernelGGL((k_hdx_tiles<false, TEACHER>), grid, block, 0, st, est, fest, src, ws, N, ntiles);
    hipLaunchKernelGGL(k_hdx_finish<TEACHER>, dim3(1), block, 0, st, ws, wt, out, coef, B, S, N, ntiles, lambda, kind);
    if (gest == nullptr) return;
    constexpr int MODE0 = TEACHER ? 2 : 0;
    if (vec && aligned16(gest)) {
        if (kind == 1)
            hipLaunchKernelGGL((k_hdx_grad<true, 1>), grid, block, 0, st, est, fest, src, coef, gest, N);
        else
            hipLaunchKernelGGL((k_hdx_grad<true, MODE0>), grid, block, 0, st, est, fest, src, coef, gest, N);
    } else {
        if (kind == 1)
            hipLaunchKernelGGL((k_hdx_grad<false, 1>), grid, block, 0, st, est, fest, src, coef, gest, N);
        else
            hipLaunchKernelGGL((k_hdx_grad<false, MODE0>), grid, block, 0, st, est, fest, src, coef, gest, N);
    }
}

}  // namespace fqss

using namespace fqss;

extern "C" int64_t fqss_hd_loss_x_ws_doubles(int B, int S, int64_t N, int teacher) {
    if (B <= 0 || S <= 0 || N <= 0 || (int64_t)B * S > 65535) return 0;
    return (int64_t)B * S * (teacher ? 5 : 3) * (cdiv(N, kHdTile) + 1) + 3 * (int64_t)S;
}

// est / src (/ fest) [B][S][N] dense; wt [S]; ws: fqss_hd_loss_x_ws_doubles(B, S, N, fest != null) doubles, uninitialised;
// out: 3 + 4S + B*S floats; coef: B*S*2 floats; gest may be null (evaluation only)
extern "C" int fqss_hd_loss_x(const float* est, const float* fest, const float* src, const float* wt, double* ws, float* out, float* coef,
                              float* gest, int B, int S, int64_t N, float kd_lambda, int kind, fqss_stream_t stream) {
    FQSS_REQUIRE(kind == 0 || kind == 1, "kind: 0 = l1, 1 = mse");
    FQSS_REQUIRE(kind == 0 || fest == nullptr, "the mse loss has no distillation term (solver.py:364): fest must be null");
    FQSS_REQUIRE(fest != nullptr || kd_lambda == 0.0f, "kd_lambda > 0 needs a teacher estimate (fest is null)");
    FQSS_REQUIRE(B >= 0 && S > 0 && N >= 0 && (int64_t)B * S <= 65535, "bad shape");
    if (B == 0 || N == 0) return FQSS_OK;
    FQSS_REQUIRE(est && src && wt && ws && out && coef, "null pointer");
    if (fest != nullptr)
        hdx_launch<true>(est, fest, src, wt, ws, out, coef, gest, B, S, N, kd_lambda, kind, (hipStream_t)stream);
    else
        hdx_launch<false>(est, fest, src, wt, ws, out, coef, gest, B, S, N, kd_lambda, kind, (hipStream_t)stream);
    return launch_status("fqss_hd_loss_x");
}
