// bss_eval.hip -- BSS-eval SDR / SIR / SAR of S <= 3 estimates against S targets (fqss_bss_eval in include/fqss.h is the definition; it
// restates the published form of mir_eval / fast_bss_eval's bss_eval_sources, both third party and absent).  With zero-extended (linear)
// correlations the three energies are quadratic forms of the correlation vectors, so no signal is ever filtered:
//   E_all = d^T G^-1 d  (projection on the T lagged copies of ALL targets: G is SPD block-Toeplitz of order n = S T),
//   E_tgt = d_q^T G_qq^-1 d_q  (projection on the lagged copies of the estimate's own target: the coh of fqss_sdr).
// Stream-ordered launches, nothing read back, all sums in fp64, no floating-point atomics -- the same bits every run:
//   k_bss_corr<S>  grid (time tiles): the tile and its halo of all 2S signals staged in LDS once; every ref_i x {ref_k, est_j} lag sum
//                  and the 4S moments of the tile -> ws partials
//   k_bss_reduce   one workgroup per correlation sequence: partials added in tile order, mean correction and normalisation
//   k_bss_assemble G (n x n) and, as S more ROWS below it, the right-hand sides d_j^T
//   k_bss_tgt      one workgroup per estimate: the Levinson recursion of fqss_sdr (eval_dev.h) -> E_tgt
//   per 32-column panel (S > 1): k_bss_panel (the diagonal block factored in LDS, the panel below it solved, one row per thread) and
//                  k_bss_syrk (trailing update of the lower triangle on v_mfma_f64_16x16x4_f64, the panel's tiles in LDS).
//                  The right-hand-side rows ride along as rows of the panel: when the last panel is done they hold y_j = L^-1 d_j,
//                  and E_all = |y_j|^2 -- the forward substitutions cost no launch of their own and there is no back substitution.
//   k_bss_finish   E_all and the three ratios with the NaN / +inf rules
#include "eval_dev.h"

namespace fqss {

constexpr int kBssTile = 512;       // time samples per workgroup of k_bss_corr
constexpr int kBssMaxT = kLevMaxF;  // filter_length <= 512: two adjacent lags per thread of a 256-thread workgroup
constexpr int kBssMaxS = 3;
constexpr int kBssNB = 32;          // panel width of the factorisation (tests/test_gpu_bss_eval.py names it: PANEL)
constexpr int kBssRows = 128;       // rows of the panel one workgroup of k_bss_panel solves: one per thread
constexpr int kBssMT = 64;          // tile of the trailing update: 4 waves x (2 x 2) MFMA blocks of 16 x 16
constexpr int kBssMisc = 16;        // [0..S) E_j, [3..3+S) E_tgt, [6..6+S) own Toeplitz solve fine (1 / 0), [9] a pivot was not positive

struct BssWs {      // offsets in doubles
    int64_t part, stride, corr, misc, g, total;
};
__host__ __device__ static inline BssWs bss_ws(int S, int64_t L, int T) {
    BssWs w;
    const int64_t n = (int64_t)S * T;
    w.stride = 2 * (int64_t)S * S * T + 4 * S;              // per tile: [ref i][signal m < 2S][T] lag sums, then (sum x^2, sum x) per signal
    w.part = 0;
    w.corr = w.part + ((L + kBssTile - 1) / kBssTile) * w.stride;      // A [i][k][T], then B [j][i][T] (= d_j), normalised
    w.misc = w.corr + 2 * (int64_t)S * S * T;
    w.g = w.misc + kBssMisc;                                 // (n + S) rows of n: G, then d_j^T
    w.total = w.g + (n + S) * n;
    return w;
}

// Signals m < S are the targets, m >= S the estimates.  Thread j owns lags 2j and 2j + 1 of every sequence.  The LDS copy is fp32,
// widened on the read: the loop is fed by LDS window reads, and fp32 halves their bytes (8 B per lane and pair of samples, not 16) and
// the footprint (24 KB at S = 3, not 48 KB) for two v_cvt per window read beside four fp64 FMAs; the widened values are exact.  Per pair of
// time samples a wave reads ref_i's two samples (one address: a broadcast) and, per signal, the next two floats of its sliding window
// (8 B per lane, consecutive across lanes) for 8 S fp64 FMAs per lane; ref_i's samples are reused across all 2S windows.
template <int S>
__global__ __launch_bounds__(256) void k_bss_corr(const float* __restrict__ est, const float* __restrict__ ref, double* __restrict__ part,
                                                  int T, int64_t L, int64_t ld_e, int64_t ld_r, int64_t stride) {
    constexpr int M = 2 * S, W = kBssTile + kBssMaxT;
    __shared__ __attribute__((aligned(16))) float sig[M][W];
    __shared__ double smem[2 * M * 4];
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * kBssTile;
    for (int m = 0; m < M; ++m) {
        const float* x = m < S ? ref + m * ld_r : est + (m - S) * ld_e;
        for (int i = tid; i < W; i += 256) sig[m][i] = t0 + i < L ? x[t0 + i] : 0.0f;
    }
    __syncthreads();
    double* out = part + (int64_t)blockIdx.x * stride;
    const int k0 = 2 * tid;
    if (k0 < T) {
        for (int i = 0; i < S; ++i) {
            const float2* a2 = reinterpret_cast<const float2*>(sig[i]);
            double acc[M][2];
            float2 x[M];
#pragma unroll
            for (int m = 0; m < M; ++m) {
                acc[m][0] = acc[m][1] = 0.0;
                x[m] = *reinterpret_cast<const float2*>(&sig[m][k0]);
            }
#pragma unroll 2
            for (int u = 0; u < kBssTile / 2; ++u) {
                const float2 a = a2[u];
                const double ax = (double)a.x, ay = (double)a.y;
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const float2 xn = *reinterpret_cast<const float2*>(&sig[m][k0 + 2 * u + 2]);
                    const double x0 = (double)x[m].x, x1 = (double)x[m].y, x2 = (double)xn.x;
                    acc[m][0] = fma(ax, x0, acc[m][0]);
                    acc[m][1] = fma(ax, x1, acc[m][1]);
                    acc[m][0] = fma(ay, x1, acc[m][0]);
                    acc[m][1] = fma(ay, x2, acc[m][1]);
                    x[m] = xn;
                }
            }
#pragma unroll
            for (int m = 0; m < M; ++m) {
                double* o = out + ((int64_t)i * M + m) * T;
                o[k0] = acc[m][0];
                if (k0 + 1 < T) o[k0 + 1] = acc[m][1];
            }
        }
    }
    double mom[2 * M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        double q = 0.0, s = 0.0;
        for (int i = tid; i < kBssTile; i += 256) {
            const double v = (double)sig[m][i];
            q = fma(v, v, q);
            s += v;
        }
        mom[2 * m] = q;
        mom[2 * m + 1] = s;
    }
    block_sum<double, 2 * M>(mom, smem);
    if (tid == 0)
        for (int i = 0; i < 2 * M; ++i) out[(int64_t)M * S * T + i] = mom[i];
}

// sum of x[i0 .. i0 + n) in index order
__device__ __forceinline__ double bss_span_sum(const float* __restrict__ x, int64_t i0, int64_t n) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += (double)x[i0 + i];
    return s;
}

// Sequence q < S^2: A_ik (x = ref_i, y = ref_k), q >= S^2: B_ij (x = ref_i, y = est_j).  With zero_mean the lag sums of the centred
// signals follow from the raw ones, the totals and the sums of the first / last lag samples, as in k_sdr_finish:
//   sum_{t < L - a} (x[t] - mx)(y[t + a] - my) = c[a] - my (Sx - last_a(x)) - mx (Sy - first_a(y)) + (L - a) mx my
__global__ __launch_bounds__(256) void k_bss_reduce(const float* __restrict__ est, const float* __restrict__ ref, double* __restrict__ ws, int S,
                                                    int T, int64_t L, int64_t ld_e, int64_t ld_r, int64_t ntiles, int zero_mean) {
    __shared__ double mom[4];
    const BssWs w = bss_ws(S, L, T);
    const int tid = threadIdx.x, q = blockIdx.x, M = 2 * S;
    const bool isB = q >= S * S;
    const int i = (isB ? q - S * S : q) / S, k = (isB ? q - S * S : q) % S, m = isB ? S + k : k;
    const float *x = ref + i * ld_r, *y = isB ? est + k * ld_e : ref + k * ld_r;
    const double* part = ws + w.part;
    if (tid < 4) {      // (sum x^2, sum x, sum y^2, sum y) in tile order
        const int64_t at = (int64_t)M * S * T + 2 * (tid < 2 ? i : m) + (tid & 1);
        double s = 0.0;
        for (int64_t tile = 0; tile < ntiles; ++tile) s += part[tile * w.stride + at];
        mom[tid] = s;
    }
    __syncthreads();
    const double n = (double)L, Sx = mom[1], Sy = mom[3];
    const double mx = zero_mean ? Sx / n : 0.0, my = zero_mean ? Sy / n : 0.0;
    const double xx = mom[0] - mx * Sx, yy = mom[2] - my * Sy;
    const double nx = fmax(sqrt(fmax(xx, 0.0)), 1e-6), ny = fmax(sqrt(fmax(yy, 0.0)), 1e-6);
    double* dst = ws + w.corr + (isB ? ((int64_t)S * S + (int64_t)k * S + i) * T : (int64_t)q * T);
    for (int a = tid; a < T; a += 256) {
        double v = 0.0;
        if (a < L) {
            for (int64_t tile = 0; tile < ntiles; ++tile) v += part[tile * w.stride + ((int64_t)i * M + m) * T + a];
            if (zero_mean) {
                const double tail_x = bss_span_sum(x, L - a, a), head_y = bss_span_sum(y, 0, a);
                v = v - my * (Sx - tail_x) - mx * (Sy - head_y) + (double)(L - a) * mx * my;
            }
            v = v / (nx * ny);
        }
        dst[a] = v;
    }
    if (tid == 0) {
        if (isB && i == 0) ws[w.misc + k] = yy / (ny * ny);      // E_j of the normalised estimate
        if (q == 0) ws[w.misc + 9] = 0.0;
    }
}

// G[(i, a)][(k, b)] = A_ik[a - b] (= A_ki[b - a] below zero) + load_diag on the diagonal; row n + j = d_j^T
__global__ __launch_bounds__(256) void k_bss_assemble(double* __restrict__ ws, int S, int T, int64_t L, double load_diag) {
    const BssWs w = bss_ws(S, L, T);
    const int n = S * T, row = blockIdx.x;
    const double* A = ws + w.corr;
    double* g = ws + w.g + (int64_t)row * n;
    if (row >= n) {
        const double* d = A + ((int64_t)S * S + (int64_t)(row - n) * S) * T;
        for (int c = threadIdx.x; c < n; c += 256) g[c] = d[c];
        return;
    }
    const int i = row / T, a = row % T;
    for (int c = threadIdx.x; c < n; c += 256) {
        const int k = c / T, b = c % T;
        double v = a >= b ? A[((int64_t)i * S + k) * T + (a - b)] : A[((int64_t)k * S + i) * T + (b - a)];
        if (c == row && load_diag >= 0.0) v += load_diag;      // (a negative or NaN load_diag: none)
        g[c] = v;
    }
}

// E_tgt of estimate j against target q = tgt[j]: r = A_qq (+ load_diag), b = B_qj through the recursion of fqss_sdr
__global__ __launch_bounds__(256) void k_bss_tgt(double* __restrict__ ws, const int* __restrict__ tgt, int S, int T, int64_t L, double load_diag) {
    __shared__ double r_s[kLevMaxF], b_s[kLevMaxF], a_s[2][kLevMaxF], red[8];
    const BssWs w = bss_ws(S, L, T);
    const int tid = threadIdx.x, j = blockIdx.x;
    int q = tgt != nullptr ? tgt[j] : j;
    q = q < 0 ? 0 : (q >= S ? S - 1 : q);
    const double *A = ws + w.corr + ((int64_t)q * S + q) * T, *B = ws + w.corr + ((int64_t)S * S + (int64_t)j * S + q) * T;
    for (int s = 0; s < 2; ++s) {
        const int k = tid + 256 * s;
        a_s[0][k] = k == 0 ? 1.0 : 0.0;
        a_s[1][k] = 0.0;
        if (k < T) {
            r_s[k] = A[k] + ((k == 0 && load_diag >= 0.0) ? load_diag : 0.0);
            b_s[k] = B[k];
        }
    }
    __syncthreads();
    bool ok;
    const double coh = levinson_coh(r_s, b_s, a_s, red, T, ok);
    if (tid == 0) {
        ws[w.misc + 3 + j] = coh;
        ws[w.misc + 6 + j] = (ok && isfinite(coh)) ? 1.0 : 0.0;
    }
}

// One panel of the right-looking factorisation: columns [k0, k0 + kb) of the (n + S) x n array.  Every workgroup factors the kb x kb
// diagonal block in LDS for itself (32 steps on a 32 x 32 block: cheaper than a launch of its own, and the same bits in each).  The rows
// below are solved one per thread, x = a L11^-T by forward substitution: the workgroup's 128 x 32 piece of the panel goes through LDS
// (whole 256-byte row pieces per 32 threads on the way in and out; row stride 33 doubles, so the 64 rows of a wave fall in different
// banks) and L11 is read as broadcasts.  Held in registers instead, the row and the unrolled substitution took 256 VGPRs and spilled.
// The factored diagonal block is not stored: the trailing update needs the solved panel only and k_bss_finish only the right-hand-side
// rows, so no workgroup writes what another one reads in this launch.
__global__ __launch_bounds__(kBssRows) void k_bss_panel(double* __restrict__ g, double* __restrict__ flag, int n, int rows, int k0) {
    __shared__ double l11[kBssNB][kBssNB + 1], xs[kBssRows][kBssNB + 1];
    const int tid = threadIdx.x, kb = min(kBssNB, n - k0);
    for (int e = tid; e < kBssNB * kBssNB; e += kBssRows) {
        const int r = e / kBssNB, c = e % kBssNB;
        l11[r][c] = (r < kb && c <= r) ? g[(int64_t)(k0 + r) * n + k0 + c] : (r == c ? 1.0 : 0.0);
    }
    __syncthreads();
    bool bad = false;
    for (int j = 0; j < kb; ++j) {
        const double p = l11[j][j];
        bad = bad || !(p > 0.0);
        const double d = sqrt(p);
        __syncthreads();
        if (tid >= j && tid < kb) l11[tid][j] = tid == j ? d : l11[tid][j] / d;
        __syncthreads();
        const int m = kb - 1 - j;      // trailing block of m x m, lower triangle: element e -> (r, c), c <= r
        for (int e = tid; e < m * m; e += kBssRows) {
            const int r = j + 1 + e / m, c = j + 1 + e % m;
            if (c <= r) l11[r][c] = l11[r][c] - l11[r][j] * l11[c][j];
        }
        __syncthreads();
    }
    if (bad && blockIdx.x == 0 && tid == 0) *flag = 1.0;
    const int row0 = k0 + kb + blockIdx.x * kBssRows;
    for (int e = tid; e < kBssRows * kBssNB; e += kBssRows) {      // 32 consecutive doubles of a row per 32 threads
        const int r = e / kBssNB, c = e % kBssNB;
        if (row0 + r < rows && c < kb) xs[r][c] = g[(int64_t)(row0 + r) * n + k0 + c];
    }
    __syncthreads();
    if (row0 + tid < rows) {
        double* x = xs[tid];
        for (int c = 0; c < kb; ++c) {
            const double* l = l11[c];
            double v = x[c];
            for (int m = 0; m < c; ++m) v = fma(-x[m], l[m], v);
            x[c] = v / l[c];
        }
    }
    __syncthreads();
    for (int e = tid; e < kBssRows * kBssNB; e += kBssRows) {
        const int r = e / kBssNB, c = e % kBssNB;
        if (row0 + r < rows && c < kb) g[(int64_t)(row0 + r) * n + k0 + c] = xs[r][c];
    }
}

// Trailing update C[r][c] -= sum_k P[r][k] P[c][k] over the panel's kb columns, rows r in [k1, rows), columns c in [k1, n), c <= r (the
// right-hand-side rows r >= n take every column).  Workgroup (bx, by), bx <= by, owns the 64 x 64 tile at (k1 + 64 by, k1 + 64 bx); its
// two 64 x 32 panel tiles sit in LDS (row stride 33 doubles: the 16 rows a fragment read touches fall in 16 different banks), zero where
// the row or the panel column does not exist, so the k loop is whole and the edge tiles are handled by predicated loads and stores.
// Wave w owns the 32 x 32 quadrant (w >> 1, w & 1) as 2 x 2 blocks of v_mfma_f64_16x16x4_f64: lane l feeds A[l % 16][l / 16] and
// B[l / 16][l % 16] -- both are panel[row l % 16][column l / 16] -- and holds D[4 v + l / 16][l % 16] in accumulator register v.
typedef double f64x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_bss_syrk(double* __restrict__ g, int n, int rows, int k0, int kb) {
    if (blockIdx.x > blockIdx.y) return;
    __shared__ double pr[kBssMT][kBssNB + 1], pc[kBssMT][kBssNB + 1];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, k1 = k0 + kb;
    const int r0 = k1 + kBssMT * blockIdx.y, c0 = k1 + kBssMT * blockIdx.x;
    for (int e = tid; e < kBssMT * kBssNB; e += 256) {
        const int r = e / kBssNB, c = e % kBssNB;
        pr[r][c] = (r0 + r < rows && c < kb) ? g[(int64_t)(r0 + r) * n + k0 + c] : 0.0;
        pc[r][c] = (c0 + r < n && c < kb) ? g[(int64_t)(c0 + r) * n + k0 + c] : 0.0;
    }
    __syncthreads();
    const int qr = 32 * (wv >> 1), qc = 32 * (wv & 1), li = lane & 15, lk = lane >> 4;
    f64x4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < kBssNB; ks += 4) {
        double a[2], b[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            a[u] = pr[qr + 16 * u + li][ks + lk];
            b[u] = pc[qc + 16 * u + li][ks + lk];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[v], acc[u][v], 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = r0 + qr + 16 * u + 4 * e + lk, c = c0 + qc + 16 * v + li;
                if (r < rows && c < n && (c <= r || r >= n)) {
                    double* p = g + (int64_t)r * n + c;
                    *p = *p - acc[u][v][e];
                }
            }
}

__device__ __forceinline__ double bss_ratio_db(double num, double den) {
    if (den <= 0.0 && num > 0.0) return (double)INFINITY;
    return 10.0 * log10(num / den);
}

// E_all = |y_j|^2 from the right-hand-side rows (wave sums on the DPP tree, the four waves in wave order), then out [3][S]
__global__ __launch_bounds__(256) void k_bss_finish(const double* __restrict__ ws, double* __restrict__ out, int S, int T, int64_t L) {
    __shared__ double red[4];
    const BssWs w = bss_ws(S, L, T);
    const int tid = threadIdx.x, j = blockIdx.x, n = S * T;
    const double* m = ws + w.misc;
    double e_all = 0.0;
    if (S > 1) {
        const double* y = ws + w.g + (int64_t)(n + j) * n;
        for (int c = tid; c < n; c += 256) e_all = fma(y[c], y[c], e_all);
        e_all = wave_sum63(e_all);
        if ((tid & 63) == 63) red[tid >> 6] = e_all;
        __syncthreads();
        e_all = ((red[0] + red[1]) + red[2]) + red[3];
    }
    if (tid != 0) return;
    const double e_j = m[j], e_tgt = m[3 + j];
    if (S == 1) e_all = e_tgt;
    const bool ok = m[6 + j] != 0.0 && (S == 1 || m[9] == 0.0) && isfinite(e_all);
    out[j] = ok ? bss_ratio_db(e_tgt, e_j - e_tgt) : (double)NAN;
    out[S + j] = ok ? bss_ratio_db(e_tgt, e_all - e_tgt) : (double)NAN;
    out[2 * S + j] = ok ? bss_ratio_db(e_all, e_j - e_all) : (double)NAN;
}

}  // namespace fqss

using namespace fqss;

// doubles of workspace of fqss_bss_eval: the tile partials, the reduced correlations and the (S T + S) x (S T) system; 0 for arguments
// fqss_bss_eval refuses
extern "C" int64_t fqss_bss_eval_ws_doubles(int S, int64_t L, int filter_length) {
    if (S < 1 || S > kBssMaxS || L < 1 || filter_length < 1 || filter_length > kBssMaxT) return 0;
    return bss_ws(S, L, filter_length).total;
}

extern "C" int fqss_bss_eval(const float* est, const float* ref, const int* tgt, double* ws, int64_t ws_doubles, double* out, int S, int64_t L,
                             int64_t ld_e, int64_t ld_r, int filter_length, int zero_mean, double load_diag, fqss_stream_t stream) {
    FQSS_REQUIRE(est && ref && ws && out, "null pointer");
    FQSS_REQUIRE(S >= 1 && S <= kBssMaxS && L >= 1 && ld_e >= L && ld_r >= L, "bad shape (1 <= S <= 3, L >= 1, ld >= L)");
    FQSS_REQUIRE(filter_length >= 1 && filter_length <= kBssMaxT, "filter_length outside 1..512");
    const int64_t ntiles = cdiv(L, kBssTile);
    FQSS_REQUIRE(ntiles <= 0x7fffffff, "L too long");
    FQSS_REQUIRE(ws_doubles >= fqss_bss_eval_ws_doubles(S, L, filter_length), "workspace shorter than fqss_bss_eval_ws_doubles");
    const hipStream_t st = (hipStream_t)stream;
    const int T = filter_length, n = S * T, rows = n + S;
    const BssWs w = bss_ws(S, L, T);
    auto corr = S == 1 ? k_bss_corr<1> : (S == 2 ? k_bss_corr<2> : k_bss_corr<3>);
    hipLaunchKernelGGL(corr, dim3((unsigned)ntiles), dim3(256), 0, st, est, ref, ws + w.part, T, L, ld_e, ld_r, w.stride);
    hipLaunchKernelGGL(k_bss_reduce, dim3(2 * S * S), dim3(256), 0, st, est, ref, ws, S, T, L, ld_e, ld_r, ntiles, zero_mean);
    hipLaunchKernelGGL(k_bss_tgt, dim3(S), dim3(256), 0, st, ws, tgt, S, T, L, load_diag);
    if (S > 1) {      // at S = 1 E_all is E_tgt by definition: no system
        double* g = ws + w.g;
        hipLaunchKernelGGL(k_bss_assemble, dim3(rows), dim3(256), 0, st, ws, S, T, L, load_diag);
        for (int k0 = 0; k0 < n; k0 += kBssNB) {
            const int kb = n - k0 < kBssNB ? n - k0 : kBssNB, below = rows - (k0 + kb);      // below >= S: the right-hand-side rows
            hipLaunchKernelGGL(k_bss_panel, dim3((unsigned)cdiv(below, kBssRows)), dim3(kBssRows), 0, st, g, ws + w.misc + 9, n, rows, k0);
            if (k0 + kb < n) {
                const unsigned tr = (unsigned)cdiv(below, kBssMT), tc = (unsigned)cdiv(n - (k0 + kb), kBssMT);
                hipLaunchKernelGGL(k_bss_syrk, dim3(tc, tr), dim3(256), 0, st, g, n, rows, k0, kb);
            }
        }
    }
    hipLaunchKernelGGL(k_bss_finish, dim3(S), dim3(256), 0, st, (const double*)ws, out, S, T, L);
    return launch_status("fqss_bss_eval");
}
