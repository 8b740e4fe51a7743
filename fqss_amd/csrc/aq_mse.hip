// aq_mse.hip -- the histogram-MSE activation observer (GradientActivationFakeQuantize_MSE, qat_quant.py:245-326 of the reference: np.histogram of
// each of the first 50 activations, merge_hist, the 100 x 100 search of mse_minmax_range).  The arithmetic is stated in include/fqss.h at
// fqss_aq_hist / fqss_aq_mse_search; everything behind the histogram is fp64.  Nothing is read back by the host: the tensor's (min, max)
// come from obs_ws, the merged grid's size M lives in the workspace and the kernels behind it are launched over its upper bound.
//   k_aq_hist      grid-stride over the rows of x (one row of n values, or the padded rows of an activation buffer), 16-B loads where the address allows (a scalar head / tail by workgroup 0), the bin index in fp64 with
//                  numpy's one-step edge correction, one privatised 512-bin uint32 histogram per wave in LDS (integer LDS atomics; lanes that
//                  share the first active lane's bin -- twice over -- add their popcount once: a post-ReLU tensor puts half its values into one
//                  bin), one flush per workgroup with global integer atomics
//   k_aq_hist_fin  rng_row = (lo, hi) or (NaN, NaN), obs_ws reset -- behind k_aq_hist, whose workgroups all read obs_ws
//   k_aq_prep      one workgroup per quantizer: a lane per row (exact cumulative counts, the row's edges), then bmin / bmax / w / M
//   k_aq_merge     a thread per merged point m: b[m] and vals[m] (np.interp of every row's cumulative counts at b[m], b[m + 1]) in global memory
//   k_aq_search    workgroup = candidate i and four j, a wave per candidate: b / vals staged through LDS in tiles of 1024, a lane sums its
//                  elements (stride 64) in tile order, the DPP tree joins the lanes -- an order that does not depend on the grid
//   k_aq_argmin    one workgroup: the strict minimum of the 10 000 errors, ties to the smaller 100 i + j; writes qmin / qmax
// Integer atomics only in the histogram, no atomics behind it: the same bits every run and on any stream.
#include "fqss_dev.h"

namespace fqss {

constexpr int kAqBins = FQSS_AQ_HIST_BINS, kAqRows = FQSS_AQ_MSE_MAX_ROWS, kAqMaxM = FQSS_AQ_MSE_MAX_BINS, kAqN = FQSS_AQ_MSE_N;
constexpr int kAqTile = 1024;            // elements of b / vals per LDS tile of k_aq_search (16 KB)
constexpr int kAqJPerWg = 4;             // candidates per workgroup of k_aq_search (one per wave)

// where the workspace keeps what (doubles from its start; the same on the host and on the device; callers ask fqss_aq_mse_ws_offset)
struct AqLayout {
    int64_t hdr, rows, cum, b, vals, err, total;
};
__host__ __device__ static inline AqLayout aq_layout(int T) {
    AqLayout w;
    w.hdr = 0;                                   // bmin, bmax, w, M, number of non-void rows
    w.rows = 16;                                 // [64][2] (lo_t, hi_t) after the lo == hi widening; NaN: void
    w.cum = w.rows + 2 * kAqRows;                // [T][513] exact cumulative counts
    w.b = w.cum + (int64_t)T * (kAqBins + 1);    // [65536] merged points
    w.vals = w.b + kAqMaxM;                      // [65536] merged weights (M - 1 of them)
    w.err = w.vals + kAqMaxM;                    // [100][100] e(i, j)
    w.total = w.err + kAqN * kAqN;
    return w;
}

__device__ __forceinline__ bool aq_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }      // false for NaN and inf

// the bin of v on the 512 uniform bins over [lo, hi]: numpy's first guess and its correction by one against the edges
__device__ __forceinline__ int aq_bin(double v, double lo, double span, double step) {
    const double f = (v - lo) / span * (double)kAqBins;
    int k = f >= (double)kAqBins ? kAqBins - 1 : (f > 0.0 ? (int)f : 0);       // (NaN -> 0: the index stays inside the row)
    if (v < lo + (double)k * step) {
        k = k > 0 ? k - 1 : 0;
    } else if (k < kAqBins - 1 && v >= lo + (double)(k + 1) * step) {
        k += 1;
    }
    return k;
}

// one count into the wave's histogram for every ACTIVE lane.  Two rounds of: the lanes whose bin is the first pending lane's add their number
// once; what is left after that adds one each.
__device__ __forceinline__ void aq_hist_add(uint32_t* hw, int k) {
    const int lane = threadIdx.x & 63;
    bool pending = true;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (pending) {
            const int first = __builtin_amdgcn_readfirstlane(k);
            const unsigned long long same = __ballot(k == first);
            if (k == first) {
                if (lane == __ffsll((long long)same) - 1) atomicAdd(&hw[k], (uint32_t)__popcll(same));
                pending = false;
            }
        }
    }
    if (pending) atomicAdd(&hw[k], 1u);
}

__global__ __launch_bounds__(256) void k_aq_hist(const float* __restrict__ x, int64_t rows, uint64_t n, int64_t ld,
                                                  const uint32_t* __restrict__ obs, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[4][kAqBins];
    const float lo32 = ord2f(obs[0]), hi32 = ord2f(obs[1]);
    if (!aq_finite(lo32) || !aq_finite(hi32)) return;          // a void row (the same answer in every thread of the grid)
    for (int i = threadIdx.x; i < 4 * kAqBins; i += 256) (&h[0][0])[i] = 0u;
    double lo = (double)lo32, hi = (double)hi32;
    if (lo == hi) {
        lo -= 0.5;
        hi += 0.5;
    }
    const double span = hi - lo, step = span / (double)kAqBins;
    __syncthreads();
    uint32_t* hw = h[threadIdx.x >> 6];
    const uint64_t vstep = (uint64_t)gridDim.x * 256;
    for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {      // n values per row, rows ld apart
        const float* xr = x + row * ld;
        uint64_t head = ((16u - (unsigned)(reinterpret_cast<uintptr_t>(xr) & 15u)) & 15u) / 4u;      // elements in front of the first 16-B boundary
        if (head > n) head = n;
        const uint64_t nvec = (n - head) / 4, tail0 = head + nvec * 4;
        const float4* xv = reinterpret_cast<const float4*>(xr + head);
        for (uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x; v < nvec; v += vstep) {
            const float4 q = xv[v];
            aq_hist_add(hw, aq_bin((double)q.x, lo, span, step));
            aq_hist_add(hw, aq_bin((double)q.y, lo, span, step));
            aq_hist_add(hw, aq_bin((double)q.z, lo, span, step));
            aq_hist_add(hw, aq_bin((double)q.w, lo, span, step));
        }
        if (blockIdx.x == 0) {
            if (threadIdx.x < head) aq_hist_add(hw, aq_bin((double)xr[threadIdx.x], lo, span, step));
            if (tail0 + threadIdx.x < n) aq_hist_add(hw, aq_bin((double)xr[tail0 + threadIdx.x], lo, span, step));      // at most 3
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kAqBins; b += 256) {
        const uint32_t s = h[0][b] + h[1][b] + h[2][b] + h[3][b];
        if (s != 0u) atomicAdd(&hist[b], s);
    }
}

__global__ void k_aq_hist_fin(uint32_t* obs, float* rng) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const float lo = ord2f(obs[0]), hi = ord2f(obs[1]);
        const bool ok = aq_finite(lo) && aq_finite(hi);
        rng[0] = ok ? lo : __uint_as_float(0x7fc00000u);
        rng[1] = ok ? hi : __uint_as_float(0x7fc00000u);
        obs[0] = 0xFFFFFFFFu;
        obs[1] = 0u;
    }
}

__global__ __launch_bounds__(64) void k_aq_prep(const uint32_t* __restrict__ hist, const float* __restrict__ rng, int T, double* __restrict__ ws) {
    __shared__ double slo[kAqRows], shi[kAqRows];
    const AqLayout L = aq_layout(T);
    const int t = threadIdx.x;
    double lo = __longlong_as_double(0x7ff8000000000000LL), hi = lo;
    if (t < T) {
        const float l32 = rng[2 * t], h32 = rng[2 * t + 1];
        if (aq_finite(l32) && aq_finite(h32)) {
            lo = (double)l32;
            hi = (double)h32;
            if (lo == hi) {
                lo -= 0.5;
                hi += 0.5;
            }
        }
        double* c = ws + L.cum + (int64_t)t * (kAqBins + 1);
        uint64_t s = 0;
        c[0] = 0.0;
        for (int k = 0; k < kAqBins; ++k) {
            s += hist[(int64_t)t * kAqBins + k];
            c[k + 1] = (double)s;                     // exact: below 2^53
        }
    }
    slo[t] = lo;
    shi[t] = hi;
    ws[L.rows + 2 * t] = lo;
    ws[L.rows + 2 * t + 1] = hi;
    __syncthreads();
    if (t == 0) {
        double bmin = INFINITY, bmax = -INFINITY, w = INFINITY;
        int nv = 0;
        for (int r = 0; r < T; ++r) {
            if (slo[r] != slo[r]) continue;
            nv += 1;
            bmin = fmin(bmin, slo[r]);
            bmax = fmax(bmax, shi[r]);
            w = fmin(w, (shi[r] - slo[r]) / (double)kAqBins);
        }
        double M = ceil(((bmax + w) - bmin) / w);
        if (!(M <= (double)kAqMaxM)) {                // too many points (or w == 0: not finite)
            w = (bmax - bmin) / (double)(kAqMaxM - 1);
            M = fmin(ceil(((bmax + w) - bmin) / w), (double)kAqMaxM);
        }
        if (!(M >= 2.0)) M = 2.0;
        ws[L.hdr + 0] = bmin;
        ws[L.hdr + 1] = bmax;
        ws[L.hdr + 2] = w;
        ws[L.hdr + 3] = nv > 0 ? M : 2.0;
        ws[L.hdr + 4] = (double)nv;
    }
}

// np.interp(b, E_t, c_t): E_t the 513 edges over (lo, hi), c_t the cumulative counts
__device__ __forceinline__ double aq_cum_at(double b, double lo, double hi, const double* __restrict__ c) {
    if (b < lo) return 0.0;
    if (b >= hi) return c[kAqBins];
    const double span = hi - lo, step = span / (double)kAqBins;
    const double f = (b - lo) / span * (double)kAqBins;
    int k = f >= (double)kAqBins ? kAqBins - 1 : (f > 0.0 ? (int)f : 0);
    for (int r = 0; r < 4 && k > 0 && b < lo + (double)k * step; ++r) k -= 1;
    for (int r = 0; r < 4 && k < kAqBins - 1 && b >= lo + (double)(k + 1) * step; ++r) k += 1;
    const double e0 = lo + (double)k * step, e1 = k == kAqBins - 1 ? hi : lo + (double)(k + 1) * step;
    const double slope = (c[k + 1] - c[k]) / (e1 - e0);
    return slope * (b - e0) + c[k];
}

__global__ __launch_bounds__(256) void k_aq_merge(double* __restrict__ ws, int T) {
    const AqLayout L = aq_layout(T);
    const int M = (int)ws[L.hdr + 3];
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M || m >= kAqMaxM) return;
    const double bmin = ws[L.hdr + 0], w = ws[L.hdr + 2];
    const double b0 = bmin + (double)m * w;
    ws[L.b + m] = b0;
    if (m >= M - 1) return;
    const double b1 = bmin + (double)(m + 1) * w;
    double acc = 0.0;
    for (int t = 0; t < T; ++t) {
        const double lo = ws[L.rows + 2 * t], hi = ws[L.rows + 2 * t + 1];
        if (lo != lo) continue;
        const double* c = ws + L.cum + (int64_t)t * (kAqBins + 1);
        acc += aq_cum_at(b1, lo, hi, c) - aq_cum_at(b0, lo, hi, c);
    }
    ws[L.vals + m] = acc;
}

__global__ __launch_bounds__(256) void k_aq_search(double* __restrict__ ws, int T) {
    __shared__ double sb[kAqTile], sv[kAqTile];
    const AqLayout L = aq_layout(T);
    const int K = (int)ws[L.hdr + 3] - 1;                      // left edges: 1 <= K <= 65535
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x / (kAqN / kAqJPerWg), j = (blockIdx.x % (kAqN / kAqJPerWg)) * kAqJPerWg + wave;
    const double* b = ws + L.b;
    const double* vals = ws + L.vals;
    const double b0 = b[0], bl = b[K - 1];
    const double delta = 0.5 * (bl - b0) / (double)kAqN;
    const double mn = b0 + delta * (double)i, mx = bl - delta * (double)j;
    const double D = (mx - mn) / 255.0;
    double acc = 0.0, sum = 0.0;
    for (int base = 0; base < K; base += kAqTile) {
        const int cnt = K - base < kAqTile ? K - base : kAqTile;
        for (int e = threadIdx.x; e < cnt; e += 256) {
            sb[e] = b[base + e];
            sv[e] = vals[base + e];
        }
        __syncthreads();
        for (int e = lane; e < cnt; e += 64) {
            const double be = sb[e], ve = sv[e];
            const double c = fmin(fmax(rint((be - mn) / D), 0.0), 255.0);
            const double d = be - (D * c + mn);
            acc += (d * d) * ve;
            sum += ve;
        }
        __syncthreads();
    }
    acc = wave_sum63(acc);
    sum = wave_sum63(sum);
    if (lane == 63) ws[L.err + i * kAqN + j] = acc / sum;
}

__global__ __launch_bounds__(256) void k_aq_argmin(const double* __restrict__ ws, int T, float* qmin, float* qmax, int* ij_out, double* err_out) {
    __shared__ double se[256];
    __shared__ int si[256];
    const AqLayout L = aq_layout(T);
    double best = INFINITY;
    int idx = 0;
    for (int k = threadIdx.x; k < kAqN * kAqN; k += 256) {     // increasing k: a tie keeps the smaller index
        const double e = ws[L.err + k];
        if (e < best) {
            best = e;
            idx = k;
        }
    }
    se[threadIdx.x] = best;
    si[threadIdx.x] = idx;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (ws[L.hdr + 4] == 0.0) {                            // every row void: the ranges stay
            if (ij_out) ij_out[0] = ij_out[1] = -1;
            if (err_out) *err_out = __longlong_as_double(0x7ff8000000000000LL);
            return;
        }
        best = INFINITY;
        idx = 0;
        for (int t = 0; t < 256; ++t) {
            if (se[t] < best || (se[t] == best && best < INFINITY && si[t] < idx)) {
                best = se[t];
                idx = si[t];
            }
        }
        const int K = (int)ws[L.hdr + 3] - 1, i = idx / kAqN, j = idx % kAqN;
        const double b0 = ws[L.b], bl = ws[L.b + K - 1];
        const double delta = 0.5 * (bl - b0) / (double)kAqN;
        *qmin = (float)(b0 + delta * (double)i);
        *qmax = (float)(bl - delta * (double)j);
        if (ij_out) {
            ij_out[0] = i;
            ij_out[1] = j;
        }
        if (err_out) *err_out = best;
    }
}

}  // namespace fqss

using namespace fqss;

extern "C" int64_t fqss_aq_mse_ws_bytes(int T) {
    if (T < 1 || T > kAqRows) return 0;
    return aq_layout(T).total * (int64_t)sizeof(double);
}

extern "C" int64_t fqss_aq_mse_ws_offset(int T, int what) {
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

static int aq_hist_launch(const char* who, const float* x, int64_t rows, int64_t cols, int64_t ld, uint32_t* obs_ws, uint32_t* hist_row,
                          float* rng_row, fqss_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    int64_t gx = cdiv(cols, 256 * 4 * 8);         // about eight 16-B loads per thread and row
    if (gx > 2048) gx = 2048;
    int64_t gy = 2048 / gx;                       // the rows share out what the columns leave of ~2048 workgroups
    if (gy > rows) gy = rows;
    if (gy < 1) gy = 1;
    hipLaunchKernelGGL(k_aq_hist, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, x, rows, (uint64_t)cols, ld, (const uint32_t*)obs_ws,
                       hist_row);
    hipLaunchKernelGGL(k_aq_hist_fin, dim3(1), dim3(64), 0, st, obs_ws, rng_row);
    return launch_status(who);
}

extern "C" int fqss_aq_hist(const float* x, int64_t n, uint32_t* obs_ws, uint32_t* hist_row, float* rng_row, fqss_stream_t stream) {
    FQSS_REQUIRE(x && obs_ws && hist_row && rng_row, "null pointer");
    FQSS_REQUIRE(n >= 1 && n < ((int64_t)1 << 32), "n outside 1 .. 2^32 - 1");
    FQSS_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3u) == 0, "x not 4-B aligned");
    return aq_hist_launch("fqss_aq_hist", x, 1, n, n, obs_ws, hist_row, rng_row, stream);
}

extern "C" int fqss_aq_hist_rows(const float* x, int64_t rows, int64_t cols, int64_t ld, uint32_t* obs_ws, uint32_t* hist_row, float* rng_row,
                                 fqss_stream_t stream) {
    FQSS_REQUIRE(x && obs_ws && hist_row && rng_row, "null pointer");
    FQSS_REQUIRE(rows >= 1 && cols >= 1 && ld >= cols && rows < ((int64_t)1 << 32) && cols < ((int64_t)1 << 32) &&
                     rows * cols < ((int64_t)1 << 32),
                 "bad shape (rows, cols >= 1, ld >= cols, rows * cols < 2^32)");
    FQSS_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3u) == 0, "x not 4-B aligned");
    return aq_hist_launch("fqss_aq_hist_rows", x, rows, cols, ld, obs_ws, hist_row, rng_row, stream);
}

extern "C" int fqss_aq_mse_search(const uint32_t* hist, const float* rng, int T, int n_bits, double* ws, float* qmin, float* qmax, int* ij_out,
                                  double* err_out, fqss_stream_t stream) {
    FQSS_REQUIRE(hist && rng && ws && qmin && qmax, "null pointer");
    FQSS_REQUIRE(T >= 1 && T <= kAqRows, "T outside 1 .. 64");
    FQSS_REQUIRE(n_bits == 8, "n_bits must be 8 (the activation grid of the fused kernels)");
    FQSS_REQUIRE(aligned16(ws), "workspace not 16-B aligned");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_aq_prep, dim3(1), dim3(64), 0, st, hist, rng, T, ws);
    hipLaunchKernelGGL(k_aq_merge, dim3(kAqMaxM / 256), dim3(256), 0, st, ws, T);
    hipLaunchKernelGGL(k_aq_search, dim3(kAqN * (kAqN / kAqJPerWg)), dim3(256), 0, st, ws, T);
    hipLaunchKernelGGL(k_aq_argmin, dim3(1), dim3(256), 0, st, (const double*)ws, T, qmin, qmax, ij_out, err_out);
    return launch_status("fqss_aq_mse_search");
}
