// stoi.hip -- short-time objective intelligibility of the evaluation side (process.metric_evaluation, process.py:129-152 of the
// reference: torchmetrics' ShortTimeObjectiveIntelligibility = pystoi.stoi(clean, estimate, fs, extended=False) -- third party and absent,
// restated; the six steps and what is pinned are in include/fqss.h at fqss_stoi).  Everything in fp64, no floating-point atomics, every
// sum in a fixed order (the DPP tree of wave_sum63, wave sums added in wave order) -- the same bits every run.  Nothing is read back: the
// kept-frame count K lives in the workspace, the kernels behind it are launched over its upper bound and leave early.
//   k_stoi_resample  grid (256-sample output tiles, 2 P signals): the tile's input span and the taps in LDS, one output per thread
//                    walking its polyphase branch (n_taps / up products); not launched at 10 kHz
//   k_stoi_energy    one wave per frame of the clean signal: 256 windowed squares, the DPP sum, e in dB
//   k_stoi_mask      one workgroup per pair: max(e), the mask, a ballot scan into the list of kept frames, K
//   k_stoi_spec      one workgroup per spectral frame and signal: its 256 silence-removed samples gathered through the list (at most two
//                    kept frames each), the second window, a 512-point radix-2 Stockham FFT in LDS, 15 band sums
//   k_stoi_corr      grid (segments, pairs): 15 bands x 30 columns, one band per wave at a time, the columns on the lanes
//   k_stoi_finish    one workgroup per pair: the segment partials summed, the division, 1e-5 when fewer than 30 frames are left
#include "fqss_dev.h"

namespace fqss {

constexpr int kStoiFrame = 256, kStoiHop = 128, kStoiFft = 512, kStoiBands = 15, kStoiSeg = 30;
constexpr int kStoiTile = 256;           // outputs per workgroup of k_stoi_resample
constexpr int kStoiMaxTaps = 1023;       // the taps and ...
constexpr int kStoiSpan = 1024;          // ... the input span of a tile, as fp64 in LDS (16 KB together)
constexpr double kStoiEps = 2.220446049250313e-16;        // 2^-52
__constant__ int kStoiLo[kStoiBands + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

// where the workspace keeps what (doubles from its start; the same on the host and on the device)
struct StoiLayout {
    int64_t Lp, NF, Tmax, Smax;          // samples at 10 kHz, frames of them, upper bounds of the spectral frames and of the segments
    int64_t sig, e, idx, tob, part, total;
};
__host__ __device__ static inline StoiLayout stoi_layout(int P, int64_t L, int up, int down) {
    StoiLayout w;
    w.Lp = (L * up + down - 1) / down;
    w.NF = w.Lp > kStoiFrame ? (w.Lp - kStoiFrame + kStoiHop - 1) / kStoiHop : 0;      // starts 128 f < Lp - 256
    w.Tmax = w.NF > 1 ? w.NF - 1 : 0;
    w.Smax = w.NF > kStoiSeg ? w.NF - kStoiSeg : 0;
    w.sig = 0;                                                     // [2][P][Lp] resampled signals (clean first); absent at 10 kHz
    w.e = w.sig + (up == down ? 0 : 2 * (int64_t)P * w.Lp);        // [P][NF] frame energies in dB
    w.idx = w.e + (int64_t)P * w.NF;                               // [P] x (NF + 1 int32: the kept frames, then K at [NF])
    w.tob = w.idx + (int64_t)P * ((w.NF + 2) / 2);                 // [P][2][15][Tmax] band amplitudes (clean first)
    w.part = w.tob + (int64_t)P * 2 * kStoiBands * w.Tmax;         // [P][Smax] one partial per segment
    w.total = w.part + (int64_t)P * w.Smax;
    return w;
}

// One signal at 10 kHz: the resampled copy in the workspace, or the fp32 input itself (wave-uniform choice).
struct StoiSig {
    const double* d;
    const float* f;
    __device__ __forceinline__ double operator[](int64_t i) const { return d ? d[i] : (double)f[i]; }
};
__device__ __forceinline__ StoiSig stoi_sig(const float* est, const float* ref, const double* ws, const StoiLayout& w, int resampled, int s,
                                            int64_t p, int P, int64_t ld_e, int64_t ld_r) {
    StoiSig g;
    g.d = resampled ? ws + w.sig + ((int64_t)s * P + p) * w.Lp : nullptr;
    g.f = s == 0 ? ref + p * ld_r : est + p * ld_e;
    return g;
}
__device__ __forceinline__ double stoi_window(int t) { return 0.5 - 0.5 * cospi(2.0 * (double)(t + 1) / 257.0); }
__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// out[n] = sum_k taps[k] u[n down + Lh - k], u the input zero-stuffed by `up`: with m = n down + Lh only k = m mod up, + up, ... meet a
// sample, x[(m - k) / up].  Lanes of a wave read nearly consecutive doubles of the span (down / up apart) and at most `up` distinct
// taps per step (equal addresses broadcast).
__global__ __launch_bounds__(256) void k_stoi_resample(const float* __restrict__ est, const float* __restrict__ ref, const double* __restrict__ taps,
                                                       int n_taps, double* __restrict__ ws, int P, int64_t L, int64_t ld_e, int64_t ld_r, int up,
                                                       int down) {
    __shared__ double span[kStoiSpan];
    __shared__ double tap[kStoiMaxTaps + 1];
    const StoiLayout w = stoi_layout(P, L, up, down);
    const int tid = threadIdx.x, s = blockIdx.y / P;
    const int64_t p = blockIdx.y % P, n0 = (int64_t)blockIdx.x * kStoiTile, Lh = (n_taps - 1) / 2;
    const float* x = s == 0 ? ref + p * ld_r : est + p * ld_e;
    const int64_t base = floor_div(n0 * down + Lh - (n_taps - 1), up);      // <= the lowest sample any output of the tile reads
    for (int i = tid; i < kStoiSpan; i += 256) {
        const int64_t g = base + i;
        span[i] = (g >= 0 && g < L) ? (double)x[g] : 0.0;
    }
    for (int i = tid; i < n_taps; i += 256) tap[i] = taps[i];
    __syncthreads();
    const int64_t n = n0 + tid;
    if (n >= w.Lp) return;
    const int64_t m = n * down + Lh;
    const int k0 = (int)(m % up);
    const int top = (int)((m - k0) / up - base);      // span index of tap k0's sample; < kStoiSpan by the host's check of the ratio
    double acc = 0.0;
    for (int k = k0, i = top; k < n_taps; k += up, --i) acc += tap[k] * span[i];      // i >= 0: base is below every sample read
    ws[w.sig + ((int64_t)s * P + p) * w.Lp + n] = acc;
}

__global__ __launch_bounds__(256) void k_stoi_energy(const float* __restrict__ est, const float* __restrict__ ref, double* __restrict__ ws, int P,
                                                     int64_t L, int64_t ld_e, int64_t ld_r, int up, int down, int resampled) {
    const StoiLayout w = stoi_layout(P, L, up, down);
    const int lane = threadIdx.x & 63;
    const int64_t p = blockIdx.y, f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= w.NF) return;      // a whole wave
    const StoiSig x = stoi_sig(est, ref, ws, w, resampled, 0, p, P, ld_e, ld_r);
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < kStoiFrame / 64; ++i) {
        const int t = lane + 64 * i;
        const double v = stoi_window(t) * x[f * kStoiHop + t];      // f 128 + 255 < Lp: the strict frame rule
        ss += v * v;
    }
    ss = wave_sum63(ss);
    if (lane == 63) ws[w.e + p * w.NF + f] = 20.0 * log10(sqrt(ss) + kStoiEps);
}

__global__ __launch_bounds__(256) void k_stoi_mask(double* __restrict__ ws, int P, int64_t L, int up, int down) {
    __shared__ double smax[256];
    __shared__ int wcount[4];
    const StoiLayout w = stoi_layout(P, L, up, down);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t p = blockIdx.x;
    const double* e = ws + w.e + p * w.NF;
    int* idx = reinterpret_cast<int*>(ws + w.idx + p * ((w.NF + 2) / 2));
    double mx = -INFINITY;
    for (int64_t f = tid; f < w.NF; f += 256) mx = fmax(mx, e[f]);
    smax[tid] = mx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) smax[tid] = fmax(smax[tid], smax[tid + h]);
        __syncthreads();
    }
    mx = smax[0];
    int kept = 0;      // frames kept before this round of 256
    for (int64_t f0 = 0; f0 < w.NF; f0 += 256) {
        const int64_t f = f0 + tid;
        const bool keep = f < w.NF && (mx - 40.0 - e[f]) < 0.0;
        const unsigned long long b = __ballot(keep);
        if (lane == 0) wcount[wv] = __popcll(b);
        __syncthreads();
        int before = kept + __popcll(b & ((1ull << lane) - 1ull));
        for (int i = 0; i < wv; ++i) before += wcount[i];
        if (keep) idx[before] = (int)f;
        kept += wcount[0] + wcount[1] + wcount[2] + wcount[3];
        __syncthreads();
    }
    if (tid == 0) idx[w.NF] = kept;
}

// Spectral frame m of the silence-removed signal: sample t is w[t] x[kept[m]][t], plus the second half of kept frame m - 1 (t < 128, m > 0)
// or the first half of kept frame m + 1 (t >= 128; m + 1 <= K - 1 exists) -- a sum of two terms, the same in either order.
// FFT: re / im planes of 512 doubles, two of each (16 KB); butterfly j reads elements j and j + 256 (consecutive doubles across the
// lanes: every bank once per half wave) and writes (j / Ns) 2 Ns + j % Ns and Ns further.  The first stage of a frame whose upper
// half is zero padding is a copy (out[2 j] = out[2 j + 1] = in[j]): done by the load.  Twiddles exp(-2 pi i k / 512), k < 256, once per
// workgroup by sincospi.
__global__ __launch_bounds__(256) void k_stoi_spec(const float* __restrict__ est, const float* __restrict__ ref, double* __restrict__ ws, int P,
                                                   int64_t L, int64_t ld_e, int64_t ld_r, int up, int down, int resampled) {
    __shared__ double re[2][kStoiFft], im[2][kStoiFft], twc[kStoiFft / 2], tws[kStoiFft / 2];
    const StoiLayout w = stoi_layout(P, L, up, down);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, s = blockIdx.y / P;
    const int64_t p = blockIdx.y % P, m = blockIdx.x;
    const int* idx = reinterpret_cast<const int*>(ws + w.idx + p * ((w.NF + 2) / 2));
    const int K = idx[w.NF];
    if (m >= K - 1) return;
    const StoiSig x = stoi_sig(est, ref, ws, w, resampled, s, p, P, ld_e, ld_r);
    const double wt = stoi_window(tid);
    double v = wt * x[(int64_t)idx[m] * kStoiHop + tid];
    if (tid < kStoiHop) {
        if (m > 0) v = stoi_window(tid + kStoiHop) * x[(int64_t)idx[m - 1] * kStoiHop + tid + kStoiHop] + v;
    } else {
        v = v + stoi_window(tid - kStoiHop) * x[(int64_t)idx[m + 1] * kStoiHop + tid - kStoiHop];
    }
    v = wt * v;
    re[0][2 * tid] = v;
    re[0][2 * tid + 1] = v;
    im[0][2 * tid] = 0.0;
    im[0][2 * tid + 1] = 0.0;
    double sn, cs;
    sincospi(-(double)tid / 256.0, &sn, &cs);
    twc[tid] = cs;
    tws[tid] = sn;
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int Ns = 2; Ns < kStoiFft; Ns *= 2) {
        const int k = tid & (Ns - 1), tw = k * (kStoiFft / 2 / Ns), o = ((tid - k) << 1) + k;
        const double ar = re[cur][tid], ai = im[cur][tid], br = re[cur][tid + 256], bi = im[cur][tid + 256];
        const double c = twc[tw], sgn = tws[tw];
        const double tr = br * c - bi * sgn, ti = br * sgn + bi * c;
        re[cur ^ 1][o] = ar + tr;
        im[cur ^ 1][o] = ai + ti;
        re[cur ^ 1][o + Ns] = ar - tr;
        im[cur ^ 1][o + Ns] = ai - ti;
        cur ^= 1;
        __syncthreads();
    }
    // band k on wave k % 4: one bin per lane (the widest band has 45), the DPP sum, lane 63 stores
    double* out = ws + w.tob + ((p * 2 + s) * kStoiBands) * w.Tmax + m;
    for (int k = wv; k < kStoiBands; k += 4) {
        const int b = kStoiLo[k] + lane;
        double pw = 0.0;
        if (b < kStoiLo[k + 1]) pw = re[cur][b] * re[cur][b] + im[cur][b] * im[cur][b];
        pw = wave_sum63(pw);
        if (lane == 63) out[k * w.Tmax] = sqrt(pw);
    }
}

// Segment sg = columns sg .. sg + 29.  Lane c < 30 holds column c of the band its wave works on; the other lanes hold zeros, which
// every sum and the min() leave alone.
__global__ __launch_bounds__(256) void k_stoi_corr(double* __restrict__ ws, int P, int64_t L, int up, int down) {
    __shared__ double red[4];
    const StoiLayout w = stoi_layout(P, L, up, down);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t p = blockIdx.y, sg = blockIdx.x;
    const int K = reinterpret_cast<const int*>(ws + w.idx + p * ((w.NF + 2) / 2))[w.NF];
    if (sg + kStoiSeg > K - 1) return;
    const double clip = 1.0 + 5.623413251903491;      // 1 + 10^(15/20)
    const bool col = lane < kStoiSeg;
    double acc = 0.0;
    for (int k = wv; k < kStoiBands; k += 4) {
        const double* xt = ws + w.tob + ((p * 2 + 0) * kStoiBands + k) * w.Tmax + sg;
        const double* yt = ws + w.tob + ((p * 2 + 1) * kStoiBands + k) * w.Tmax + sg;
        const double x = col ? xt[lane] : 0.0, y = col ? yt[lane] : 0.0;
        const double xn = sqrt(wave_sum(x * x)), yn = sqrt(wave_sum(y * y));
        const double yp = fmin(y * (xn / (yn + kStoiEps)), x * clip);
        const double mx = wave_sum(x) / (double)kStoiSeg, my = wave_sum(yp) / (double)kStoiSeg;
        const double xc = col ? x - mx : 0.0, yc = col ? yp - my : 0.0;
        const double nx = sqrt(wave_sum(xc * xc)) + kStoiEps, ny = sqrt(wave_sum(yc * yc)) + kStoiEps;
        acc += wave_sum63((xc / nx) * (yc / ny));
    }
    if (lane == 63) red[wv] = acc;
    __syncthreads();
    if (tid == 0) ws[w.part + p * w.Smax + sg] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void k_stoi_finish(const double* __restrict__ ws, double* __restrict__ d, int P, int64_t L, int up, int down) {
    __shared__ double smem[4];
    const StoiLayout w = stoi_layout(P, L, up, down);
    const int64_t p = blockIdx.x;
    const int K = reinterpret_cast<const int*>(ws + w.idx + p * ((w.NF + 2) / 2))[w.NF];
    const int64_t nseg = (int64_t)K - 1 - (kStoiSeg - 1);      // T - 29
    double s[1] = {0.0};
    for (int64_t i = threadIdx.x; i < nseg; i += 256) s[0] += ws[w.part + p * w.Smax + i];
    block_sum<double, 1>(s, smem);
    if (threadIdx.x == 0) d[p] = nseg >= 1 ? s[0] / ((double)kStoiBands * (double)nseg) : 1e-5;
}

static int64_t gcd64(int64_t a, int64_t b) { return b == 0 ? a : gcd64(b, a % b); }
static bool stoi_ratio_ok(int up, int down) { return up >= 1 && down >= 1 && up <= 65536 && down <= 65536 && gcd64(up, down) == 1; }
constexpr int64_t kStoiMaxUpL = (int64_t)1 << 37;      // L up: frame numbers and grids stay below 2^31
static bool stoi_shape_ok(int P, int64_t L, int up, int down) {
    return P >= 1 && P <= 32767 && L >= 1 && stoi_ratio_ok(up, down) && L <= kStoiMaxUpL / up;
}

}  // namespace fqss

using namespace fqss;

// doubles of workspace of fqss_stoi (stoi_layout above); 0 for arguments fqss_stoi refuses
extern "C" int64_t fqss_stoi_ws_doubles(int P, int64_t L, int up, int down) {
    if (!stoi_shape_ok(P, L, up, down)) return 0;
    return stoi_layout(P, L, up, down).total;
}

extern "C" int fqss_stoi(const float* est, const float* ref, const double* taps, int n_taps, double* ws, int64_t ws_doubles, double* d, int P,
                         int64_t L, int64_t ld_e, int64_t ld_r, int up, int down, fqss_stream_t stream) {
    FQSS_REQUIRE(est && ref && taps && ws && d, "null pointer");
    FQSS_REQUIRE(stoi_ratio_ok(up, down), "up / down not in 1..65536 or not reduced");
    FQSS_REQUIRE(stoi_shape_ok(P, L, up, down) && ld_e >= L && ld_r >= L, "bad shape (1 <= P <= 32767, 1 <= L <= 2^37 / up, ld >= L)");
    FQSS_REQUIRE(n_taps >= 1 && (n_taps & 1) && (up != down || n_taps == 1), "n_taps even, or not 1 at up = down = 1");
    // a tile of 256 outputs reads at most (255 down + n_taps - 1) / up + 2 consecutive input samples
    FQSS_REQUIRE(n_taps <= kStoiMaxTaps && 255 * (int64_t)down + n_taps <= (kStoiSpan - 2) * (int64_t)up,
                 "resampler outside what one workgroup stages");
    const StoiLayout w = stoi_layout(P, L, up, down);
    FQSS_REQUIRE(ws_doubles >= w.total, "workspace shorter than fqss_stoi_ws_doubles");
    hipStream_t st = (hipStream_t)stream;
    const int resampled = up != down;
    if (resampled)
        hipLaunchKernelGGL(k_stoi_resample, dim3((unsigned)cdiv(w.Lp, kStoiTile), 2u * P), dim3(256), 0, st, est, ref, taps, n_taps, ws, P, L, ld_e,
                           ld_r, up, down);
    if (w.NF > 0) hipLaunchKernelGGL(k_stoi_energy, dim3((unsigned)cdiv(w.NF, 4), (unsigned)P), dim3(256), 0, st, est, ref, ws, P, L, ld_e, ld_r, up, down, resampled);
    hipLaunchKernelGGL(k_stoi_mask, dim3((unsigned)P), dim3(256), 0, st, ws, P, L, up, down);
    if (w.Tmax > 0)
        hipLaunchKernelGGL(k_stoi_spec, dim3((unsigned)w.Tmax, 2u * P), dim3(256), 0, st, est, ref, ws, P, L, ld_e, ld_r, up, down, resampled);
    if (w.Smax > 0) hipLaunchKernelGGL(k_stoi_corr, dim3((unsigned)w.Smax, (unsigned)P), dim3(256), 0, st, ws, P, L, up, down);
    hipLaunchKernelGGL(k_stoi_finish, dim3((unsigned)P), dim3(256), 0, st, (const double*)ws, d, P, L, up, down);
    return launch_status("fqss_stoi");
}
