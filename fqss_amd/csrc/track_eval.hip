// track_eval.hip -- whole-track evaluation of the HTDemucs recipe on the device (val.py:95-131 of the reference, `val_musdbhq_NSDR`;
// calc_nsdr of its process.py:70-75): the statistics the track is normalised by, the multi-channel chunk batches, the per-item
// normalize=False splitter of a batch, and the nSDR (the overlap-add with the de-normalisation in its store: fqss_infer_ola_chunks,
// infer.hip).  Statements: include/fqss.h.
//
// How the sums are formed (fqss_track_stats, fqss_nsdr): a tile is FQSS_TRACK_TILE = 4096 samples = 256 lanes x 4 visits x 4 consecutive
// samples.  A lane adds its 16 samples in fp64 in (visit, sample) order, the workgroup adds its lanes on the fixed DPP tree
// (block_sum), and the tile's partial goes to the workspace; one workgroup then adds the partials in tile order on the same tree.  The
// order is a function of the shape alone -- the 16-byte and the one-sample load forms visit the same samples in the same order -- so a
// result does not depend on alignment, grid or run.  No floating-point atomics anywhere.
//
// fqss_frame_sdr (the window-wise SDR of museval's default branch and its median over the track) keeps the same discipline with a window,
// not a tile, as the unit: one workgroup per (window, source) adds all channels of its window, one workgroup per source sorts the
// windows' values in LDS and takes the middle.
#include "eval_dev.h"

namespace fqss {

constexpr int kTile = FQSS_TRACK_TILE;
static_assert(kTile == 256 * 4 * 4, "a tile is 256 lanes x 4 visits x 4 samples");

// sum of p[0 .. n) in every thread of a 256-thread workgroup: lane i adds p[i], p[i + 256], .. in index order, then the DPP tree and the
// four waves in wave order.  smem: 5 doubles
__device__ __forceinline__ double tile_order_sum(const double* p, int64_t n, double* smem) {
    double v[1] = {0.0};
    for (int64_t i = threadIdx.x; i < n; i += 256) v[0] += p[i];
    block_sum<double, 1>(v, smem);
    if (threadIdx.x == 0) smem[4] = v[0];
    __syncthreads();
    const double s = smem[4];
    __syncthreads();
    return s;
}

// ---- fqss_track_stats ----
// PASS 1: ws[tile] = sum of m_t over the tile; PASS 2: ws[ntiles + tile] = sum of (m_t - mean)^2 with mean = (sum of ws[0 .. ntiles)) / L
// taken by every workgroup for itself (ntiles doubles from L2: no launch of its own for one division)
template <bool VEC, int PASS>
__global__ __launch_bounds__(256) void k_track_stats_tiles(const float* __restrict__ x, double* ws, int C, int64_t L, int64_t ld,
                                                            int64_t ntiles) {
    __shared__ double smem[5];
    double mean = 0.0;
    if (PASS == 2) mean = tile_order_sum(ws, ntiles, smem) / (double)L;
    const float fc = (float)C;
    double acc[1] = {0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t i = (int64_t)blockIdx.x * kTile + (int64_t)(j * 256 + (int)threadIdx.x) * 4;
        if (i >= L) break;
        float m[4], v[4];
        load_quad<VEC>(x, i, L, m);
        for (int c = 1; c < C; ++c) {
            load_quad<VEC>(x + c * ld, i, L, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] += v[e];           // fp32, channel order
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double mt = (double)(m[e] / fc);              // IEEE fp32 division
            const double d = mt - mean;
            if (i + e < L) acc[0] += PASS == 1 ? mt : d * d;
        }
    }
    block_sum<double, 1>(acc, smem);
    if (threadIdx.x == 0) ws[(PASS - 1) * ntiles + blockIdx.x] = acc[0];
}

__global__ __launch_bounds__(256) void k_track_stats_finish(const double* ws, int64_t ntiles, int64_t L, float* __restrict__ stats) {
    __shared__ double smem[5];
    const double mean = tile_order_sum(ws, ntiles, smem) / (double)L;
    const double var = tile_order_sum(ws + ntiles, ntiles, smem) / (double)(L - 1);      // L = 1: 0 / 0, NaN as torch
    if (threadIdx.x == 0) {
        stats[0] = (float)mean;
        stats[1] = (float)sqrt(var);
    }
}

// ---- fqss_chunk_gather_mc ----
// out[g][c][t] = norm(mix[c][k * stride + t]), k = min(k0 + g, N - 1); 0 past L.  blockIdx.y = g * C + c; a lane moves quads
template <bool VEC>
__global__ __launch_bounds__(256) void k_chunk_gather_mc(const float* __restrict__ mix, const float* __restrict__ stats, float* __restrict__ out,
                                                          int C, int64_t L, int64_t ld, int64_t seg, int64_t stride, int64_t k0, int64_t N) {
    const int g = blockIdx.y / C, c = blockIdx.y % C;
    int64_t k = k0 + g;
    if (k > N - 1) k = N - 1;
    const float* src = mix + c * ld + k * stride;
    const int64_t rest = L - k * stride, n = rest < seg ? rest : seg;       // in-range samples of the chunk, >= 1
    float* dst = out + (int64_t)blockIdx.y * seg;
    const bool norm = stats != nullptr;
    const float mean = norm ? stats[0] : 0.0f, sd = norm ? stats[1] : 1.0f;
    for (int64_t t = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; t < seg; t += (int64_t)gridDim.x * 1024) {
        float v[4];
        load_quad<VEC>(src, t, n, v);
        if (norm) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = t + e < n ? (v[e] - mean) / sd : 0.0f;       // fp32 subtraction, IEEE fp32 division
        }
        if (VEC) {      // seg % 4 == 0: the quad is whole
            *reinterpret_cast<float4*>(dst + t) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (t + e < seg) dst[t + e] = v[e];
        }
    }
}

// ---- fqss_splitter2_raw_rows ----
// stage 1: max|x[b][:]| into row_max[b] as the bit image of a non-negative float, which orders like the unsigned integer it is
// (atomicMax: exact and order-free; zeroed by the caller) -- the idiom of fqss_splitter2_rows.  stage 2: split2_raw under thr_b.
__global__ __launch_bounds__(256) void k_rows_absmax(const float* __restrict__ x, int B, int64_t N, uint32_t* __restrict__ row_max) {
    __shared__ float wmx[4];
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        float vmax = 0.0f;
        for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < N; t += (int64_t)gridDim.x * 256) vmax = fmaxf(vmax, fabsf(x[b * N + t]));
        vmax = wave_max(vmax);
        if ((threadIdx.x & 63) == 0) wmx[threadIdx.x >> 6] = vmax;
        __syncthreads();
        if (threadIdx.x == 0) atomicMax(row_max + b, __float_as_uint(fmaxf(fmaxf(wmx[0], wmx[1]), fmaxf(wmx[2], wmx[3]))));
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_splitter2_raw_rows(const float* __restrict__ x, float* __restrict__ out, int B, int64_t N,
                                                             const uint32_t* __restrict__ row_max) {
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const float thr = __uint_as_float(row_max[b]);
        const float delta = thr / 128.0f;
        for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < N; t += (int64_t)gridDim.x * 256)
            split2_raw(x[b * N + t], thr, delta, out[(b * 2 + 0) * N + t], out[(b * 2 + 1) * N + t]);
    }
}

// ---- fqss_nsdr ----
// grid (tiles, P): ws[p][0][tile] = sum ref^2, ws[p][1][tile] = sum (ref - est)^2 over the tile, everything in fp64
template <bool VEC>
__global__ __launch_bounds__(256) void k_nsdr_tiles(const float* __restrict__ est, const float* __restrict__ ref, double* __restrict__ ws,
                                                     int64_t N, int64_t ld_e, int64_t ld_r, int64_t ntiles) {
    __shared__ double smem[2 * 4];
    const int64_t p = blockIdx.y;
    const float *e = est + p * ld_e, *r = ref + p * ld_r;
    double acc[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t i = (int64_t)blockIdx.x * kTile + (int64_t)(j * 256 + (int)threadIdx.x) * 4;
        if (i >= N) break;
        float ve[4], vr[4];
        load_quad<VEC>(e, i, N, ve);        // past N: 0 and 0, which add nothing
        load_quad<VEC>(r, i, N, vr);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double rr = (double)vr[q], dd = rr - (double)ve[q];
            acc[0] += rr * rr;
            acc[1] += dd * dd;
        }
    }
    block_sum<double, 2>(acc, smem);
    if (threadIdx.x == 0) {
        ws[(p * 2 + 0) * ntiles + blockIdx.x] = acc[0];
        ws[(p * 2 + 1) * ntiles + blockIdx.x] = acc[1];
    }
}

__global__ __launch_bounds__(256) void k_nsdr_finish(const double* __restrict__ ws, int64_t ntiles, double* __restrict__ db) {
    __shared__ double smem[5];
    const int64_t p = blockIdx.x;
    const double num = tile_order_sum(ws + (p * 2 + 0) * ntiles, ntiles, smem);
    const double den = tile_order_sum(ws + (p * 2 + 1) * ntiles, ntiles, smem);
    if (threadIdx.x == 0) db[p] = 10.0 * log10((num + 1e-7) / (den + 1e-7));
}

// ---- fqss_frame_sdr ----
// grid (W, S): one workgroup owns window w of source s across all C channels.  A lane takes the quads tid, tid + 256, .. of the window,
// channel after channel, and keeps num, den and the two "saw a non-zero sample" marks (0 or 1: their sums on the same tree are exact) in
// registers.  ws[0][s][w] = num, ws[1][s][w] = den, ws[2][s][w] = (reference not silent) + 2 * (estimate not silent)
template <bool VEC>
__global__ __launch_bounds__(256) void k_fsdr_windows(const float* __restrict__ est, const float* __restrict__ ref, double* __restrict__ ws,
                                                       int C, int64_t win, int64_t hop, int64_t ld_e, int64_t ld_r, int64_t W) {
    __shared__ double smem[4 * 4];
    const int64_t w = blockIdx.x, s = blockIdx.y, SW = (int64_t)gridDim.y * W;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < C; ++c) {
        const float *e = est + (s * C + c) * ld_e + w * hop, *r = ref + (s * C + c) * ld_r + w * hop;
#pragma unroll 2
        for (int64_t i = (int64_t)threadIdx.x * 4; i < win; i += 1024) {
            float ve[4], vr[4];
            load_quad<VEC>(e, i, win, ve);      // past the window: 0 and 0, which add nothing and mark nothing
            load_quad<VEC>(r, i, win, vr);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double rr = (double)vr[q], dd = rr - (double)ve[q];
                acc[0] += rr * rr;
                acc[1] += dd * dd;
                if (vr[q] != 0.0f) acc[2] = 1.0;
                if (ve[q] != 0.0f) acc[3] = 1.0;
            }
        }
    }
    block_sum<double, 4>(acc, smem);
    if (threadIdx.x == 0) {
        ws[0 * SW + s * W + w] = acc[0];
        ws[1 * SW + s * W + w] = acc[1];
        ws[2 * SW + s * W + w] = (acc[2] > 0.0 ? 1.0 : 0.0) + (acc[3] > 0.0 ? 2.0 : 0.0);
    }
}

// the monotone 64-bit integer image of a double: negative values with all bits flipped, the others with the sign bit set, so that
// unsigned order is numeric order with +inf above every finite value; every NaN is the one key above +inf
constexpr unsigned long long kFsdrNanKey = ~0ull;
__device__ __forceinline__ unsigned long long fsdr_key(double v) {
    if (v != v) return kFsdrNanKey;
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __forceinline__ double fsdr_unkey(unsigned long long k) {
    return __builtin_bit_cast(double, (k >> 63) ? (k & ~(1ull << 63)) : ~k);
}

// grid (S), 1024 threads, n keys in LDS (n: the power of two >= max(W, 1)).  Every window's validity and dB value from the workspace
// (stored to frames when given), its key into LDS, the padding as NaN keys; a bitonic sort; then the ONE lane that sees the last
// non-NaN key next to a NaN key (or to the end) knows K = its index + 1 and takes the middle.  No counter: the keys fill the 64 KB.
constexpr int kFsdrThreads = 1024;
__global__ __launch_bounds__(kFsdrThreads) void k_fsdr_median(const double* __restrict__ ws, double* __restrict__ frames,
                                                               double* __restrict__ med, int S, int64_t W, int n) {
    extern __shared__ unsigned long long key[];
    const int64_t s = blockIdx.x, SW = (int64_t)S * W;
    const double nan = __builtin_nan("");
    for (int i = threadIdx.x; i < n; i += kFsdrThreads) {
        unsigned long long k = kFsdrNanKey;
        if (i < W) {
            bool valid = true;
            for (int t = 0; t < S; ++t) valid = valid && ws[2 * SW + t * W + i] == 3.0;
            double v = nan;
            if (valid) {
                const double num = ws[s * W + i], den = ws[SW + s * W + i];
                v = den == 0.0 ? __builtin_inf() : 10.0 * log10(num / den);
            }
            if (frames != nullptr) frames[s * W + i] = v;
            k = fsdr_key(v);
        }
        key[i] = k;
    }
    __syncthreads();
    for (int k2 = 2; k2 <= n; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (n >> 1); t += kFsdrThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;      // the t-th pair (i, i + j) of this round
                const unsigned long long a = key[i], b = key[p];
                if ((a > b) == ((i & k2) == 0)) {
                    key[i] = b;
                    key[p] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < n; i += kFsdrThreads) {
        if (key[i] != kFsdrNanKey && (i + 1 == n || key[i + 1] == kFsdrNanKey)) {
            const int K = i + 1;
            med[s] = (K & 1) ? fsdr_unkey(key[K >> 1]) : 0.5 * (fsdr_unkey(key[(K >> 1) - 1]) + fsdr_unkey(key[K >> 1]));
        }
    }
    if (threadIdx.x == 0 && key[0] == kFsdrNanKey) med[s] = nan;      // K = 0
}

}  // namespace fqss

using namespace fqss;

static inline bool mult4(int64_t v) { return (v & 3) == 0; }
static inline bool tiles_ok(int64_t n) { return n > 0 && cdiv(n, kTile) <= 0x7fffffff; }

extern "C" int64_t fqss_track_stats_ws_doubles(int64_t L) { return tiles_ok(L) ? 2 * cdiv(L, kTile) : 0; }

extern "C" int fqss_track_stats(const float* x, double* ws, int64_t ws_doubles, float* stats, int C, int64_t L, int64_t ld,
                                fqss_stream_t stream) {
    FQSS_REQUIRE(x && ws && stats, "null pointer");
    FQSS_REQUIRE(C > 0 && C <= 64 && tiles_ok(L) && ld >= L, "bad shape (1 <= C <= 64, L >= 1, ld >= L)");
    FQSS_REQUIRE(ws_doubles >= fqss_track_stats_ws_doubles(L), "workspace shorter than fqss_track_stats_ws_doubles");
    const int64_t ntiles = cdiv(L, kTile);
    const dim3 grid((unsigned)ntiles), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (aligned16(x) && mult4(ld)) {
        hipLaunchKernelGGL((k_track_stats_tiles<true, 1>), grid, block, 0, st, x, ws, C, L, ld, ntiles);
        hipLaunchKernelGGL((k_track_stats_tiles<true, 2>), grid, block, 0, st, x, ws, C, L, ld, ntiles);
    } else {
        hipLaunchKernelGGL((k_track_stats_tiles<false, 1>), grid, block, 0, st, x, ws, C, L, ld, ntiles);
        hipLaunchKernelGGL((k_track_stats_tiles<false, 2>), grid, block, 0, st, x, ws, C, L, ld, ntiles);
    }
    hipLaunchKernelGGL(k_track_stats_finish, dim3(1), block, 0, st, ws, ntiles, L, stats);
    return launch_status("fqss_track_stats");
}

extern "C" int fqss_chunk_gather_mc(const float* mix, const float* stats, float* out, int C, int64_t L, int64_t ld, int64_t seg,
                                    int64_t stride, int64_t k0, int G, fqss_stream_t stream) {
    FQSS_REQUIRE(mix && out, "null pointer");
    FQSS_REQUIRE(L > 0 && seg > 0 && stride > 0 && stride <= seg && C > 0 && G > 0 && (int64_t)G * C <= 65535 && ld >= L && k0 >= 0 &&
                     k0 < cdiv(L, stride),
                 "bad shape (1 <= stride <= seg, 0 <= k0 < ceil(L / stride), 1 <= G * C <= 65535, ld >= L)");
    int64_t gx = cdiv(seg, 4096);
    if (gx > 1024) gx = 1024;
    const dim3 grid((unsigned)gx, (unsigned)(G * C));
    const int64_t N = cdiv(L, stride);
    if (aligned16(mix) && aligned16(out) && mult4(ld) && mult4(seg) && mult4(stride))
        hipLaunchKernelGGL(k_chunk_gather_mc<true>, grid, dim3(256), 0, (hipStream_t)stream, mix, stats, out, C, L, ld, seg, stride, k0, N);
    else
        hipLaunchKernelGGL(k_chunk_gather_mc<false>, grid, dim3(256), 0, (hipStream_t)stream, mix, stats, out, C, L, ld, seg, stride, k0, N);
    return launch_status("fqss_chunk_gather_mc");
}

extern "C" int fqss_splitter2_raw_rows(const float* x, float* out, int B, int64_t N, uint32_t* row_max, fqss_stream_t stream) {
    FQSS_REQUIRE(x && out && row_max, "null pointer");
    FQSS_REQUIRE(B > 0 && N > 0, "bad shape");
    const dim3 grid = grid_rows(B, N, 1, 1024);
    hipLaunchKernelGGL(k_rows_absmax, grid, dim3(256), 0, (hipStream_t)stream, x, B, N, row_max);
    hipLaunchKernelGGL(k_splitter2_raw_rows, grid, dim3(256), 0, (hipStream_t)stream, x, out, B, N, row_max);
    return launch_status("fqss_splitter2_raw_rows");
}

extern "C" int64_t fqss_nsdr_ws_doubles(int P, int64_t N) { return P > 0 && P <= 65535 && tiles_ok(N) ? 2 * (int64_t)P * cdiv(N, kTile) : 0; }

extern "C" int fqss_nsdr(const float* est, const float* ref, double* ws, int64_t ws_doubles, double* db, int P, int64_t N, int64_t ld_e,
                         int64_t ld_r, fqss_stream_t stream) {
    FQSS_REQUIRE(est && ref && ws && db, "null pointer");
    FQSS_REQUIRE(P > 0 && P <= 65535 && tiles_ok(N) && ld_e >= N && ld_r >= N, "bad shape (1 <= P <= 65535, N >= 1, ld_e, ld_r >= N)");
    FQSS_REQUIRE(ws_doubles >= fqss_nsdr_ws_doubles(P, N), "workspace shorter than fqss_nsdr_ws_doubles");
    const int64_t ntiles = cdiv(N, kTile);
    const dim3 grid((unsigned)ntiles, (unsigned)P);
    if (aligned16(est) && aligned16(ref) && mult4(ld_e) && mult4(ld_r))
        hipLaunchKernelGGL(k_nsdr_tiles<true>, grid, dim3(256), 0, (hipStream_t)stream, est, ref, ws, N, ld_e, ld_r, ntiles);
    else
        hipLaunchKernelGGL(k_nsdr_tiles<false>, grid, dim3(256), 0, (hipStream_t)stream, est, ref, ws, N, ld_e, ld_r, ntiles);
    hipLaunchKernelGGL(k_nsdr_finish, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, ws, ntiles, db);
    return launch_status("fqss_nsdr");
}

static_assert(FQSS_FSDR_MAX_WINDOWS * sizeof(unsigned long long) <= 65536 && (FQSS_FSDR_MAX_WINDOWS & (FQSS_FSDR_MAX_WINDOWS - 1)) == 0,
              "the padded keys of one source are a power of two and fit in the 64 KB of LDS one workgroup may ask for");
static inline bool fsdr_shape_ok(int S, int C, int64_t L, int64_t win, int64_t hop) {
    return S >= 1 && S <= 65535 && C >= 1 && L >= 0 && win >= 1 && hop >= 1;
}
static inline int64_t fsdr_windows(int64_t L, int64_t win, int64_t hop) { return L >= win ? (L - win) / hop + 1 : 0; }

extern "C" int64_t fqss_frame_sdr_ws_doubles(int S, int C, int64_t L, int64_t win, int64_t hop) {
    if (!fsdr_shape_ok(S, C, L, win, hop)) return 0;
    const int64_t W = fsdr_windows(L, win, hop);
    return W <= FQSS_FSDR_MAX_WINDOWS ? 3 * (int64_t)S * W : 0;
}

extern "C" int fqss_frame_sdr(const float* est, const float* ref, double* ws, int64_t ws_doubles, double* frames, double* med, int S, int C,
                              int64_t L, int64_t win, int64_t hop, int64_t ld_e, int64_t ld_r, fqss_stream_t stream) {
    FQSS_REQUIRE(fsdr_shape_ok(S, C, L, win, hop), "bad shape (1 <= S <= 65535, C >= 1, L >= 0, win >= 1, hop >= 1)");
    FQSS_REQUIRE(ld_e >= L && ld_r >= L, "row stride shorter than a row (ld_e, ld_r >= L)");
    const int64_t W = fsdr_windows(L, win, hop);
    FQSS_REQUIRE(W <= FQSS_FSDR_MAX_WINDOWS, "more than FQSS_FSDR_MAX_WINDOWS windows");
    FQSS_REQUIRE(ws_doubles >= fqss_frame_sdr_ws_doubles(S, C, L, win, hop), "workspace shorter than fqss_frame_sdr_ws_doubles");
    FQSS_REQUIRE(med && (W == 0 || (est && ref && ws)), "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (W > 0) {
        const dim3 grid((unsigned)W, (unsigned)S);
        if (aligned16(est) && aligned16(ref) && mult4(ld_e) && mult4(ld_r) && mult4(hop))      // every window of every row starts on 16 bytes
            hipLaunchKernelGGL(k_fsdr_windows<true>, grid, dim3(256), 0, st, est, ref, ws, C, win, hop, ld_e, ld_r, W);
        else
            hipLaunchKernelGGL(k_fsdr_windows<false>, grid, dim3(256), 0, st, est, ref, ws, C, win, hop, ld_e, ld_r, W);
    }
    int n = 1;
    while (n < W) n <<= 1;
    hipLaunchKernelGGL(k_fsdr_median, dim3((unsigned)S), dim3(kFsdrThreads), (size_t)n * sizeof(unsigned long long), st, ws, frames, med, S,
                       W, n);
    return launch_status("fqss_frame_sdr");
}
