// repitch.hip -- demucs' repitch augmentation (pitch / tempo) of the htdemucs env on int16 stems, in integers only: a WSOLA time
// stretch whose segment positions come from a sequential search (k_rp_search), then a polyphase rate change that rebuilds the stretched
// stream tile by tile in LDS and never stores it (k_rp_resample).  The statement both kernels are pinned to, bit for bit, is in
// include/fqss.h at fqss_hd_repitch.  No floating point and no atomics: the same bits every run and on any stream.
//
// No MFMA here: the search is a correlation of 16-bit samples against a Toeplitz matrix (every candidate offset re-reads the same window
// one frame further on), so a thread that owns adjacent offsets slides one register window and feeds the packed int16 dot instruction;
// laying the window out as a dense matrix for the matrix cores would multiply the LDS traffic by the tile height for no fewer cycles.
#include "fqss_dev.h"

namespace fqss {

constexpr int kRpHs = FQSS_RP_HS, kRpV = FQSS_RP_V, kRpR = FQSS_RP_R, kRpJ = FQSS_RP_J;
constexpr int kRpWin = 2 * kRpR + kRpV;        // frames one search reads: candidates n_m - R .. n_m + R, V frames each
constexpr int kRpTile = 1024;                  // output frames per workgroup of k_rp_resample
constexpr int kRpSpan = 1184;                  // >= frames of z512 one tile reads: floor(1023 * 55 / 49) + 1 + J = 1181
static_assert(kRpWin == 6 * 256 && kRpV % 512 == 0 && kRpR % 2 == 0 && 2 * kRpR < 2048, "k_rp_search: 256 threads x 4 (+1) offsets, 11-bit offset field");
static_assert((kRpTile - 1) * 55 / 49 + 1 + kRpJ <= kRpSpan, "k_rp_resample: the tile's span of z512 fits its LDS buffer");

// pitch index 0..4 = -2..+2 semitones: rho = P / Q and the first row of that ratio's taps inside hq [FQSS_RP_HQ_ROWS][J]
struct RpRatio { int P, Q, row; };
__host__ __device__ __forceinline__ RpRatio rp_ratio(int idx) {
    switch (idx) {
    case 0: return {49, 55, 0};
    case 1: return {17, 18, 55};
    case 3: return {18, 17, 74};
    case 4: return {55, 49, 91};
    default: return {1, 1, 73};
    }
}
// segments a stream with ratio P / Q needs: stage 2 reads z512 up to index floor((T_rp - 1) P / Q) + J / 2
__host__ __device__ __forceinline__ int64_t rp_segments(int64_t T_rp, int P, int Q) { return (((T_rp - 1) * P) / Q + kRpJ / 2) / kRpHs + 1; }

typedef short rp_s2 __attribute__((ext_vector_type(2)));

// one 32-bit word of the stream at frame f, zero outside [0, T_in).  C == 2: the frame (left in the low half).  C == 1: the samples f
// and f + 1, so that a word at ANY sample offset is a ready operand of the packed dot.
template <int C>
__device__ __forceinline__ uint32_t rp_word(const int16_t* __restrict__ x, int64_t T_in, int64_t f) {
    if constexpr (C == 2) {
        return (f >= 0 && f < T_in) ? reinterpret_cast<const uint32_t*>(x)[f] : 0u;
    } else {
        const uint32_t lo = (f >= 0 && f < T_in) ? (uint16_t)x[f] : 0u, hi = (f + 1 >= 0 && f + 1 < T_in) ? (uint16_t)x[f + 1] : 0u;
        return lo | (hi << 16);
    }
}
__device__ __forceinline__ int rp_lo(uint32_t w) { return (int16_t)(w & 0xffffu); }
__device__ __forceinline__ int rp_hi(uint32_t w) { return (int16_t)(w >> 16); }
// energy of one frame: at most 2 * 2^30 = 2^31, so unsigned
template <int C>
__device__ __forceinline__ uint32_t rp_e2(uint32_t w) {
    const int l = rp_lo(w), r = rp_hi(w);
    return C == 2 ? (uint32_t)(l * l) + (uint32_t)(r * r) : (uint32_t)(l * l);
}
__device__ __forceinline__ int rp_dot2(uint32_t a, uint32_t b, int c) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(rp_s2, a), __builtin_bit_cast(rp_s2, b), c, false);
}

// The template of the next search, split for 32-bit accumulation: t = 256 * th + tl with tl = the low byte taken signed, so |tl| <= 128 and
// |th| <= 128.  tpl holds {th word, tl word} per template word (a frame when C == 2, two samples when C == 1).
template <int C>
__device__ __forceinline__ void rp_load_template(uint32_t* tpl, const int16_t* __restrict__ x, int64_t T_in, int64_t first) {
    constexpr int STEP = 3 - C, NI = kRpV / STEP;
    for (int j = threadIdx.x; j < NI; j += 256) {
        const uint32_t w = rp_word<C>(x, T_in, first + STEP * j);
        const int a = rp_lo(w), b = rp_hi(w);
        const int al = (int8_t)(a & 0xff), bl = (int8_t)(b & 0xff);
        const int ah = (a - al) >> 8, bh = (b - bl) >> 8;                 // exact: a - al is a multiple of 256
        tpl[2 * j] = ((uint32_t)ah & 0xffffu) | ((uint32_t)bh << 16);
        tpl[2 * j + 1] = ((uint32_t)al & 0xffffu) | ((uint32_t)bl << 16);
    }
}

// Stage 1.  One workgroup per stream walks its segments in order; the only dependence between segments is p_{m-1} -> the template.
//   cost(d) - |t|^2 = E(d) - 2 corr(d),   E(d) = sum of the window's squares,   corr(d) = sum of x[n_m + d + i][c] * t[i][c]
// (|t|^2 is the same for every d and is left out of the arg-min).  Thread `tid` owns the offsets e = d + R = 4 tid .. 4 tid + 4 (the fifth
// repeats its neighbour's first, except for thread 255 whose fifth is e = 2R): its window words slide through registers, four new ones
// per ds_read_b128, while the template words are LDS broadcasts.
// Bounds.  One packed dot adds two products of |x| <= 2^15 and |th|, |tl| <= 2^7: at most 2^23.  A 32-bit accumulator takes 128 of them
// (128 template words = 256 products), at most 2^30, and is then folded into int64 as 256 * hi + lo.  |corr| <= V * C * 2^30 = 2^40,
// E <= V * 2^31 = 2^40, so cost' + 2^41 lies in [0, 2^43) and (cost' + 2^41) << 11 | e fits uint64; the minimum of that key is the lowest
// cost and, among equal costs, the lowest offset.
template <int C>
__global__ __launch_bounds__(256) void k_rp_search(const int16_t* __restrict__ pcm, const int* __restrict__ rows, int* __restrict__ pos_ws,
                                                   int64_t T_in, int64_t T_rp, int M) {
    constexpr int STEP = 3 - C;                // window words between two template words
    constexpr int NI = kRpV / STEP;            // template words
    constexpr int WN = 4 + 4 * STEP;           // window words in registers for 4 template words x 5 offsets
    constexpr int PF = kRpWin / 256;           // window words a thread fetches ahead
    __shared__ __attribute__((aligned(16))) uint32_t win[2][kRpWin];
    __shared__ __attribute__((aligned(16))) uint32_t tpl[2 * kRpV];
    __shared__ uint64_t csum[kRpWin / 4];
    __shared__ uint64_t red[4];
    const int tid = threadIdx.x;
    const int64_t bs = blockIdx.x;
    const int16_t* x = pcm + bs * T_in * C;
    int* pos = pos_ws + bs * M;
    const int on = rows[3 * bs], A = rows[3 * bs + 2];
    const RpRatio rt = rp_ratio(rows[3 * bs + 1]);
    int Mrow = 0;
    if (on) {
        const int64_t need = rp_segments(T_rp, rt.P, rt.Q);
        Mrow = need < M ? (int)need : M;
    }
    for (int m = tid; m < M; m += 256)
        if (m == 0 || m >= Mrow) pos[m] = 0;   // p_0 = 0; columns this stream does not use
    if (Mrow <= 1) return;                     // the same for every thread of the workgroup

    {
        const int64_t n1 = ((int64_t)kRpHs * A) >> 16;
#pragma unroll
        for (int q = 0; q < PF; ++q) win[0][tid + 256 * q] = rp_word<C>(x, T_in, n1 - kRpR + tid + 256 * q);
        rp_load_template<C>(tpl, x, T_in, kRpHs);
    }
    __syncthreads();
    const int e0 = 4 * tid;
    int cur = 0;
    for (int m = 1; m < Mrow; ++m) {
        const int64_t n = ((int64_t)m * kRpHs * A) >> 16;
        const bool more = m + 1 < Mrow;
        uint32_t pf[PF];                       // the next segment's window does not wait for this search: in flight under it
        if (more) {
            const int64_t nn = ((int64_t)(m + 1) * kRpHs * A) >> 16;
#pragma unroll
            for (int q = 0; q < PF; ++q) pf[q] = rp_word<C>(x, T_in, nn - kRpR + tid + 256 * q);
        }
        const uint32_t* w = win[cur];
        for (int q = tid; q < kRpWin / 4; q += 256) {
            const uint4 v = *reinterpret_cast<const uint4*>(w + 4 * q);
            csum[q] = (uint64_t)rp_e2<C>(v.x) + rp_e2<C>(v.y) + rp_e2<C>(v.z) + rp_e2<C>(v.w);
        }
        __syncthreads();
        uint64_t E = 0;                        // E(e0): V frames = V / 4 sums of four
#pragma unroll 8
        for (int q = 0; q < kRpV / 4; ++q) E += csum[tid + q];

        int64_t corr[5] = {0, 0, 0, 0, 0};
        uint32_t wb[WN];
        {
            const uint4 v = *reinterpret_cast<const uint4*>(w + e0);
            wb[WN - 4] = v.x; wb[WN - 3] = v.y; wb[WN - 2] = v.z; wb[WN - 1] = v.w;
        }
        for (int g = 0; g < NI; g += 128) {
            int ah[5] = {0, 0, 0, 0, 0}, al[5] = {0, 0, 0, 0, 0};
#pragma unroll 2
            for (int i0 = g; i0 < g + 128; i0 += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) wb[u] = wb[WN - 4 + u];
#pragma unroll
                for (int u = 0; u < STEP; ++u) {
                    const uint4 v = *reinterpret_cast<const uint4*>(w + e0 + STEP * i0 + 4 + 4 * u);
                    wb[4 + 4 * u] = v.x; wb[5 + 4 * u] = v.y; wb[6 + 4 * u] = v.z; wb[7 + 4 * u] = v.w;
                }
                const uint4 t0 = *reinterpret_cast<const uint4*>(tpl + 2 * i0), t1 = *reinterpret_cast<const uint4*>(tpl + 2 * i0 + 4);
                const uint32_t th[4] = {t0.x, t0.z, t1.x, t1.z}, tl[4] = {t0.y, t0.w, t1.y, t1.w};
#pragma unroll
                for (int ii = 0; ii < 4; ++ii)
#pragma unroll
                    for (int dd = 0; dd < 5; ++dd) {
                        ah[dd] = rp_dot2(wb[dd + STEP * ii], th[ii], ah[dd]);
                        al[dd] = rp_dot2(wb[dd + STEP * ii], tl[ii], al[dd]);
                    }
            }
#pragma unroll
            for (int dd = 0; dd < 5; ++dd) corr[dd] += (int64_t)ah[dd] * 256 + al[dd];
        }
        uint64_t best = ~0ull;
#pragma unroll
        for (int dd = 0; dd < 5; ++dd) {
            if (dd) E = E - rp_e2<C>(w[e0 + dd - 1]) + rp_e2<C>(w[e0 + dd - 1 + kRpV]);
            const int64_t cost = (int64_t)E - 2 * corr[dd];
            const uint64_t key = ((uint64_t)(cost + ((int64_t)1 << 41)) << 11) | (uint32_t)(e0 + dd);
            best = key < best ? key : best;
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            const uint64_t other = __shfl_xor(best, o);
            best = other < best ? other : best;
        }
        if ((tid & 63) == 0) red[tid >> 6] = best;
        __syncthreads();                       // every wave is also done with tpl and, since the last iteration, with win[cur ^ 1]
        const uint64_t k01 = red[0] < red[1] ? red[0] : red[1], k23 = red[2] < red[3] ? red[2] : red[3];
        const int64_t p = n - kRpR + (int64_t)((k01 < k23 ? k01 : k23) & 2047u);
        if (tid == 0) pos[m] = (int)p;
        if (more) {
#pragma unroll
            for (int q = 0; q < PF; ++q) win[cur ^ 1][tid + 256 * q] = pf[q];
            rp_load_template<C>(tpl, x, T_in, p + kRpHs);
        }
        __syncthreads();
        cur ^= 1;
    }
}

// one frame of the stream as integers, zero outside [0, T_in)
template <int C>
__device__ __forceinline__ void rp_frame(const int16_t* __restrict__ x, int64_t T_in, int64_t f, int (&v)[C]) {
    if constexpr (C == 2) {
        const uint32_t w = rp_word<2>(x, T_in, f);
        v[0] = rp_lo(w);
        v[1] = rp_hi(w);
    } else {
        v[0] = (f >= 0 && f < T_in) ? x[f] : 0;
    }
}

// Stage 2.  grid (tiles of 1024 output frames, streams).  A stream that is off copies its tile.  A stream that is on rebuilds the span
// of z512 its tile reads -- at most 1181 frames, two int16 loads and one integer blend per element -- in LDS next to its ratio's taps,
// then every output is J 32 x 32 -> 64-bit multiply-adds read from LDS.  |z512| <= 2^24 and the taps of a phase sum to 2^15 with
// sum |h| < 2^17, so |acc| < 2^41.
template <int C>
__global__ __launch_bounds__(256) void k_rp_resample(const int16_t* __restrict__ pcm, const int* __restrict__ rows, const int* __restrict__ hq,
                                                     const int* __restrict__ pos_ws, int16_t* __restrict__ out, int64_t T_in, int64_t T_rp, int M) {
    __shared__ int zs[kRpSpan * C];
    __shared__ int hs[55 * kRpJ];
    const int tid = threadIdx.x;
    const int64_t bs = blockIdx.y, n0 = (int64_t)blockIdx.x * kRpTile;
    const int cnt = T_rp - n0 < kRpTile ? (int)(T_rp - n0) : kRpTile;
    const int16_t* x = pcm + bs * T_in * C;
    int16_t* y = out + bs * T_rp * C;
    if (!rows[3 * bs]) {                       // T_rp <= T_in: a crop
        for (int k = tid; k < cnt; k += 256) {
            if constexpr (C == 2) reinterpret_cast<uint32_t*>(y)[n0 + k] = reinterpret_cast<const uint32_t*>(x)[n0 + k];
            else y[n0 + k] = x[n0 + k];
        }
        return;
    }
    const RpRatio rt = rp_ratio(rows[3 * bs + 1]);
    const int* pos = pos_ws + bs * M;
    const int64_t c_lo = (n0 * rt.P) / rt.Q;
    const int phi_lo = (int)(n0 * rt.P - c_lo * rt.Q);
    const int64_t z0 = c_lo - kRpJ / 2 + 1;                                         // the first index of z512 the tile reads
    const int span = min(kRpSpan, (phi_lo + (cnt - 1) * rt.P) / rt.Q + kRpJ);      // the last one is c_hi + J / 2
    for (int k = tid; k < rt.Q * kRpJ; k += 256) hs[k] = hq[rt.row * kRpJ + k];
    for (int k = tid; k < span; k += 256) {
        const int64_t idx = z0 + k;
        int v[C];
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = 0;
        const int m = idx >= 0 ? (int)(idx / kRpHs) : M;
        if (m < M) {
            const int i = (int)(idx - (int64_t)m * kRpHs);
            int a[C];
            rp_frame<C>(x, T_in, (int64_t)pos[m] + i, a);
            if (m >= 1 && i < kRpV) {
                int t[C];
                rp_frame<C>(x, T_in, (int64_t)pos[m - 1] + kRpHs + i, t);
#pragma unroll
                for (int c = 0; c < C; ++c) v[c] = (kRpV - i) * t[c] + i * a[c];
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) v[c] = kRpV * a[c];
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) zs[k * C + c] = v[c];
    }
    __syncthreads();
    for (int k = tid; k < cnt; k += 256) {
        const int u = phi_lo + k * rt.P, dc = u / rt.Q, phi = u - dc * rt.Q;       // c = c_lo + dc; its first tap reads index c - J/2 + 1
        const int* h = hs + phi * kRpJ;
        const int* z = zs + dc * C;
        int64_t acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0;
#pragma unroll 8
        for (int j = 0; j < kRpJ; ++j)
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += (int64_t)h[j] * z[j * C + c];
        int r[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int64_t s = (acc[c] + (1 << 23)) >> 24;
            r[c] = (int)(s < -32768 ? -32768 : s > 32767 ? 32767 : s);
        }
        if constexpr (C == 2) reinterpret_cast<uint32_t*>(y)[n0 + k] = ((uint32_t)r[0] & 0xffffu) | ((uint32_t)r[1] << 16);
        else y[n0 + k] = (int16_t)r[0];
    }
}
}  // namespace fqss

using namespace fqss;

extern "C" int64_t fqss_hd_repitch_ws_bytes(int B, int S, int64_t T_rp) {
    if (B < 1 || S < 1 || T_rp < 1 || T_rp >= ((int64_t)1 << 30)) return -1;
    return (int64_t)B * S * rp_segments(T_rp, 55, 49) * (int64_t)sizeof(int);
}

// pcm int16 [B][S][T_in][C]; rows int32 [B * S][3] = (on, pitch index, A); hq int32 [FQSS_RP_HQ_ROWS][FQSS_RP_J]; pos_ws int32
// [B * S][M], M = fqss_hd_repitch_ws_bytes / (4 B S); out int16 [B][S][T_rp][C].  Every read of pcm is guarded by [0, T_in) and every index
// into pos_ws and hq by M and the ratio table, whatever the rows hold; their ranges are still the caller's to check before the upload.
// stages: FQSS_RP_SEARCH | FQSS_RP_RESAMPLE; the rate change alone reads the positions an earlier search left in pos_ws.
extern "C" int fqss_hd_repitch(const int16_t* pcm, const int* rows, const int* hq, int* pos_ws, int16_t* out, int B, int S, int C, int64_t T_in,
                               int64_t T_rp, int stages, fqss_stream_t stream) {
    FQSS_REQUIRE(pcm && rows && hq && pos_ws && out, "null pointer");
    FQSS_REQUIRE(B > 0 && S > 0 && (int64_t)B * S <= 65535 && (C == 1 || C == 2) && T_rp > 0 && T_in >= T_rp && T_in < ((int64_t)1 << 30) && stages >= 1 && stages <= 3,
                 "bad shape");
    FQSS_REQUIRE((uintptr_t)pcm % (2 * C) == 0 && (uintptr_t)out % (2 * C) == 0 && (uintptr_t)rows % 4 == 0 && (uintptr_t)hq % 4 == 0 &&
                 (uintptr_t)pos_ws % 4 == 0, "alignment");
    const int n = B * S, M = (int)rp_segments(T_rp, 55, 49);
    const dim3 tiles((unsigned)cdiv(T_rp, kRpTile), (unsigned)n);
    hipStream_t st = (hipStream_t)stream;
    const bool search = stages & FQSS_RP_SEARCH, resample = stages & FQSS_RP_RESAMPLE;
    if (C == 2) {
        if (search) hipLaunchKernelGGL(k_rp_search<2>, dim3(n), dim3(256), 0, st, pcm, rows, pos_ws, T_in, T_rp, M);
        if (resample) hipLaunchKernelGGL(k_rp_resample<2>, tiles, dim3(256), 0, st, pcm, rows, hq, pos_ws, out, T_in, T_rp, M);
    } else {
        if (search) hipLaunchKernelGGL(k_rp_search<1>, dim3(n), dim3(256), 0, st, pcm, rows, pos_ws, T_in, T_rp, M);
        if (resample) hipLaunchKernelGGL(k_rp_resample<1>, tiles, dim3(256), 0, st, pcm, rows, hq, pos_ws, out, T_in, T_rp, M);
    }
    return launch_status("fqss_hd_repitch");
}
