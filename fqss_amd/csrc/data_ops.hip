// data_ops.hip -- the arithmetic of the data side that lives in the reference's own files: the SNR
// augmentation of the LibriMix dataset (process.py:57-103 generate_2mix_snr / generate_mix_noise / max_clip, train_utils.py:30-52),
// batched on the device: one (a, b, snr) triple per row.  File reading and resampling (soundfile, torchaudio) are third party.
//   mode 0 (generate_2mix_snr): the louder-than-requested signal is attenuated:  snr_now = 10 log10(Ea / Eb);
//           snr_now < snr ? b *= sqrt((Ea / Eb) 10^(-snr/10)) : a *= sqrt((Eb / Ea) 10^(snr/10));   untouched when an energy is 0
//   mode 1 (generate_mix_noise):  b *= sqrt((Ea / Eb) / 10^(snr/10))   (gain 1 when Ea = 0)
//   then mix = a + b and max_clip: max|mix| >= 0.9 -> mix *= 0.9 / max|mix|.
// Three streams (energies, mix + peak, clip); the per-row scalars never leave the device.
#include "fqss_dev.h"

namespace fqss {

__global__ __launch_bounds__(256) void k_row_energies(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ ws, int64_t T,
                                                       int64_t ld_a, int64_t ld_b) {
    __shared__ double smem[2 * 4];
    const int64_t r = blockIdx.y;
    double v[2] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += (int64_t)gridDim.x * 256) {
        const double x = a[r * ld_a + i], y = b[r * ld_b + i];
        v[0] += x * x;
        v[1] += y * y;
    }
    block_sum<double, 2>(v, smem);
    if (threadIdx.x == 0) { atomicAdd(ws + 2 * r, v[0]); atomicAdd(ws + 2 * r + 1, v[1]); }
}

__device__ __forceinline__ void snr_gains(const double* ws, int64_t r, int64_t T, float snr, int mode, float& ga, float& gb) {
    const float Ea = (float)(ws[2 * r] / (double)T), Eb = (float)(ws[2 * r + 1] / (double)T);
    ga = gb = 1.0f;
    if (mode == 0) {
        if (Ea > 0.0f && Eb > 0.0f) {
            const float now = 10.0f * log10f(Ea / Eb);
            if (now < snr) gb = sqrtf((Ea / Eb) * powf(10.0f, -snr / 10.0f));
            else ga = sqrtf((Eb / Ea) * powf(10.0f, snr / 10.0f));
        }
    } else if (Ea > 0.0f) {
        gb = sqrtf((Ea / Eb) / powf(10.0f, snr / 10.0f));
    }
}

__global__ __launch_bounds__(256) void k_snr_mix(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ snr,
                                                  const double* __restrict__ ws, float* __restrict__ out, uint32_t* __restrict__ peak, int64_t T,
                                                  int64_t ld_a, int64_t ld_b, int64_t ld_o, int mode) {
    const int64_t r = blockIdx.y;
    float ga, gb;
    snr_gains(ws, r, T, snr[r], mode, ga, gb);
    float mx = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += (int64_t)gridDim.x * 256) {
        const float m = a[r * ld_a + i] * ga + b[r * ld_b + i] * gb;
        out[r * ld_o + i] = m;
        mx = fmaxf(mx, fabsf(m));
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) atomicMax(peak + r, __float_as_uint(mx));      // non-negative floats order like their bit patterns
}

__global__ __launch_bounds__(256) void k_max_clip(float* __restrict__ x, const uint32_t* __restrict__ peak, int64_t T, int64_t ld, float max_check,
                                                   float max_clip) {
    const int64_t r = blockIdx.y;
    const float mx = __uint_as_float(peak[r]);
    if (!(mx >= max_check)) return;
    const float gain = max_clip / mx;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += (int64_t)gridDim.x * 256) x[r * ld + i] *= gain;
}

// Polyphase sinc resampler (librimix_dataset.py:54, 111-165: torchaudio.transforms.Resample(16000, 8000) on every clip read):
//   y[r][n * nw + p] = sum_k h[p][k] * xpad[r][n * og + k],  xpad = x with `width` zeros in front (and zeros behind), K = 2 width + og
// with og / nw the reduced rate ratio (2 / 1 for 16 -> 8 kHz).  The taps h (sinc * Hann window, torchaudio's published
// _get_sinc_resample_kernel) are computed on the host in fp64; the stream is read once (the K-fold tap overlap is served by L1 / L2).
__global__ __launch_bounds__(256) void k_resample_fir(const float* __restrict__ x, const float* __restrict__ h, float* __restrict__ y,
                                                       int64_t L, int64_t Lout, int64_t ld_x, int64_t ld_y, int og, int nw, int width, int K) {
    const int64_t r = blockIdx.y;
    const float* xr = x + r * ld_x;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < Lout; o += (int64_t)gridDim.x * 256) {
        const int64_t n = o / nw;
        const int p = (int)(o - n * nw);
        const int64_t base = n * og - width;
        float acc = 0.0f;
        for (int k = 0; k < K; ++k) {
            const int64_t i = base + k;
            const float v = (i >= 0 && i < L) ? xr[i] : 0.0f;
            acc = fmaf(h[p * K + k], v, acc);
        }
        y[r * ld_y + o] = acc;
    }
}

// Stems of the htdemucs env (train_env/htdemucs_musdbhq/wav_dataset.py; reference: demucs' wav reader + the augmentation chain of
// solver.py:60-69, 314-318 -- Shift, FlipChannels, FlipSign, Scale, Remix -- folded by the host into one table row per output (b, s)):
//   b' = src_b[b,s];  c' = (C == 2 && flip[b,s]) ? 1 - c : c
//   v = float(pcm[b'][s][t + off[b,s]][c']) * 2^-15;   normalise: v = (v - mean[b']) / std[b'];   sources[b][s][c][t] = v * gain[b,s]
//   mix[b][c][t] = ((sources[b][0][c][t] + sources[b][1][c][t]) + ...)   left to right on the rounded values
// One rounding per written operation.  A pure stream: a lane takes V consecutive frames (both channels of a frame: the interleaved
// input is read once, for the stem and for the mix), walks the S stems with the mix in registers and writes V consecutive floats per
// output row -- V = 4 (16-byte stores) when T_out is a multiple of 4, which keeps every output row 16-byte aligned; V = 1 otherwise.
// `off` leaves the input frame-aligned only (4 bytes for stereo): the V frames are one load of that alignment.  The table rows are
// indexed by (blockIdx.y, s) alone, so they are scalar loads.  Every index of the table was range-checked by the host wrapper.
template <int C, int V>
__global__ __launch_bounds__(256) void k_hd_augment_mix(const int16_t* __restrict__ pcm, const float* __restrict__ mean,
                                                         const float* __restrict__ stdv, const int* __restrict__ src_b,
                                                         const int* __restrict__ off, const int* __restrict__ flip,
                                                         const float* __restrict__ gain, float* __restrict__ sources, float* __restrict__ mix,
                                                         int S, int64_t T_in, int64_t T_out, int normalise) {
    typedef float vec_t __attribute__((ext_vector_type(V)));
    struct __attribute__((packed, aligned(2 * C))) Frames { int16_t x[V * C]; };
    const int64_t b = blockIdx.y;
    const int64_t n = T_out / V;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t t = i * V;
        float acc[C][V];
        for (int s = 0; s < S; ++s) {
            const int64_t k = b * S + s;
            const int64_t bs = src_b[k];
            const bool fl = C == 2 && flip[k] != 0;
            const float g = gain[k];
            float m = 0.0f, sd = 1.0f;
            if (normalise) { m = mean[bs]; sd = stdv[bs]; }
            const Frames f = *reinterpret_cast<const Frames*>(pcm + ((bs * S + s) * T_in + t + off[k]) * C);
            float o[C][V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                int16_t raw[C];
                raw[0] = f.x[j * C];
                if (C == 2) {
                    raw[1] = f.x[j * C + 1];
                    if (fl) { const int16_t x0 = raw[0]; raw[0] = raw[1]; raw[1] = x0; }
                }
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    float v = (float)raw[c] * 0x1p-15f;
                    if (normalise) v = (v - m) / sd;
                    v = v * g;
                    o[c][j] = v;
                    acc[c][j] = s == 0 ? v : acc[c][j] + v;
                }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                vec_t w;
#pragma unroll
                for (int j = 0; j < V; ++j) w[j] = o[c][j];
                *reinterpret_cast<vec_t*>(sources + ((b * S + s) * C + c) * T_out + t) = w;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            vec_t w;
#pragma unroll
            for (int j = 0; j < V; ++j) w[j] = acc[c][j];
            *reinterpret_cast<vec_t*>(mix + (b * C + c) * T_out + t) = w;
        }
    }
}

// Sepformer recipe (train_env/speechbrain_librimix/prepare_data.py; reference: compute_forward of speechbrain_librimix_trainer.py:51-75,
// 262-326 after the speed perturbation): random circular shift per source, re-mix, WHAM noise, `wavedrop` (speechbrain's
// TimeDomainSpecAugment: DropFreq = one 101-tap FIR, the composed notches; DropChunk = zeroed intervals) and the random cut, worked
// from the training window BACKWARDS: only the window plus a 50-sample halo each side is read, and nothing of utterance length is built.
//   n = min_s L_s (min with L_n when noise is given, with L_m in premix mode);  t_s[b,p] = src_s[b][(p - shift_s) mod L_s],  0 <= p < n
//   m[b,p] = ((t_0 + t_1) + ...) (+ noise[b,p] last), one rounding per add (premix: m = mix_in, nothing summed);  m = 0 outside [0, n)
//   f[b,p] = acc_101, acc_0 = 0, acc_{k+1} = fmaf(h[k], m[b, p + k - 50], acc_k)        (filter = 0: f = m, bit for bit)
//   mix[b,q] = (exists c < n_chunk[b]: lo_c <= start + q < hi_c) ? 0 : f[b, start + q];   tgt[b,s,q] = t_s[b, start + q]
// A workgroup owns SB_TILE = 1024 outputs of one item.  Phase 1: the 256 lanes walk the SB_TILE + 100 positions of the tile and its
// halo, stride 256 (every load and every target store is one dense 1 KB line per wave); a lane gathers its position from the S rolled
// sources -- one wrap compare per source, no modulo --, forms m in registers, writes the targets of the inner positions and parks m in
// LDS as fp32 (4496 bytes), zero where p falls outside [0, n).  One barrier.  Phase 2: a lane owns 4 consecutive outputs and slides over
// its 104 LDS values as 26 ds_read_b128 (16 bytes per lane, consecutive across lanes: no bank conflict), two of them live at a time; the
// taps are indexed by the unrolled loop counter alone, so they are scalar loads; 4 independent fma chains, each in tap order k = 0..100.
// Then the chunk rows of the item (uniform per workgroup: scalar loads) and one 16-byte store (T_out % 4 == 0; scalar otherwise).
// No atomics, no workspace: the same bits every run and on any stream.  shift, start and the lengths are checked by the entry point;
// the chunk table is device memory and only selects which outputs become zero -- no index is formed from it.
constexpr int SB_TILE = 1024, SB_HALO = 50, SB_TAPS = 2 * SB_HALO + 1, SB_SPAN = SB_TILE + 2 * SB_HALO;

struct SbArgs {
    const float* src[3];
    int64_t L[3], ld[3], shift[3];
    const float* noise; int64_t ld_n;
    const float* mix_in; int64_t ld_m;
    const float* h;
    const int* chunk; const int* n_chunk;
    float* mix; float* tgt;
    int64_t n, start, T_out;
    int filter;
};

template <int S, bool WIDE>
__global__ __launch_bounds__(256) void k_sb_augment(const SbArgs a) {
    __shared__ __attribute__((aligned(16))) float m_lds[SB_SPAN];
    const int64_t b = blockIdx.y;
    const int64_t q0 = (int64_t)blockIdx.x * SB_TILE;
    const float* __restrict__ h = a.h;
    for (int i = threadIdx.x; i < SB_SPAN; i += 256) {
        const int64_t q = q0 + i - SB_HALO, p = a.start + q;
        const bool inner = i >= SB_HALO && i < SB_HALO + SB_TILE && q < a.T_out;       // inner => 0 <= p < n (start + T_out <= n)
        float m = 0.0f;
        if (p >= 0 && p < a.n) {
            const bool sum = a.mix_in == nullptr;
            if (sum || inner) {
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    int64_t j = p - a.shift[s];                                       // in (-L_s, n): one wrap brings it into [0, L_s)
                    if (j < 0) j += a.L[s];
                    const float t = a.src[s][b * a.ld[s] + j];
                    m = s == 0 ? t : m + t;
                    if (inner) a.tgt[(b * S + s) * a.T_out + q] = t;
                }
            }
            if (!sum) m = a.mix_in[b * a.ld_m + p];
            else if (a.noise) m = m + a.noise[b * a.ld_n + p];
        }
        m_lds[i] = m;
    }
    __syncthreads();
    const int o0 = 4 * threadIdx.x;
    const int64_t q = q0 + o0;
    if (q >= a.T_out) return;
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4* __restrict__ lv = reinterpret_cast<const f4*>(m_lds) + threadIdx.x;     // lv[j] = m_lds[o0 + 4 j .. + 3]
    float out[4];
    if (a.filter) {
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        f4 lo = lv[0];
#pragma unroll
        for (int kk = 0; kk < SB_TAPS; kk += 4) {                                      // taps kk .. kk + 3 see m_lds[o0 + kk .. o0 + kk + 6]
            const f4 hi = kk + 4 < SB_TAPS ? lv[kk / 4 + 1] : lo;                      // (the last round holds tap 100 alone)
            const float w[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (kk + j < SB_TAPS) {
                    const float hk = h[kk + j];
#pragma unroll
                    for (int o = 0; o < 4; ++o) acc[o] = fmaf(hk, w[j + o], acc[o]);
                }
            }
            lo = hi;
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) out[o] = acc[o];
    } else {
#pragma unroll
        for (int o = 0; o < 4; ++o) out[o] = m_lds[SB_HALO + o0 + o];
    }
    const int nc = a.n_chunk ? min(a.n_chunk[b], FQSS_SB_C_MAX) : 0;
    for (int c = 0; c < nc; ++c) {
        const int64_t lo = a.chunk[(b * FQSS_SB_C_MAX + c) * 2], hi = a.chunk[(b * FQSS_SB_C_MAX + c) * 2 + 1];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int64_t p = a.start + q + o;
            if (p >= lo && p < hi) out[o] = 0.0f;
        }
    }
    float* __restrict__ y = a.mix + b * a.T_out + q;
    if (WIDE) {
        *reinterpret_cast<f4*>(y) = f4{out[0], out[1], out[2], out[3]};
    } else {
#pragma unroll
        for (int o = 0; o < 4; ++o)
            if (q + o < a.T_out) y[o] = out[o];
    }
}

}  // namespace fqss

using namespace fqss;

extern "C" int fqss_resample_fir(const float* x, const float* h, float* y, int64_t rows, int64_t L, int64_t Lout, int64_t ld_x,
                                 int64_t ld_y, int orig, int newf, int width, fqss_stream_t stream) {
    if (rows == 0 || Lout == 0) return FQSS_OK;
    FQSS_REQUIRE(x && h && y, "null pointer");
    FQSS_REQUIRE(rows > 0 && rows <= 65535 && L > 0 && Lout > 0 && ld_x >= L && ld_y >= Lout && orig > 0 && newf > 0 && width >= 0, "bad shape");
    FQSS_REQUIRE(Lout <= (newf * L + orig - 1) / orig, "output longer than ceil(new * L / orig)");
    int64_t gx = cdiv(Lout, 1024);
    if (gx > 512) gx = 512;
    hipLaunchKernelGGL(k_resample_fir, dim3((unsigned)gx, (unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, h, y, L, Lout, ld_x, ld_y,
                       orig, newf, width, 2 * width + orig);
    return launch_status("fqss_resample_fir");
}

// a, b, out: B rows of T samples; snr [B] (dB) on the device; ws: 2*B doubles and peak: B uint32, both zeroed by the caller
extern "C" int fqss_snr_mix(const float* a, const float* b, const float* snr, double* ws, uint32_t* peak, float* out, int64_t B, int64_t T,
                            int64_t ld_a, int64_t ld_b, int64_t ld_o, int mode, int clip, fqss_stream_t stream) {
    FQSS_REQUIRE(a && b && snr && ws && peak && out, "null pointer");
    FQSS_REQUIRE(B > 0 && B <= 65535 && T > 0 && ld_a >= T && ld_b >= T && ld_o >= T && (mode == 0 || mode == 1), "bad shape");
    int64_t gx = cdiv(T, 2048);
    if (gx > 256) gx = 256;
    dim3 grid((unsigned)gx, (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_row_energies, grid, dim3(256), 0, s, a, b, ws, T, ld_a, ld_b);
    hipLaunchKernelGGL(k_snr_mix, grid, dim3(256), 0, s, a, b, snr, ws, out, peak, T, ld_a, ld_b, ld_o, mode);
    if (clip) hipLaunchKernelGGL(k_max_clip, grid, dim3(256), 0, s, out, peak, T, ld_o, 0.9f, 0.9f);
    return launch_status("fqss_snr_mix");
}

// pcm int16 [B][S][T_in][C] (frames interleaved, as the WAV files hold them); mean / std [B] (ignored unless normalise); src_b / off /
// flip / gain [B * S]; sources fp32 [B][S][C][T_out], mix fp32 [B][C][T_out].  The table is device memory: its ranges (src_b in [0, B),
// off in [0, T_in - T_out], flip in {0, 1}, finite gain, std > 0) are the caller's to check before the upload.
extern "C" int fqss_hd_augment_mix(const int16_t* pcm, const float* mean, const float* stdv, const int* src_b, const int* off, const int* flip,
                                   const float* gain, float* sources, float* mix, int B, int S, int C, int64_t T_in, int64_t T_out,
                                   int normalise, fqss_stream_t stream) {
    FQSS_REQUIRE(pcm && src_b && off && flip && gain && sources && mix && (!normalise || (mean && stdv)), "null pointer");
    FQSS_REQUIRE(B > 0 && B <= 65535 && S >= 1 && S <= 8 && (C == 1 || C == 2) && T_out > 0 && T_in >= T_out, "bad shape");
    FQSS_REQUIRE((int64_t)B * S * T_in <= (INT64_MAX >> 3) && (uintptr_t)pcm % (2 * C) == 0 && (uintptr_t)sources % 4 == 0 && (uintptr_t)mix % 4 == 0,
                 "size or alignment");
    const bool wide = T_out % 4 == 0 && (uintptr_t)sources % 16 == 0 && (uintptr_t)mix % 16 == 0;
    int64_t gx = cdiv(wide ? T_out / 4 : T_out, 256);
    if (gx > 512) gx = 512;
    const dim3 grid((unsigned)gx, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
#define FQSS_HD_AUG(CC, VV)                                                                                                                  \
    hipLaunchKernelGGL((k_hd_augment_mix<CC, VV>), grid, dim3(256), 0, st, pcm, mean, stdv, src_b, off, flip, gain, sources, mix, S, T_in, \
                       T_out, normalise)
    if (C == 2) { if (wide) FQSS_HD_AUG(2, 4); else FQSS_HD_AUG(2, 1); }
    else        { if (wide) FQSS_HD_AUG(1, 4); else FQSS_HD_AUG(1, 1); }
#undef FQSS_HD_AUG
    return launch_status("fqss_hd_augment_mix");
}

// src_s fp32 [B] rows of L_s samples, row stride ld_s (src1 / src2 NULL past S); noise / mix_in nullable, rows of L_n / L_m samples;
// taps [101] fp32 (read only when filter != 0); chunk int32 [B][FQSS_SB_C_MAX][2] = (lo, hi) and n_chunk int32 [B], both nullable
// together (no chunk anywhere); mix fp32 [B][T_out], tgt fp32 [B][S][T_out].  Everything that forms an address is checked here.
extern "C" int fqss_sb_augment(const float* src0, const float* src1, const float* src2, int64_t L0, int64_t L1, int64_t L2, int64_t ld0,
                               int64_t ld1, int64_t ld2, int64_t shift0, int64_t shift1, int64_t shift2, const float* noise, int64_t L_n,
                               int64_t ld_n, const float* mix_in, int64_t L_m, int64_t ld_m, const float* taps, const int* chunk,
                               const int* n_chunk, float* mix, float* tgt, int B, int S, int64_t start, int64_t T_out, int filter,
                               fqss_stream_t stream) {
    FQSS_REQUIRE(B > 0 && B <= 65535 && S >= 1 && S <= 3 && T_out > 0 && start >= 0, "bad shape");
    FQSS_REQUIRE(mix && tgt && (!filter || taps) && (chunk != nullptr) == (n_chunk != nullptr), "null pointer");
    SbArgs a = {};
    const float* src[3] = {src0, src1, src2};
    const int64_t L[3] = {L0, L1, L2}, ld[3] = {ld0, ld1, ld2}, shift[3] = {shift0, shift1, shift2};
    int64_t n = INT64_MAX;
    for (int s = 0; s < S; ++s) {
        FQSS_REQUIRE(src[s], "null source");
        FQSS_REQUIRE(L[s] > 0 && ld[s] >= L[s] && shift[s] >= 0 && shift[s] < L[s], "source length, stride or shift out of range");
        FQSS_REQUIRE(!mix_in || shift[s] == 0, "premix mode takes no shift");
        a.src[s] = src[s]; a.L[s] = L[s]; a.ld[s] = ld[s]; a.shift[s] = shift[s];
        if (L[s] < n) n = L[s];
    }
    if (mix_in) {
        FQSS_REQUIRE(!noise, "premix mode takes no noise");
        FQSS_REQUIRE(L_m > 0 && ld_m >= L_m, "mixture length or stride out of range");
        if (L_m < n) n = L_m;
    } else if (noise) {
        FQSS_REQUIRE(L_n > 0 && ld_n >= L_n, "noise length or stride out of range");
        if (L_n < n) n = L_n;
    }
    FQSS_REQUIRE(n < ((int64_t)1 << 31) && T_out <= n && start <= n - T_out, "window outside [0, n) (or n >= 2^31: the chunk table is int32)");
    const bool wide = T_out % 4 == 0 && (uintptr_t)mix % 16 == 0;
    a.noise = noise; a.ld_n = ld_n; a.mix_in = mix_in; a.ld_m = ld_m; a.h = taps; a.chunk = chunk; a.n_chunk = n_chunk;
    a.mix = mix; a.tgt = tgt; a.n = n; a.start = start; a.T_out = T_out; a.filter = filter ? 1 : 0;
    const dim3 grid((unsigned)cdiv(T_out, SB_TILE), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
#define FQSS_SB_AUG(SS)                                                                                   \
    do {                                                                                                  \
        if (wide) hipLaunchKernelGGL((k_sb_augment<SS, true>), grid, dim3(256), 0, st, a);                \
        else hipLaunchKernelGGL((k_sb_augment<SS, false>), grid, dim3(256), 0, st, a);                    \
    } while (0)
    if (S == 1) FQSS_SB_AUG(1); else if (S == 2) FQSS_SB_AUG(2); else FQSS_SB_AUG(3);
#undef FQSS_SB_AUG
    return launch_status("fqss_sb_augment");
}
