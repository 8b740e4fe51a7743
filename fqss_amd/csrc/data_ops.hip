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
