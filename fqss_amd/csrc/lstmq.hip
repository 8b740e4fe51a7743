// lstmq.hip -- the recurrence of LSTMQ_static (qat_layers.py:741-862 of the reference): the bidirectional single-layer LSTM with twelve
// learned-range 8-bit activation quantizers per direction applied at EVERY time step,
//     ih = fq(x W_ih^T + b_ih)      hh = fq(h W_hh^T + b_hh)       gates = fq_add0(ih + hh)
//     i = fq_sig0(sigmoid(.))   f = fq_sig1(sigmoid(.))   g = fq_tanh0(tanh(.))   o = fq_sig2(sigmoid(.))
//     c = fq_add1(fq_mul0(f c) + fq_mul1(i g))               h = fq_mul2(o fq_tanh1(tanh(c)))
// The reverse direction's h goes through the FORWARD direction's mul2 quantizer (the reference's line 835, kept for checkpoint
// compatibility): the kernels read ranges[0][mul2] / add into gaccs[0][mul2] for both directions and never touch [1][mul2].
//
// As in lstm.hip the input projection of both directions is one row GEMM in front (`pre`, un-quantized: fq_ih is applied here) and the
// weight / input gradients are row GEMMs behind the backward kernel.  Same mapping: a workgroup owns kNB = 2 sequences of one
// direction for all of its steps, one thread per gate row, no grid synchronisation.  A launch processes the steps [k0, k1) of the
// S-step sequence in processing order (step k = time k forward, time S-1-k reverse) from a carried state (h0, c0) and hands the
// state after step k1-1 on (hc_last): the module runs its observing prefix step by step and the rest of the sequence here.
// The quantizer arithmetic is fq_asym / load_qrange of fqss_dev.h op for op; the twelve ranges of a direction are derived once per
// workgroup into LDS (wave-uniform broadcast reads); sigmoid / tanh are the gate functions of lstm.hip (fqss_lstm_gate_fn).
//
// Saved for the backward, per (step, sequence, direction): the value W_hh h + b_hh in front of fq_hh (4H floats: the one quantizer
// input that cannot be recomputed from its upstream) and the cell state behind fq_add1 (H floats) -- 20 H bytes, against 24 H of the
// float recurrence.  The backward recomputes every other quantizer input from `pre`, these two images and c of the step before with
// the SAME device functions (same operations in the same order: the same bits), so each STE sees exactly the forward's (u, code).
// STE (qat_quant.py:139-146): pass-through inside the clip range, +-(round(u) - u)/255 into min / max inside, 1 into the clipped
// bound outside; the range partials are summed in fp64 per thread, reduced per workgroup and added to that workgroup's own gacc slot.
//
// Two forward forms share the element-wise device functions: the generic one (any H <= 256, W_hh streamed from L2, one thread per gate
// row like k_lstm_fwd) and the register-resident H = 128 specialisation (like k_lstm_fwd_st).  The backward has the generic form only
// (H = 128 runs on it: the register-resident quad split of k_lstm_bwd<128> is not built for the quantized recurrence yet).
#include <cstdlib>

#include "fqss_dev.h"

namespace fqss {
namespace {

constexpr int kNB = 2;   // sequences per workgroup (lstm.hip)

enum { Q_IH = 0, Q_HH, Q_ADD0, Q_SIG0, Q_SIG1, Q_SIG2, Q_TANH0, Q_TANH1, Q_MUL0, Q_MUL1, Q_ADD1, Q_MUL2, kNQ };

struct LstmqRanges { const float* p[2][kNQ][2]; };   // [direction][quantizer][min, max] device scalars
struct LstmqGaccs { double* p[2][kNQ]; };            // [direction][quantizer] FQSS_GACC_SLOTS x 3 doubles

// the gate functions of the H = 128 float forward (lstm.hip gate_fn, verbatim: what fqss_lstm_gate_fn evaluates)
__device__ __forceinline__ float gate_fn(float x, bool th) {
    const float a = fabsf(x);
    const float z = __builtin_amdgcn_fmed3f(th ? a : x, -87.0f, 87.0f);
    const float kh = th ? -2.8853900432586669921875f : -1.44269502162933349609375f;
    const float kl = th ? -3.851925849e-08f : -1.925962925e-08f;
    const float t = kh * z;
    const float tl = fmaf(kl, z, fmaf(kh, z, -t));
    const float e = __builtin_amdgcn_exp2f(t);
    const float corr = fmaf(tl, 0.693147182464599609375f, 1.0f);
    const float d = fmaf(e, corr, 1.0f);
    const float n = th ? fmaf(-e, corr, 1.0f) : 1.0f;
    const float r = __builtin_amdgcn_rcpf(d);
    float q = n * r;
    q = fmaf(fmaf(-d, q, n), r, q);
    if (!th) return (x != x) ? x : q;
    const float u = a * a;
    float p = fmaf(u, 0.019728317856788635f, -0.0537986196577549f);
    p = fmaf(u, p, 0.13332897424697876f);
    p = fmaf(u, p, -0.3333333134651184f);
    const float small = fmaf(a * u, p, a);
    return copysignf(a < 0.36f ? small : q, x);
}

__device__ __forceinline__ float fq(float t, const QRange& r) {
    float c, u;
    bool inr;
    return fq_asym(t, r, c, u, inr);
}

// STE + range partials of one quantizer at one element (the arithmetic of k_actq_bwd, ACT_NONE)
__device__ __forceinline__ float ste(float t, float g, const QRange& r, double& p_du, double& p_out) {
    float c, u;
    bool inr;
    (void)fq_asym(t, r, c, u, inr);
    p_du += (double)(g * (inr ? (c - u) : c));
    p_out += (double)(inr ? 0.0f : g);
    return inr ? div_by(g * r.delta, r.delta, r.inv) : 0.0f;
}

// quantizer of gate block 0..3 (i, f, g, o)
__device__ __forceinline__ int gate_q(int gk) { return gk == 0 ? Q_SIG0 : (gk == 1 ? Q_SIG1 : (gk == 2 ? Q_TANH0 : Q_SIG2)); }

// one gate row: the three quantizers in front of the non-linearity; returns the argument of sigmoid / tanh
__device__ __forceinline__ float gate_arg(float p, float hhraw, const QRange* qr, float& sum) {
    sum = fq(p, qr[Q_IH]) + fq(hhraw, qr[Q_HH]);
    return fq(sum, qr[Q_ADD0]);
}

struct CellVals { float x0, x1, xs, c, th, tq, xh, h; };     // quantizer inputs of the cell update, in order; c / h: the new state
__device__ __forceinline__ CellVals cell_fwd(float gi, float gf, float gg, float go, float c_prev, const QRange* qr) {
    CellVals v;
    v.x0 = gf * c_prev;
    v.x1 = gi * gg;
    v.xs = fq(v.x0, qr[Q_MUL0]) + fq(v.x1, qr[Q_MUL1]);
    v.c = fq(v.xs, qr[Q_ADD1]);
    v.th = gate_fn(v.c, true);
    v.tq = fq(v.th, qr[Q_TANH1]);
    v.xh = go * v.tq;
    v.h = fq(v.xh, qr[Q_MUL2]);
    return v;
}

__device__ __forceinline__ void load_ranges(QRange* qr, const LstmqRanges& R, int dir) {
    if (threadIdx.x < kNQ) {
        const int d = threadIdx.x == Q_MUL2 ? 0 : dir;      // both directions' h on the forward direction's mul2 grid
        qr[threadIdx.x] = load_qrange(R.p[d][threadIdx.x][0], R.p[d][threadIdx.x][1]);
    }
}

// pre   [S][B][2][4H]  x W_ih^T + b_ih, un-quantized (gate order i, f, g, o)
// whh   [2][4H][H], bhh [2][4H];  h0 / c0 [2][B][H] state after step k0-1 (null: zeros)
// hout  [S][B][2H]     (forward | reverse halves; only the times of the steps [k0, k1) are written)
// hc_last [2][2][B][H] h | c after step k1-1 (nullable)
// hsav  [S][B][2][4H]  W_hh h + b_hh,  csav [S][B][2][H] cell state  (both null: inference)
__global__ __launch_bounds__(1024) void k_lstmq_fwd(const float* __restrict__ pre, const float* __restrict__ whh, const float* __restrict__ bhh,
                                                    const float* __restrict__ h0, const float* __restrict__ c0, const LstmqRanges R,
                                                    float* __restrict__ hout, float* __restrict__ hc_last, float* __restrict__ hsav,
                                                    float* __restrict__ csav, int S, int B, int H, int k0, int k1) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ QRange qr[kNQ];
    float* hs = smem;                        // [kNB][H]
    float* gs = smem + kNB * (H + 16);       // [kNB][4H]
    const int dir = blockIdx.y;
    const int b0 = blockIdx.x * kNB;
    const int j = threadIdx.x;               // gate row (j < 4H)
    const bool jv = j < 4 * H;
    const float* W = whh + ((int64_t)dir * 4 * H + (jv ? j : 0)) * H;
    const float bj = jv ? bhh[dir * 4 * H + j] : 0.f;
    load_ranges(qr, R, dir);
    for (int e = threadIdx.x; e < kNB * H; e += blockDim.x) {
        const int nb = e / H, k = e - nb * H;
        hs[e] = (h0 != nullptr && b0 + nb < B) ? h0[((int64_t)dir * B + b0 + nb) * H + k] : 0.f;
    }
    const int cn = threadIdx.x / H, ck = threadIdx.x - cn * H;
    const bool cell = threadIdx.x < kNB * H && (b0 + cn) < B;
    float c = (cell && c0 != nullptr) ? c0[((int64_t)dir * B + b0 + cn) * H + ck] : 0.f;
    float h = (cell && h0 != nullptr) ? h0[((int64_t)dir * B + b0 + cn) * H + ck] : 0.f;
    __syncthreads();
    const int gk = jv ? j / H : 0;           // gate kind: wave-uniform for H % 64 == 0
    const bool is_g = gk == 2;
    const int qg = gate_q(gk);
    // the input projection of a step is requested kPF steps ahead (k_lstm_fwd): unconditional loads from clamped indices
    constexpr int kPF = 4;
    float pf[kPF][kNB];
    const int jc = jv ? j : 4 * H - 1;
    auto fetch = [&](float (&dst)[kNB], int step) {
        const int sn = min(step, S - 1);
        const int tn = dir == 0 ? sn : S - 1 - sn;
#pragma unroll
        for (int nb = 0; nb < kNB; ++nb) dst[nb] = pre[(((int64_t)tn * B + min(b0 + nb, B - 1)) * 2 + dir) * 4 * H + jc];
    };
#pragma unroll
    for (int u = 0; u < kPF; ++u) fetch(pf[u], k0 + u);
    auto one_step = [&](int step, const float (&pcur)[kNB]) {
        const int t = dir == 0 ? step : S - 1 - step;
        if (jv) {
            float acc[kNB];
#pragma unroll
            for (int nb = 0; nb < kNB; ++nb) acc[nb] = 0.f;
            for (int k = 0; k < H; ++k) {
                const float wv = W[k];
#pragma unroll
                for (int nb = 0; nb < kNB; ++nb) acc[nb] = fmaf(wv, hs[nb * H + k], acc[nb]);
            }
#pragma unroll
            for (int nb = 0; nb < kNB; ++nb) {
                const float hhraw = acc[nb] + bj;
                float sum;
                const float a = gate_fn(gate_arg(pcur[nb], hhraw, qr, sum), is_g);
                gs[nb * 4 * H + j] = fq(a, qr[qg]);
                if (hsav != nullptr && b0 + nb < B) hsav[((((int64_t)t * B + b0 + nb) * 2) + dir) * 4 * H + j] = hhraw;
            }
        }
        __syncthreads();
        if (cell) {
            const float* g = gs + cn * 4 * H;
            const CellVals v = cell_fwd(g[ck], g[H + ck], g[2 * H + ck], g[3 * H + ck], c, qr);
            c = v.c;
            h = v.h;
            hs[cn * H + ck] = h;
            const int64_t sb = (int64_t)t * B + b0 + cn;
            hout[sb * 2 * H + dir * H + ck] = h;
            if (csav != nullptr) csav[(sb * 2 + dir) * H + ck] = c;
        }
        __syncthreads();
    };
    int step = k0;
    for (; step + kPF <= k1; step += kPF) {
#pragma unroll
        for (int u = 0; u < kPF; ++u) {
            float pc[kNB];
#pragma unroll
            for (int nb = 0; nb < kNB; ++nb) pc[nb] = pf[u][nb];
            fetch(pf[u], step + u + kPF);
            one_step(step + u, pc);
        }
    }
#pragma unroll
    for (int u = 0; u < kPF - 1; ++u)       // the last (k1 - k0) % kPF steps: already in the ring
        if (step + u < k1) one_step(step + u, pf[u]);
    if (cell && hc_last != nullptr) {
        hc_last[((int64_t)dir * B + b0 + cn) * H + ck] = h;
        hc_last[((int64_t)(2 + dir) * B + b0 + cn) * H + ck] = c;
    }
}

// The register-resident H = 128 forward: the mapping of k_lstm_fwd_st (lstm.hip) -- W_hh in 128 VGPRs per thread for the whole launch, a
// quad of lanes shares four gate rows and each lane keeps one k-quarter of them, partial sums meet by quad-permute DPP adds, the two
// sequences half a step apart (a phase = the cell update of the OTHER sequence on two waves + this sequence's 128 FMAs per lane on all
// waves), the input projection requested four steps ahead -- with the element-wise device functions of the generic form in place of the
// float gate / cell arithmetic.  The gate kind, and so which of sig0 / sig1 / tanh0 / sig2 applies, is wave-uniform; the ranges are read
// from LDS at one address per wave.  The sums of W_hh h are formed in another order than in the generic form (quarters, then the quad):
// the saved hsav carries this form's bits, and the backward reads them rather than recomputing the product.
template <int H>
__global__ __launch_bounds__(4 * H) void k_lstmq_fwd_st(const float* __restrict__ pre, const float* __restrict__ whh, const float* __restrict__ bhh,
                                                        const float* __restrict__ h0, const float* __restrict__ c0, const LstmqRanges R,
                                                        float* __restrict__ hout, float* __restrict__ hc_last, float* __restrict__ hsav,
                                                        float* __restrict__ csav, int S, int B, int k0, int k1) {
    static_assert(kNB == 2 && H % 64 == 0, "two sequences half a step apart; wave-uniform gate kinds and cell roles");
    constexpr int KQ = H / 4, HQS = KQ + 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ QRange qr[kNQ];
    float* hs = smem;                              // [kNB][4 quarters][HQS]
    float* gs = smem + kNB * 4 * HQS;              // [kNB][4H]
    const int dir = blockIdx.y;
    const int b0 = blockIdx.x * kNB;
    const int j = threadIdx.x;                     // gate row
    const int q4 = j >> 2, kq = j & 3;
    float wreg[H];
    {
        const float* Wq = whh + ((int64_t)dir * 4 * H + q4 * 4) * H + kq * KQ;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int k = 0; k < KQ; ++k) wreg[r * KQ + k] = Wq[(int64_t)r * H + k];
    }
    const float bj = bhh[dir * 4 * H + j];
    load_ranges(qr, R, dir);
    for (int e = threadIdx.x; e < kNB * 4 * HQS; e += blockDim.x) {
        const int nb = e / (4 * HQS), rem = e - nb * 4 * HQS, qt = rem / HQS, pos = rem - qt * HQS;
        hs[e] = (pos < KQ && h0 != nullptr && b0 + nb < B) ? h0[((int64_t)dir * B + b0 + nb) * H + qt * KQ + pos] : 0.f;
    }
    // cell roles: threads [0, H) keep sequence 1's cell state, threads [H, 2H) sequence 0's (whole waves)
    const int crole = j < H ? 1 : (j < 2 * H ? 0 : -1);
    const int ck = j & (H - 1);
    const bool cell_ok = crole >= 0 && b0 + crole < B;
    const int64_t st = cell_ok ? ((int64_t)dir * B + b0 + crole) * H + ck : 0;      // this thread's element of a [2][B][H] state
    float c = (cell_ok && c0 != nullptr) ? c0[st] : 0.f;
    float h = (cell_ok && h0 != nullptr) ? h0[st] : 0.f;
    __syncthreads();
    constexpr int kPF = 4;
    float pf[kPF][kNB];
    auto fetch = [&](float (&dst)[kNB], int step) {
        const int sn = min(step, S - 1);
        const int tn = dir == 0 ? sn : S - 1 - sn;
#pragma unroll
        for (int nb = 0; nb < kNB; ++nb) dst[nb] = pre[(((int64_t)tn * B + min(b0 + nb, B - 1)) * 2 + dir) * 4 * H + j];
    };
#pragma unroll
    for (int u = 0; u < kPF; ++u) fetch(pf[u], k0 + u);
    const int gk = j / H;                          // gate order i, f, g, o; wave-uniform
    const bool is_g = gk == 2;
    const int qg = gate_q(gk);
    auto time_of = [&](int step) { return dir == 0 ? step : S - 1 - step; };
    auto cell_update = [&](int nb, int step) {               // by the threads whose role is nb (wave-uniform branch at the call)
        const float* g = gs + nb * 4 * H;
        const CellVals v = cell_fwd(g[ck], g[H + ck], g[2 * H + ck], g[3 * H + ck], c, qr);
        c = v.c;
        h = v.h;
        hs[(nb * 4 + ck / KQ) * HQS + (ck % KQ)] = h;
        const int64_t sb = (int64_t)time_of(step) * B + b0 + nb;
        hout[sb * 2 * H + dir * H + ck] = h;
        if (csav != nullptr) csav[(sb * 2 + dir) * H + ck] = c;
    };
    auto gates = [&](int nb, int step, float pcur) {         // W_hh h_{t-1} of sequence nb, the quantizers around its gate function
        float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KQ; k += 4) {
            const float4 hv = *reinterpret_cast<const float4*>(hs + (nb * 4 + kq) * HQS + k);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                part[r] = fmaf(wreg[r * KQ + k], hv.x, part[r]);
                part[r] = fmaf(wreg[r * KQ + k + 1], hv.y, part[r]);
                part[r] = fmaf(wreg[r * KQ + k + 2], hv.z, part[r]);
                part[r] = fmaf(wreg[r * KQ + k + 3], hv.w, part[r]);
            }
        }
        float mine = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = part[r];
            v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
            v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
            mine = (kq == r) ? v : mine;
        }
        const float hhraw = mine + bj;
        float sum;
        const float a = gate_fn(gate_arg(pcur, hhraw, qr, sum), is_g);
        gs[nb * 4 * H + j] = fq(a, qr[qg]);
        if (hsav != nullptr && b0 + nb < B) hsav[((((int64_t)time_of(step) * B + b0 + nb) * 2) + dir) * 4 * H + j] = hhraw;
    };
    auto one_step = [&](int step, const float (&pcur)[kNB]) {
        if (crole == 1 && cell_ok && step > k0) cell_update(1, step - 1);
        gates(0, step, pcur[0]);
        __syncthreads();
        if (crole == 0 && cell_ok) cell_update(0, step);
        gates(1, step, pcur[1]);
        __syncthreads();
    };
    int step = k0;
    for (; step + kPF <= k1; step += kPF) {
#pragma unroll
        for (int u = 0; u < kPF; ++u) {
            float pc[kNB];
#pragma unroll
            for (int nb = 0; nb < kNB; ++nb) pc[nb] = pf[u][nb];
            fetch(pf[u], step + u + kPF);
            one_step(step + u, pc);
        }
    }
#pragma unroll
    for (int u = 0; u < kPF - 1; ++u)
        if (step + u < k1) one_step(step + u, pf[u]);
    if (crole == 1 && cell_ok) cell_update(1, k1 - 1);
    if (cell_ok && hc_last != nullptr) {
        hc_last[st] = h;
        hc_last[(int64_t)2 * B * H + st] = c;
    }
}

// gout [S][B][2H], g_hc_last [2][2][B][H] (gradient of hc_last; nullable) -> d_pre, d_hh [S][B][2][4H] (gradients at the inputs of
// fq_ih / fq_hh; only the times of the steps [k0, k1) are written), d_h0 / d_c0 [2][B][H] (nullable), range partials -> gaccs.
// kMaxT: 512 for H <= 128 (the 24 fp64 partial sums of a thread stay in registers), 1024 above (they spill: odd sizes only)
template <int kMaxT>
__global__ __launch_bounds__(kMaxT) void k_lstmq_bwd(const float* __restrict__ gout, const float* __restrict__ g_hc_last, const float* __restrict__ whh,
                                                    const float* __restrict__ pre, const float* __restrict__ hsav, const float* __restrict__ csav,
                                                    const float* __restrict__ c0, const LstmqRanges R, const LstmqGaccs G,
                                                    float* __restrict__ d_pre, float* __restrict__ d_hh, float* __restrict__ d_h0,
                                                    float* __restrict__ d_c0, int S, int B, int H, int k0, int k1) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ QRange qr[kNQ];
    __shared__ double red[2 * kNQ * 16];
    float* dgs = smem;                   // [kNB][4H]  d_hh of the step
    float* ps = smem + kNB * 4 * H;      // [4][kNB][H] partial dh_{t-1}
    const int dir = blockIdx.y;
    const int b0 = blockIdx.x * kNB;
    const int tid = threadIdx.x;
    const bool tv = tid < 4 * H;
    const int part = tv ? tid / H : 0, k = tv ? tid - part * H : 0;
    const float* Wc = whh + ((int64_t)dir * 4 * H + part * H) * H + k;   // column k of gate block `part`, row stride H
    load_ranges(qr, R, dir);
    for (int e = tid; e < 4 * kNB * H; e += blockDim.x) ps[e] = 0.f;
    for (int e = tid; e < kNB * 4 * H; e += blockDim.x) dgs[e] = 0.f;      // (an absent second sequence contributes zeros)
    const int cn = tid / H, ck = tid - cn * H;
    const bool cell = tid < kNB * H && (b0 + cn) < B;
    const int64_t st = cell ? ((int64_t)dir * B + b0 + cn) * H + ck : 0;   // this thread's element of a [2][B][H] state
    float dc_rec = (cell && g_hc_last != nullptr) ? g_hc_last[(int64_t)2 * B * H + st] : 0.f;
    double du[kNQ], po[kNQ];
#pragma unroll
    for (int i = 0; i < kNQ; ++i) du[i] = po[i] = 0.0;
    __syncthreads();
    for (int step = k1 - 1; step >= k0; --step) {
        const int t = dir == 0 ? step : S - 1 - step;
        if (cell) {
            const int64_t sb = (int64_t)t * B + b0 + cn;
            const int64_t g4 = (sb * 2 + dir) * 4 * H + ck;
            float c_prev;
            if (step > k0) {
                const int tp = dir == 0 ? step - 1 : S - step;
                c_prev = csav[(((int64_t)tp * B + b0 + cn) * 2 + dir) * H + ck];
            } else {
                c_prev = c0 != nullptr ? c0[st] : 0.f;
            }
            // the forward's values again: same functions, same inputs, same bits
            float p[4], hr[4], sum[4], a[4], aq[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                p[r] = pre[g4 + r * H];
                hr[r] = hsav[g4 + r * H];
                a[r] = gate_fn(gate_arg(p[r], hr[r], qr, sum[r]), r == 2);
                aq[r] = fq(a[r], qr[gate_q(r)]);
            }
            const CellVals v = cell_fwd(aq[0], aq[1], aq[2], aq[3], c_prev, qr);
            // dL/dh of this step: the output's gradient + the recurrent part (the four gate blocks' partial products; at the last step
            // of the launch the gradient of the carried state instead)
            const float rec = step == k1 - 1 ? (g_hc_last != nullptr ? g_hc_last[st] : 0.f)
                                             : ((ps[(0 * kNB + cn) * H + ck] + ps[(1 * kNB + cn) * H + ck]) +
                                                (ps[(2 * kNB + cn) * H + ck] + ps[(3 * kNB + cn) * H + ck]));
            const float dh = gout[sb * 2 * H + dir * H + ck] + rec;
            const float d_xh = ste(v.xh, dh, qr[Q_MUL2], du[Q_MUL2], po[Q_MUL2]);
            const float d_th = ste(v.th, d_xh * aq[3], qr[Q_TANH1], du[Q_TANH1], po[Q_TANH1]);
            const float dc = dc_rec + d_th * (1.0f - v.th * v.th);
            const float d_xs = ste(v.xs, dc, qr[Q_ADD1], du[Q_ADD1], po[Q_ADD1]);
            const float d_x0 = ste(v.x0, d_xs, qr[Q_MUL0], du[Q_MUL0], po[Q_MUL0]);
            const float d_x1 = ste(v.x1, d_xs, qr[Q_MUL1], du[Q_MUL1], po[Q_MUL1]);
            dc_rec = d_x0 * aq[1];
            const float dq[4] = {d_x1 * aq[2], d_x0 * c_prev, d_x1 * aq[0], d_xh * v.tq};      // i, f, g, o
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qi = gate_q(r);
                const float d_a = ste(a[r], dq[r], qr[qi], du[qi], po[qi]);
                const float d_s = r == 2 ? d_a * (1.0f - a[r] * a[r]) : (d_a * (1.0f - a[r])) * a[r];
                const float d_sum = ste(sum[r], d_s, qr[Q_ADD0], du[Q_ADD0], po[Q_ADD0]);
                const float dp = ste(p[r], d_sum, qr[Q_IH], du[Q_IH], po[Q_IH]);
                const float dhh = ste(hr[r], d_sum, qr[Q_HH], du[Q_HH], po[Q_HH]);
                d_pre[g4 + r * H] = dp;
                d_hh[g4 + r * H] = dhh;
                dgs[cn * 4 * H + r * H + ck] = dhh;
            }
        }
        __syncthreads();
        if (tv) {
            float acc[kNB];
#pragma unroll
            for (int nb = 0; nb < kNB; ++nb) acc[nb] = 0.f;
            for (int r = 0; r < H; ++r) {
                const float wv = Wc[(int64_t)r * H];
#pragma unroll
                for (int nb = 0; nb < kNB; ++nb) acc[nb] = fmaf(wv, dgs[nb * 4 * H + part * H + r], acc[nb]);
            }
#pragma unroll
            for (int nb = 0; nb < kNB; ++nb) ps[(part * kNB + nb) * H + k] = acc[nb];
        }
        __syncthreads();
    }
    if (cell) {
        if (d_h0 != nullptr)
            d_h0[st] = (ps[(0 * kNB + cn) * H + ck] + ps[(1 * kNB + cn) * H + ck]) + (ps[(2 * kNB + cn) * H + ck] + ps[(3 * kNB + cn) * H + ck]);
        if (d_c0 != nullptr) d_c0[st] = dc_rec;
    }
    // range partials: fp64 per thread -> per workgroup -> this workgroup's own slot of each quantizer ("+=": launches of one backward
    // follow each other on the stream).  Both directions add into the forward direction's mul2 array, in different slots.  More than
    // FQSS_GACC_SLOTS workgroups (over 2048 sequences) fold onto the slots with fp64 atomics: exact enough, no longer order-free.
    double v[2 * kNQ];
#pragma unroll
    for (int i = 0; i < kNQ; ++i) {
        v[2 * i] = du[i];
        v[2 * i + 1] = po[i];
    }
    block_sum<double, 2 * kNQ>(v, red);
    if (tid == 0) {
        const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        const bool fold = (int64_t)gridDim.x * gridDim.y > FQSS_GACC_SLOTS;
        for (int i = 0; i < kNQ; ++i) {
            double* slot = G.p[i == Q_MUL2 ? 0 : dir][i] + 3 * (wg % FQSS_GACC_SLOTS);
            const double dmax = v[2 * i] / 255.0;
            if (fold) {
                atomicAdd(slot, v[2 * i + 1] - dmax);
                atomicAdd(slot + 1, dmax);
            } else {
                slot[0] += v[2 * i + 1] - dmax;
                slot[1] += dmax;
            }
        }
    }
}

}  // namespace
}  // namespace fqss

using namespace fqss;

static int lstmq_ranges(const char* who, const float* const* ranges, LstmqRanges& R) {
    for (int d = 0; d < 2; ++d)
        for (int i = 0; i < kNQ; ++i)
            for (int m = 0; m < 2; ++m) {
                const float* p = ranges[(d * kNQ + i) * 2 + m];
                if (d == 1 && i == Q_MUL2) p = ranges[(0 * kNQ + Q_MUL2) * 2 + m];      // never read from the reverse slot
                if (p == nullptr) { set_error("%s: null range (2 x 12 quantizers: min, max each)", who); return FQSS_EINVAL; }
                R.p[d][i][m] = p;
            }
    return FQSS_OK;
}

static int lstmq_fwd_impl(const char* who, bool generic, const float* pre, const float* whh, const float* bhh, const float* h0, const float* c0,
                          const float* const* ranges, float* hout, float* hc_last, float* hsav, float* csav, int S, int B, int H, int k0,
                          int k1, fqss_stream_t stream) {
    // (not FQSS_REQUIRE: the message has to name the entry the caller used)
#define LSTMQ_NEED(cond, msg) do { if (!(cond)) { set_error("%s: %s", who, msg); return FQSS_EINVAL; } } while (0)
    LSTMQ_NEED(pre && whh && bhh && ranges && hout && ((hsav == nullptr) == (csav == nullptr)), "null tensor (hsav / csav: both or neither)");
    LSTMQ_NEED((h0 == nullptr) == (c0 == nullptr), "h0 / c0: both or neither");
    LSTMQ_NEED(S > 0 && B > 0 && H > 0 && H <= 256, "bad shape (H <= 256)");
    LSTMQ_NEED(0 <= k0 && k0 < k1 && k1 <= S, "bad step range (0 <= k0 < k1 <= S)");
#undef LSTMQ_NEED
    LstmqRanges R;
    if (int e = lstmq_ranges(who, ranges, R)) return e;
    const dim3 grid((unsigned)cdiv(B, kNB), 2);
    if (H == 128 && !generic) {
        const size_t lds2 = (size_t)(kNB * 4 * (H / 4 + 4) + kNB * 4 * H) * sizeof(float);
        hipLaunchKernelGGL(k_lstmq_fwd_st<128>, grid, dim3(512), lds2, (hipStream_t)stream, pre, whh, bhh, h0, c0, R, hout, hc_last, hsav, csav, S,
                           B, k0, k1);
    } else {
        const size_t lds = (size_t)(kNB * (H + 16) + kNB * 4 * H) * sizeof(float);
        const int threads = (int)cdiv(4 * H, 64) * 64;
        hipLaunchKernelGGL(k_lstmq_fwd, grid, dim3(threads), lds, (hipStream_t)stream, pre, whh, bhh, h0, c0, R, hout, hc_last, hsav, csav, S, B,
                           H, k0, k1);
    }
    return launch_status(who);
}

extern "C" int fqss_lstmq_fwd(const float* pre, const float* whh, const float* bhh, const float* h0, const float* c0,
                              const float* const* ranges, float* hout, float* hc_last, float* hsav, float* csav, int S, int B, int H,
                              int k0, int k1, fqss_stream_t stream) {
    return lstmq_fwd_impl("fqss_lstmq_fwd", false, pre, whh, bhh, h0, c0, ranges, hout, hc_last, hsav, csav, S, B, H, k0, k1, stream);
}

// test hook: the same call on the generic kernel at every H, so that the register-resident H = 128 form can be held against it
extern "C" int fqss_lstmq_fwd_generic(const float* pre, const float* whh, const float* bhh, const float* h0, const float* c0,
                                      const float* const* ranges, float* hout, float* hc_last, float* hsav, float* csav, int S, int B, int H,
                                      int k0, int k1, fqss_stream_t stream) {
    return lstmq_fwd_impl("fqss_lstmq_fwd_generic", true, pre, whh, bhh, h0, c0, ranges, hout, hc_last, hsav, csav, S, B, H, k0, k1, stream);
}

extern "C" int fqss_lstmq_bwd(const float* gout, const float* g_hc_last, const float* whh, const float* pre, const float* hsav,
                              const float* csav, const float* c0, const float* const* ranges, double* const* gaccs, float* d_pre,
                              float* d_hh, float* d_h0, float* d_c0, int S, int B, int H, int k0, int k1, fqss_stream_t stream) {
    FQSS_REQUIRE(gout && whh && pre && hsav && csav && ranges && gaccs && d_pre && d_hh, "null tensor");
    FQSS_REQUIRE(S > 0 && B > 0 && H > 0 && H <= 256, "bad shape (H <= 256)");
    FQSS_REQUIRE(0 <= k0 && k0 < k1 && k1 <= S, "bad step range (0 <= k0 < k1 <= S)");
    LstmqRanges R;
    if (int e = lstmq_ranges("fqss_lstmq_bwd", ranges, R)) return e;
    LstmqGaccs G;
    for (int d = 0; d < 2; ++d)
        for (int i = 0; i < kNQ; ++i) {
            double* p = gaccs[d * kNQ + i];
            if (d == 1 && i == Q_MUL2) p = gaccs[Q_MUL2];       // never written through the reverse slot
            FQSS_REQUIRE(p, "null gacc (2 x 12 quantizers)");
            G.p[d][i] = p;
        }
    const dim3 grid((unsigned)cdiv(B, kNB), 2);
    const size_t lds = (size_t)(kNB * 4 * H + 4 * kNB * H) * sizeof(float);
    const int threads = (int)cdiv(4 * H, 64) * 64;
    if (threads <= 512)
        hipLaunchKernelGGL(k_lstmq_bwd<512>, grid, dim3(threads), lds, (hipStream_t)stream, gout, g_hc_last, whh, pre, hsav, csav, c0, R, G, d_pre,
                           d_hh, d_h0, d_c0, S, B, H, k0, k1);
    else
        hipLaunchKernelGGL(k_lstmq_bwd<1024>, grid, dim3(threads), lds, (hipStream_t)stream, gout, g_hc_last, whh, pre, hsav, csav, c0, R, G, d_pre,
                           d_hh, d_h0, d_c0, S, B, H, k0, k1);
    return launch_status("fqss_lstmq_bwd");
}
