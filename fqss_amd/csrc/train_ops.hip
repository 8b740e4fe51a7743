// train_ops.hip -- K15/K16: the scalar end of the step.
//   kd_loss    SDR-weighted knowledge-distillation loss with 2-speaker PIT, forward AND backward:
//              one streaming pass accumulates the 24 second-order moments of (est, teacher, target)
//              per sample in fp64, a one-block kernel does PIT / weights / loss / gradient
//              coefficients, one streaming pass writes dL/d est.
//   kd_loss_n  the same sequence for 1 to 3 sources (k_kd_moments_n<S>, k_kd_final_n<S>, k_kd_grad_n): 6S + 3S^2 moments,
//              PIT over the S! permutations in itertools order.  Two sources keep the kernels above.
//   sumsq + adam_clip   global-norm clip and Adam over ONE flat fp32 parameter buffer.
//   optim_clip          the same clip and clocks with Adam + L2, AdamW or SGD momentum behind them (k_optim_clip<KIND, W>).
//   ema_update          EMA copies of that buffer (demucs' ModelEMA), the weight read from a device-resident count.
//
// Reference replaced: System.common_step (mysystem.py:124-151), PairwiseWSDR (wsdr.py:56-95),
// asteroid PITLossWrapper("pw_mtx") for n_src=2 (third-party, restated in oracle/fqss_oracle.py),
// pl gradient_clip_val=5.0 + torch.optim.Adam (asteroid_librimix_trainer.py:94,132).
#include <vector>

#include "fqss_dev.h"

namespace fqss {

constexpr double kEps = 1e-8;
constexpr int kNMom = 24;
constexpr int kStatStride = 32;
// moment slots per sample. signals: e0 e1 (student) f0 f1 (teacher) t0 t1 (targets)
//  0..5   sums            S[e0,e1,f0,f1,t0,t1]
//  6..11  self products   ee0 ee1 ff0 ff1 tt0 tt1
// 12..15  e_i.t_j  (i*2+j)      16..19  e_i.f_j      20..23  f_i.t_j

__global__ __launch_bounds__(256) void k_kd_moments(const float* __restrict__ est, const float* __restrict__ fest,
                                                     const float* __restrict__ tgt, int64_t T, double* stats) {
    __shared__ double red[kNMom * 4];
    const int b = blockIdx.y;
    const float* e0 = est + (int64_t)b * 2 * T;
    const float* f0 = fest + (int64_t)b * 2 * T;
    const float* t0 = tgt + (int64_t)b * 2 * T;
    double a[kNMom];
#pragma unroll
    for (int i = 0; i < kNMom; ++i) a[i] = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < T; t += (int64_t)gridDim.x * 256) {
        const double s[6] = {(double)e0[t], (double)e0[T + t], (double)f0[t], (double)f0[T + t], (double)t0[t], (double)t0[T + t]};
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            a[i] += s[i];
            a[6 + i] += s[i] * s[i];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                a[12 + i * 2 + j] += s[i] * s[4 + j];
                a[16 + i * 2 + j] += s[i] * s[2 + j];
                a[20 + i * 2 + j] += s[2 + i] * s[4 + j];
            }
    }
    block_sum<double, kNMom>(a, red);
    if (threadIdx.x == 0)
        for (int i = 0; i < kNMom; ++i) atomicAdd(&stats[(int64_t)b * kStatStride + i], a[i]);
}

struct PairSdr {
    double sdr;      // ||proj||^2 / (||noise||^2 + eps)
    double cx, cy;   // d sdr / d x~ = cx * x~ + cy * y~   (x~, y~ zero-mean)
};

// x: estimate, y: reference; raw moments over T samples (wsdr.py:63-89 with sdr_type='sisdr')
__device__ PairSdr pair_sdr(double Sx, double Sy, double Sxx, double Syy, double Sxy, double T) {
    const double X2 = Sxx - Sx * Sx / T, Y2 = Syy - Sy * Sy / T, D = Sxy - Sx * Sy / T;
    const double E = Y2 + kEps;
    const double alpha = D / E;
    const double P = alpha * alpha * Y2;
    double Nn = X2 - 2.0 * alpha * D + alpha * alpha * Y2;
    if (Nn < 0.0) Nn = 0.0;
    const double den = Nn + kEps;
    PairSdr r;
    r.sdr = P / den;
    r.cx = -2.0 * P / (den * den);
    r.cy = 2.0 * alpha * Y2 / (E * den) + P * (2.0 * alpha + 2.0 * D * kEps / (E * E)) / (den * den);
    return r;
}

// one block; thread b < B handles sample b. coef[b][i][8] = {A, Bt, jt, Bf, jf, mean_e, -, -}, means[b][6]
// per_sample = 0: the asteroid objective (mysystem.py:124-151): -10 log10 of the batch MEANS of the task / KD ratios.
// per_sample = 1: the speechbrain objective (speechbrain_librimix_trainer.py:99-115, 141-149; wsdr.py PitWrapper over cal_w_si_snr):
//   loss_b = -10 log10((1-lam) task_b + lam kd_b + eps) per sample, then the mean over the samples with loss_b > threshold (all of
//   them when none is above, or when the threshold is off).  The KD weights follow the reference's broadcast `si_snr[1, C, C] *
//   weights[1, B]`: at B = 1 the sample's w, at B = 2 (= n_src) the weight of STUDENT SOURCE j is w[j], in both samples (the host refuses
//   B > 2, where that broadcast raises).  The reference projects the teacher / target on the student there (roles swapped): the ratio
//   is symmetric up to eps / energy ~ 1e-11, the same pair_sdr serves both.
// per_sample = 2: the teacher-free loss of kd_lambda = 0 (mysystem.py:153-156: asteroid's PITLossWrapper(pairwise_neg_sisdr), restated in
//   oracle/fqss_oracle.py::neg_sisdr_pit): mean_b min_perm mean_src -10 log10(sdr(e_p(i), t_i) + eps); the teacher slots are ignored.
__global__ __launch_bounds__(1024) void k_kd_final(int B, int64_t T, float kd_lambda, double* stats, float* out,
                                                    float* w_out, float* sisdr_out, int per_sample, int use_threshold, float threshold) {
    __shared__ double red[2 * 16];
    __shared__ double sh_w[2];
    __shared__ int sh_keep;
    const int b = threadIdx.x;
    const double Td = (double)T;
    double task_b = 0.0, kd_b = 0.0, wb = 0.0, pit_db = 0.0;
    int pt = 0, pf = 0;  // selected permutation (0: identity, 1: swapped) for task / kd
    PairSdr st[2][2], sf[2][2];
    if (b < B) {
        const double* m = stats + (int64_t)b * kStatStride;
        double neg_log_ft[2][2], neg_log_et[2][2];
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) {
                st[i][j] = pair_sdr(m[i], m[4 + j], m[6 + i], m[10 + j], m[12 + i * 2 + j], Td);        // e_i vs t_j
                sf[i][j] = pair_sdr(m[i], m[2 + j], m[6 + i], m[8 + j], m[16 + i * 2 + j], Td);         // e_i vs f_j
                const PairSdr ft = pair_sdr(m[2 + i], m[4 + j], m[8 + i], m[10 + j], m[20 + i * 2 + j], Td);  // f_i vs t_j
                neg_log_ft[i][j] = -10.0 * log10(ft.sdr + kEps);
                neg_log_et[i][j] = -10.0 * log10(st[i][j].sdr + kEps);
            }
        // PIT (pw_mtx): loss_p = mean_i pw[est=p[i]][tgt=i]; p0 = (0,1), p1 = (1,0); torch.min keeps the first on ties
        const double lf0 = 0.5 * (neg_log_ft[0][0] + neg_log_ft[1][1]), lf1 = 0.5 * (neg_log_ft[1][0] + neg_log_ft[0][1]);
        const double le0 = 0.5 * (neg_log_et[0][0] + neg_log_et[1][1]), le1 = 0.5 * (neg_log_et[1][0] + neg_log_et[0][1]);
        const double sdrs = lf1 < lf0 ? lf1 : lf0, sdrqs = le1 < le0 ? le1 : le0;
        wb = pow(10.0, (sdrs - sdrqs) / 10.0);  // w = SDR_student / SDR_teacher (mysystem.py:141)
        // task / kd use the NEGATED linear ratio through the same PIT (min of negatives = max of ratios)
        const double t0 = -0.5 * (st[0][0].sdr + st[1][1].sdr), t1 = -0.5 * (st[1][0].sdr + st[0][1].sdr);
        pt = t1 < t0 ? 1 : 0;
        task_b = -(pt ? t1 : t0);
        if (per_sample == 2) {      // the PIT runs over the mean of the dB values here, not over the mean ratio
            pt = le1 < le0 ? 1 : 0;
            pit_db = pt ? le1 : le0;
        }
        w_out[b] = (float)wb;
        sisdr_out[b] = (float)(-sdrqs);
        if (per_sample == 1 && b < 2) sh_w[b] = wb;
    }
    if (per_sample == 1) {
        if (threadIdx.x == 0) sh_keep = 0;
        __syncthreads();
    }
    double wsrc[2] = {wb, wb};      // KD weight of student source 0 / 1 in this sample
    if (per_sample == 1 && B == 2) {
        wsrc[0] = sh_w[0];
        wsrc[1] = sh_w[1];
    }
    if (b < B) {
        const double k0 = -0.5 * (wsrc[0] * sf[0][0].sdr + wsrc[1] * sf[1][1].sdr);
        const double k1 = -0.5 * (wsrc[1] * sf[1][0].sdr + wsrc[0] * sf[0][1].sdr);
        pf = k1 < k0 ? 1 : 0;
        kd_b = -(pf ? k1 : k0);
    }
    double v[2] = {task_b, kd_b};
    block_sum<double, 2>(v, red);
    __shared__ double sh_task, sh_kd;
    if (threadIdx.x == 0) {
        sh_task = v[0] / (double)B;
        sh_kd = v[1] / (double)B;
    }
    __syncthreads();
    const double task = sh_task, kd = sh_kd;
    const double lam = (double)kd_lambda;
    double gt = 0.0, gk[2] = {0.0, 0.0};     // d loss / d (task ratio of a pair), d loss / d (kd ratio of student source j's pair)
    double gti[2] = {0.0, 0.0};              // mode 2: d loss / d (ratio of the pair of estimate i): the log is taken per pair
    if (per_sample == 2) {
        double lv[2] = {(b < B) ? pit_db : 0.0, 0.0};
        block_sum<double, 2>(lv, red);
        if (threadIdx.x == 0) {
            out[0] = (float)(lv[0] / (double)B);
            out[1] = 0.0f;
            out[2] = (float)task;
            out[3] = 0.0f;
        }
        if (b < B)
            for (int i = 0; i < 2; ++i) {
                const int jt = pt ? 1 - i : i;
                gti[i] = -10.0 / (log(10.0) * (st[i][jt].sdr + kEps)) * 0.5 / (double)B;
            }
    } else if (!per_sample) {
        const double arg = (1.0 - lam) * task + lam * kd + kEps;
        if (threadIdx.x == 0) {
            out[0] = (float)(-10.0 * log10(arg));
            out[1] = (float)(-10.0 * log10(kd + kEps));
            out[2] = (float)task;
            out[3] = (float)kd;
        }
        // dL/d arg = -10/(ln10 * arg); d arg/d sdr_task(b, pair) = (1-lam)/(2B); d arg/d sdr_kd = lam*w_b/(2B)
        const double dL = -10.0 / (log(10.0) * arg);
        gt = dL * (1.0 - lam) / (2.0 * (double)B);
        gk[0] = gk[1] = dL * lam * wb / (2.0 * (double)B);
    } else {
        const double arg_b = (1.0 - lam) * task_b + lam * kd_b + kEps;
        const double loss_b = (b < B) ? -10.0 * log10(arg_b) : 0.0;
        const bool above = (b < B) && (!use_threshold || loss_b > (double)threshold);
        if (above) atomicAdd(&sh_keep, 1);
        __syncthreads();
        const int nkeep = sh_keep;
        const bool keep = (b < B) && (nkeep == 0 || above);       // nothing above the threshold: the loss stays as it is (:146-147)
        const double cnt = (double)(nkeep == 0 ? B : nkeep);
        double lv[2] = {keep ? loss_b : 0.0, 0.0};
        block_sum<double, 2>(lv, red);
        if (threadIdx.x == 0) {
            out[0] = (float)(lv[0] / cnt);
            out[1] = (float)(-10.0 * log10(kd + kEps));
            out[2] = (float)task;
            out[3] = (float)kd;
        }
        if (keep) {
            const double dL = -10.0 / (log(10.0) * arg_b) / cnt;
            gt = dL * (1.0 - lam) / 2.0;
            gk[0] = dL * lam * wsrc[0] / 2.0;
            gk[1] = dL * lam * wsrc[1] / 2.0;
        }
    }
    if (b < B) {
        double* m = stats + (int64_t)b * kStatStride;
        double cf[2][5];
        for (int i = 0; i < 2; ++i) {
            // target index paired with estimate i: perm p has est p[j] on tgt j -> est i sits on tgt j with p[j]==i
            const int jt = pt ? 1 - i : i, jf = pf ? 1 - i : i;
            const double gti_ = (per_sample == 2) ? gti[i] : gt;
            cf[i][0] = gti_ * st[i][jt].cx + gk[i] * sf[i][jf].cx;  // coefficient of e~_i
            cf[i][1] = gti_ * st[i][jt].cy;                         // coefficient of t~_jt
            cf[i][2] = (double)jt;
            cf[i][3] = gk[i] * sf[i][jf].cy;                      // coefficient of f~_jf
            cf[i][4] = (double)jf;
        }
        // means for the zero-mean views, then the coefficient table (overwrites the moment slots)
        double mean[6];
        for (int i = 0; i < 6; ++i) mean[i] = m[i] / Td;
        for (int i = 0; i < 6; ++i) m[i] = mean[i];
        for (int i = 0; i < 2; ++i)
            for (int k = 0; k < 5; ++k) m[8 + i * 8 + k] = cf[i][k];
    }
}

// gest[b][i][t] = A*(e_i - mean) + Bt*(t_jt - mean) + Bf*(f_jf - mean)
__global__ __launch_bounds__(256) void k_kd_grad(const float* __restrict__ est, const float* __restrict__ fest,
                                                  const float* __restrict__ tgt, int64_t T, const double* stats,
                                                  float* __restrict__ gest) {
    const int b = blockIdx.y >> 1, i = blockIdx.y & 1;
    const double* m = stats + (int64_t)b * kStatStride;
    const double* cf = m + 8 + i * 8;
    const int jt = (int)cf[2], jf = (int)cf[4];
    const float A = (float)cf[0], Bt = (float)cf[1], Bf = (float)cf[3];
    const float me = (float)m[i], mt = (float)m[4 + jt], mf = (float)m[2 + jf];
    const float* e = est + ((int64_t)b * 2 + i) * T;
    const float* tt = tgt + ((int64_t)b * 2 + jt) * T;
    const float* ff = fest + ((int64_t)b * 2 + jf) * T;
    float* g = gest + ((int64_t)b * 2 + i) * T;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < T; t += (int64_t)gridDim.x * 256)
        g[t] = A * (e[t] - me) + Bt * (tt[t] - mt) + Bf * (ff[t] - mf);
}

// =============================================================================================
// The same three-kernel sequence for S = 1..3 sources (fqss_kd_loss_n / fqss_kd_moments_n).  The two-source kernels above stay as
// they are; S = 2 is instantiated here only so that the tests can hold this code against them.
// stats row of one sample (FQSS_KD_STATS_STRIDE_N doubles; signals e_0.. (student) f_0.. (teacher) t_0.. (targets)):
//   [0, 3S) sums   [3S, 6S) self products   6S + i*S + j: e_i.t_j   6S + S^2 + i*S + j: e_i.f_j   6S + 2S^2 + i*S + j: f_i.t_j
//   (6S + 3S^2 moments: 9 / 24 / 45; at S = 2 these are the slots of k_kd_moments).  The moments stay where they are; k_kd_final_n adds
//   [48, 48 + 3S) the means and 57 + 5i + {0..4} = {A, Bt, jt, Bf, jf} of estimate i for k_kd_grad_n.
constexpr int kStatStrideN = FQSS_KD_STATS_STRIDE_N;
constexpr int kMeanSlotN = 48, kCoefSlotN = 57;
static_assert(6 * 3 + 3 * 3 * 3 <= kMeanSlotN && kMeanSlotN + 3 * 3 <= kCoefSlotN && kCoefSlotN + 5 * 3 <= kStatStrideN, "stats row at S = 3");

template <int S>
__global__ __launch_bounds__(256) void k_kd_moments_n(const float* __restrict__ est, const float* __restrict__ fest,
                                                       const float* __restrict__ tgt, int64_t T, double* stats) {
    constexpr int NM = 6 * S + 3 * S * S;
    __shared__ double red[NM * 4];
    const int b = blockIdx.y;
    const float* e0 = est + (int64_t)b * S * T;
    const float* f0 = fest + (int64_t)b * S * T;
    const float* t0 = tgt + (int64_t)b * S * T;
    double a[NM];
#pragma unroll
    for (int i = 0; i < NM; ++i) a[i] = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < T; t += (int64_t)gridDim.x * 256) {
        double s[3 * S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            s[i] = (double)e0[(int64_t)i * T + t];
            s[S + i] = (double)f0[(int64_t)i * T + t];
            s[2 * S + i] = (double)t0[(int64_t)i * T + t];
        }
#pragma unroll
        for (int i = 0; i < 3 * S; ++i) {
            a[i] += s[i];
            a[3 * S + i] += s[i] * s[i];
        }
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
            for (int j = 0; j < S; ++j) {
                a[6 * S + i * S + j] += s[i] * s[2 * S + j];
                a[6 * S + S * S + i * S + j] += s[i] * s[S + j];
                a[6 * S + 2 * S * S + i * S + j] += s[S + i] * s[2 * S + j];
            }
    }
    block_sum<double, NM>(a, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NM; ++i) atomicAdd(&stats[(int64_t)b * kStatStrideN + i], a[i]);
    }
}

// permutation q of itertools.permutations(range(S)), element i -- as arithmetic, so that no table is indexed at run time.
// S = 3: the first element is q / 2, the other two follow ascending (q even) or descending (q odd).
template <int S>
__device__ __forceinline__ int perm_at(int q, int i) {
    if (S == 1) return 0;
    if (S == 2) return q ? 1 - i : i;
    const int first = q >> 1, r0 = first == 0 ? 1 : 0, r1 = first == 2 ? 1 : 2;
    return i == 0 ? first : ((i == 1) != ((q & 1) != 0) ? r0 : r1);
}
// the position j with perm(q)[j] == i: the signal that estimate i is paired with under permutation q (the inverse map)
template <int S>
__device__ __forceinline__ int perm_inv(int q, int i) {
    int j = 0;
#pragma unroll
    for (int k = 1; k < S; ++k)
        if (perm_at<S>(q, k) == i) j = k;
    return j;
}

// one block; thread b < B handles sample b.  mode 0 / 1 / 2 = per_sample 0 / 1 / 2 of k_kd_final.  Every PIT candidate pairs the
// student's source p[i] with signal i of the other side: asteroid's pw_mtx form mean_i pw[est = p[i]][tgt = i] and the speechbrain
// wrapper's mean_i M[other = i][student = p[i]] are that same pairing, and the gradient of estimate i goes to signal p^-1[i].
// Only the S*S ratios are kept per thread; the derivative coefficients of the S selected pairs are recomputed from the moments.
template <int S>
__global__ __launch_bounds__(1024) void k_kd_final_n(int B, int64_t T, float kd_lambda, double* stats, float* out, float* w_out,
                                                      float* sisdr_out, int mode, int use_threshold, float threshold) {
    constexpr int NP = S == 1 ? 1 : (S == 2 ? 2 : 6);
    constexpr int oET = 6 * S, oEF = 6 * S + S * S, oFT = 6 * S + 2 * S * S;
    __shared__ double red[2 * 16];
    __shared__ double sh_w[S];
    __shared__ int sh_keep;
    __shared__ double sh_task, sh_kd;
    const int b = threadIdx.x;
    const double Td = (double)T, invS = 1.0 / (double)S;
    double* m = stats + (int64_t)(b < B ? b : 0) * kStatStrideN;
    double task_b = 0.0, kd_b = 0.0, wb = 0.0, pit_db = 0.0;
    int pt = 0, pf = 0;     // selected permutation for task / kd
    double rf[S][S];        // linear ratio of e_i against f_j
    if (b < B) {
        // four separate reductions over the permutations (at S = 3 they can select different ones); one table at a time, so that
        // no more than two S x S tables are live
        double sdrs = 0.0, sdrqs = 0.0, tbest = 0.0;
        int pe = 0;
        {
            double nl_ft[S][S];     // teacher vs target, dB
#pragma unroll
            for (int i = 0; i < S; ++i)
#pragma unroll
                for (int j = 0; j < S; ++j)
                    nl_ft[i][j] = -10.0 * log10(pair_sdr(m[S + i], m[2 * S + j], m[4 * S + i], m[5 * S + j], m[oFT + i * S + j], Td).sdr + kEps);
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                double lf = 0.0;
#pragma unroll
                for (int i = 0; i < S; ++i) lf += nl_ft[perm_at<S>(q, i)][i];
                lf *= invS;
                if (q == 0 || lf < sdrs) sdrs = lf;
            }
        }
        {
            double rt[S][S];        // student vs target, linear ratio
#pragma unroll
            for (int i = 0; i < S; ++i)
#pragma unroll
                for (int j = 0; j < S; ++j) rt[i][j] = pair_sdr(m[i], m[2 * S + j], m[3 * S + i], m[5 * S + j], m[oET + i * S + j], Td).sdr;
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                double le = 0.0, tq = 0.0;
#pragma unroll
                for (int i = 0; i < S; ++i) {
                    le += -10.0 * log10(rt[perm_at<S>(q, i)][i] + kEps);
                    tq += rt[perm_at<S>(q, i)][i];
                }
                le *= invS;
                tq = -tq * invS;    // task / kd use the NEGATED linear ratio through the same PIT
                if (q == 0 || le < sdrqs) {
                    sdrqs = le;
                    pe = q;
                }
                if (q == 0 || tq < tbest) {
                    tbest = tq;
                    pt = q;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
            for (int j = 0; j < S; ++j) rf[i][j] = pair_sdr(m[i], m[S + j], m[3 * S + i], m[4 * S + j], m[oEF + i * S + j], Td).sdr;
        wb = pow(10.0, (sdrs - sdrqs) / 10.0);  // w = SDR_student / SDR_teacher (mysystem.py:141)
        task_b = -tbest;
        if (mode == 2) {    // the PIT runs over the mean of the dB values here, not over the mean ratio
            pt = pe;
            pit_db = sdrqs;
        }
        w_out[b] = (float)wb;
        sisdr_out[b] = (float)(-sdrqs);
        if (mode == 1 && b < S) sh_w[b] = wb;
    }
    if (mode == 1) {
        if (threadIdx.x == 0) sh_keep = 0;
        __syncthreads();
    }
    double wsrc[S];         // KD weight of student source j in this sample
#pragma unroll
    for (int j = 0; j < S; ++j) wsrc[j] = (mode == 1 && B == S) ? sh_w[j] : wb;
    if (b < B) {
        double kbest = 0.0;
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            double kq = 0.0;
#pragma unroll
            for (int i = 0; i < S; ++i) kq += wsrc[perm_at<S>(q, i)] * rf[perm_at<S>(q, i)][i];
            kq = -kq * invS;
            if (q == 0 || kq < kbest) {
                kbest = kq;
                pf = q;
            }
        }
        kd_b = -kbest;
    }
    double v[2] = {task_b, kd_b};
    block_sum<double, 2>(v, red);
    if (threadIdx.x == 0) {
        sh_task = v[0] / (double)B;
        sh_kd = v[1] / (double)B;
    }
    __syncthreads();
    const double task = sh_task, kd = sh_kd;
    const double lam = (double)kd_lambda;
    // d loss / d (task ratio of a pair), d loss / d (kd ratio of student source j's pair); spelled so that at S = 2 every product
    // rounds as in k_kd_final (invS = 0.5 is exact)
    double gt = 0.0, gk[S];
#pragma unroll
    for (int j = 0; j < S; ++j) gk[j] = 0.0;
    if (mode == 2) {
        double lv[2] = {(b < B) ? pit_db : 0.0, 0.0};
        block_sum<double, 2>(lv, red);
        if (threadIdx.x == 0) {
            out[0] = (float)(lv[0] / (double)B);
            out[1] = 0.0f;
            out[2] = (float)task;
            out[3] = 0.0f;
        }
    } else if (mode == 0) {
        const double arg = (1.0 - lam) * task + lam * kd + kEps;
        if (threadIdx.x == 0) {
            out[0] = (float)(-10.0 * log10(arg));
            out[1] = (float)(-10.0 * log10(kd + kEps));
            out[2] = (float)task;
            out[3] = (float)kd;
        }
        // dL/d arg = -10/(ln10 * arg); d arg/d sdr_task(b, pair) = (1-lam)/(S B); d arg/d sdr_kd = lam*w_b/(S B)
        const double dL = -10.0 / (log(10.0) * arg);
        gt = dL * (1.0 - lam) * invS / (double)B;
#pragma unroll
        for (int j = 0; j < S; ++j) gk[j] = dL * lam * wb * invS / (double)B;
    } else {
        const double arg_b = (1.0 - lam) * task_b + lam * kd_b + kEps;
        const double loss_b = (b < B) ? -10.0 * log10(arg_b) : 0.0;
        const bool above = (b < B) && (!use_threshold || loss_b > (double)threshold);
        if (above) atomicAdd(&sh_keep, 1);
        __syncthreads();
        const int nkeep = sh_keep;
        const bool keep = (b < B) && (nkeep == 0 || above);       // nothing above the threshold: the loss stays as it is
        const double cnt = (double)(nkeep == 0 ? B : nkeep);
        double lv[2] = {keep ? loss_b : 0.0, 0.0};
        block_sum<double, 2>(lv, red);
        if (threadIdx.x == 0) {
            out[0] = (float)(lv[0] / cnt);
            out[1] = (float)(-10.0 * log10(kd + kEps));
            out[2] = (float)task;
            out[3] = (float)kd;
        }
        if (keep) {
            const double dL = -10.0 / (log(10.0) * arg_b) / cnt;
            gt = dL * (1.0 - lam) * invS;
#pragma unroll
            for (int j = 0; j < S; ++j) gk[j] = dL * lam * wsrc[j] * invS;
        }
    }
    if (b < B) {
#pragma unroll
        for (int i = 0; i < S; ++i) {
            // estimate i sits on signal j with p[j] == i: the inverse map, not p[i] (they differ for the 3-cycles)
            const int jt = perm_inv<S>(pt, i), jf = perm_inv<S>(pf, i);
            const PairSdr a = pair_sdr(m[i], m[2 * S + jt], m[3 * S + i], m[5 * S + jt], m[oET + i * S + jt], Td);
            const PairSdr c = pair_sdr(m[i], m[S + jf], m[3 * S + i], m[4 * S + jf], m[oEF + i * S + jf], Td);
            // mode 2: the log is taken per pair, d loss / d (ratio of the pair of estimate i)
            const double gti = (mode == 2) ? -10.0 / (log(10.0) * (a.sdr + kEps)) * invS / (double)B : gt;
            const double gki = gk[i];
            double* cf = m + kCoefSlotN + 5 * i;
            cf[0] = gti * a.cx + gki * c.cx;    // coefficient of e~_i
            cf[1] = gti * a.cy;                 // coefficient of t~_jt
            cf[2] = (double)jt;
            cf[3] = gki * c.cy;                 // coefficient of f~_jf
            cf[4] = (double)jf;
        }
#pragma unroll
        for (int i = 0; i < 3 * S; ++i) m[kMeanSlotN + i] = m[i] / Td;
    }
}

// gest[b][i][t] = A*(e_i - mean) + Bt*(t_jt - mean) + Bf*(f_jf - mean); grid (column blocks, S * B)
__global__ __launch_bounds__(256) void k_kd_grad_n(const float* __restrict__ est, const float* __restrict__ fest,
                                                    const float* __restrict__ tgt, int S, int64_t T, const double* stats,
                                                    float* __restrict__ gest) {
    const int b = blockIdx.y / S, i = blockIdx.y - b * S;
    const double* m = stats + (int64_t)b * kStatStrideN;
    const double* cf = m + kCoefSlotN + 5 * i;
    const int jt = (int)cf[2], jf = (int)cf[4];
    const float A = (float)cf[0], Bt = (float)cf[1], Bf = (float)cf[3];
    const float me = (float)m[kMeanSlotN + i], mt = (float)m[kMeanSlotN + 2 * S + jt], mf = (float)m[kMeanSlotN + S + jf];
    const float* e = est + ((int64_t)b * S + i) * T;
    const float* tt = tgt + ((int64_t)b * S + jt) * T;
    const float* ff = fest + ((int64_t)b * S + jf) * T;
    float* g = gest + ((int64_t)b * S + i) * T;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < T; t += (int64_t)gridDim.x * 256)
        g[t] = A * (e[t] - me) + Bt * (tt[t] - mt) + Bf * (ff[t] - mf);
}

// =============================================================================================
__global__ __launch_bounds__(256) void k_sumsq(const float* __restrict__ g, int64_t n, double* acc) {
    __shared__ double red[4];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = (double)g[i];
        s += v * v;
    }
    double v[1] = {s};
    block_sum<double, 1>(v, red);
    if (threadIdx.x == 0) atomicAdd(acc, v[0]);
}

// torch.optim.Adam single-tensor math (amsgrad=False, weight_decay=0, maximize=False):
//   m.lerp_(g, 1-b1); v.mul_(b2).addcmul_(g, g, 1-b2); denom = sqrt(v)/sqrt(1-b2^t) + eps; p -= (lr/(1-b1^t)) * m/denom
// torch keeps `t` PER PARAMETER and starts it when the parameter first receives a gradient (weights:
// step 1, weight ranges: step 2, activation ranges: step 51, never-used parameters: never touched).
// t0[i] = number of global steps that passed before element i became active (INT_MAX: inactive).
__global__ __launch_bounds__(256) void k_adam_clip(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                    const double* sumsq, float max_norm, float grad_scale, float lr,
                                                    float beta1, float beta2, float eps, const int32_t* step_t,
                                                    const int32_t* __restrict__ t0) {
    const int tg = *step_t + 1;
    const double norm = sqrt(*sumsq) * (double)grad_scale;
    double coef = (double)max_norm / (norm + 1e-6);   // torch.nn.utils.clip_grad_norm_
    if (coef > 1.0) coef = 1.0;
    if (max_norm <= 0.0f) coef = 1.0;
    const float gs = (float)((double)grad_scale * coef);
    const float omb1 = (float)(1.0 - (double)beta1), omb2 = (float)(1.0 - (double)beta2);
    int cached = -1;
    float step_size = 0.0f, bc2_sqrt = 1.0f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int t = tg - (t0 ? t0[i] : 0);
        if (t <= 0) continue;  // parameter has never had a gradient: torch.optim skips it
        if (t != cached) {
            const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
            step_size = (float)((double)lr / bc1);
            bc2_sqrt = (float)sqrt(bc2);
            cached = t;
        }
        const float gi = g[i] * gs;
        const float mi = m[i] + omb1 * (gi - m[i]);
        const float vi = v[i] * beta2 + (omb2 * gi) * gi;   // addcmul: self + value*t1*t2
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] = p[i] + ((-step_size) * mi) / denom;           // addcdiv: self + value*t1/t2
    }
}

// The optimizer family (fqss.h: fqss_optim_clip): torch.optim.Adam with L2 decay, AdamW, SGD with momentum -- the single-tensor paths
// (foreach=False, maximize=False, amsgrad=False, dampening 0), on the clip and the per-element clock of k_adam_clip.
//   Adam   grad = grad.add(param, alpha=wd), then the Adam update above
//   AdamW  param.mul_(1 - lr * wd), then the Adam update on the undecayed gradient
//   SGD    grad = grad.add(param, alpha=wd); buf = clone(grad) on the parameter's first step, else buf.mul_(mu).add_(grad);
//          grad = nesterov ? grad.add(buf, alpha=mu) : buf; param.add_(grad, alpha=-lr)
// Bytes per element: Adam kinds read p, g, m, v, t0 and write p, m, v = 32 B (28 B without t0); SGD with momentum reads p, g, buf, t0
// and writes p, buf = 24 B, without momentum 16 B (+ 4 B t0); the decay table adds 1/16 B.  Nothing is reused, so the kernel is its
// bytes: W = 4 moves them as 16-B accesses (every pointer 16-B aligned; a last group of n % 4 elements goes scalar), W = 1 serves any
// address.  KIND is a template parameter: the SGD body carries neither the bias corrections nor the second moment's registers.
__device__ __forceinline__ void load4(const float* src, float* a) {      // src 16-B aligned, a[0..3]
    const float4 t = *reinterpret_cast<const float4*>(src);
    a[0] = t.x, a[1] = t.y, a[2] = t.z, a[3] = t.w;
}
__device__ __forceinline__ void store4(float* dst, const float* a) {
    *reinterpret_cast<float4*>(dst) = make_float4(a[0], a[1], a[2], a[3]);
}

template <int KIND, int W>
__global__ __launch_bounds__(256) void k_optim_clip(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                     float* __restrict__ v, int64_t n, const double* sumsq, float max_norm,
                                                     float grad_scale, float lr, float beta1, float beta2, float eps,
                                                     const int32_t* step_t, const int32_t* __restrict__ t0, float wd0,
                                                     const float* __restrict__ wd_slot, float mu, int nesterov) {
    constexpr bool kAdam = KIND != FQSS_OPT_SGD;
    const int tg = *step_t + 1;
    const double norm = sqrt(*sumsq) * (double)grad_scale;
    double coef = (double)max_norm / (norm + 1e-6);   // torch.nn.utils.clip_grad_norm_
    if (coef > 1.0) coef = 1.0;
    if (max_norm <= 0.0f) coef = 1.0;
    const float gs = (float)((double)grad_scale * coef);
    const float omb1 = (float)(1.0 - (double)beta1), omb2 = (float)(1.0 - (double)beta2);
    const bool use_buf = !kAdam && mu != 0.0f;
    int cached = -1;
    float step_size = 0.0f, bc2_sqrt = 1.0f;
    float wd_cached = 0.0f, shrink = 1.0f;            // AdamW: 1 - lr * wd of the last decay seen (fp64, rounded once like torch's scalar)
    const int64_t groups = (n + W - 1) / W;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < groups; q += (int64_t)gridDim.x * 256) {
        const int64_t base = q * W;
        const bool whole = W == 1 || base + W <= n;
        const int cnt = whole ? W : (int)(n - base);
        int ta[W];
        float pa[W], ga[W], ma[W], va[W];
        bool vec = false;                   // this group moves as 16-B words
        if constexpr (W == 4) vec = whole;
        if (vec) {
            int4 t4 = make_int4(0, 0, 0, 0);
            if (t0) t4 = *reinterpret_cast<const int4*>(t0 + base);
            const int t0s[4] = {t4.x, t4.y, t4.z, t4.w};
            for (int e = 0; e < W; ++e) ta[e] = tg - t0s[e];
        } else {
            for (int e = 0; e < cnt; ++e) ta[e] = tg - (t0 ? t0[base + e] : 0);
        }
        bool any = false;
        for (int e = 0; e < cnt; ++e) any = any || ta[e] > 0;
        if (!any) continue;   // parameters that never had a gradient: torch.optim skips them, decay included
        if (vec) {
            load4(p + base, pa);
            load4(g + base, ga);
            if (kAdam || use_buf) load4(m + base, ma);
            if (kAdam) load4(v + base, va);
        } else {
            for (int e = 0; e < cnt; ++e) {
                pa[e] = p[base + e];
                ga[e] = g[base + e];
                if (kAdam || use_buf) ma[e] = m[base + e];
                if (kAdam) va[e] = v[base + e];
            }
        }
        const float wd = wd_slot ? wd_slot[base >> 6] : wd0;      // a group of 4 never straddles a 64-float slot
        for (int e = 0; e < cnt; ++e) {
            const int t = ta[e];
            if (t <= 0) continue;                                 // (its loaded bits go back unchanged)
            float gi = ga[e] * gs;
            if (KIND == FQSS_OPT_ADAMW) {
                if (wd != 0.0f) {
                    if (wd != wd_cached) {
                        shrink = (float)(1.0 - (double)lr * (double)wd);
                        wd_cached = wd;
                    }
                    pa[e] = pa[e] * shrink;
                }
            } else if (wd != 0.0f) {
                gi = fmaf(wd, pa[e], gi);        // add(alpha=): one rounding in torch's kernels
            }
            if (kAdam) {
                if (t != cached) {
                    const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
                    step_size = (float)((double)lr / bc1);
                    bc2_sqrt = (float)sqrt(bc2);
                    cached = t;
                }
                const float mi = ma[e] + omb1 * (gi - ma[e]);
                const float vi = va[e] * beta2 + (omb2 * gi) * gi;   // addcmul: self + value*t1*t2
                ma[e] = mi;
                va[e] = vi;
                const float denom = sqrtf(vi) / bc2_sqrt + eps;
                pa[e] = pa[e] + ((-step_size) * mi) / denom;         // addcdiv: self + value*t1/t2
            } else {
                float d = gi;
                if (use_buf) {
                    const float buf = (t == 1) ? gi : ma[e] * mu + gi;
                    ma[e] = buf;
                    d = nesterov ? fmaf(mu, buf, gi) : buf;
                }
                pa[e] = fmaf(-lr, d, pa[e]);
            }
        }
        if (vec) {
            store4(p + base, pa);
            if (kAdam || use_buf) store4(m + base, ma);
            if (kAdam) store4(v + base, va);
        } else {
            for (int e = 0; e < cnt; ++e) {
                if (ta[e] <= 0) continue;
                p[base + e] = pa[e];
                if (kAdam || use_buf) m[base + e] = ma[e];
                if (kAdam) v[base + e] = va[e];
            }
        }
    }
}

// EMA copies of the arena (fqss.h: fqss_ema_update): ema = ema * (1 - w) + w * p, demucs' ModelEMA.update().  count (nullable): the
// device-resident count of the unbiased form; every thread derives the same w from it, k_ema_count_end advances it behind this launch.
template <int W>
__global__ __launch_bounds__(256) void k_ema_update(float* __restrict__ ema, const float* __restrict__ p, int64_t n, float w_host,
                                                     double decay, const double* count) {
    double wd = (double)w_host;
    if (count) wd = 1.0 / (*count * decay + 1.0);
    const float w = (float)wd, omw = (float)(1.0 - wd);
    const int64_t groups = (n + W - 1) / W;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < groups; q += (int64_t)gridDim.x * 256) {
        const int64_t base = q * W;
        if (W == 4 && base + 4 <= n) {
            const float4 a = *reinterpret_cast<const float4*>(ema + base), b = *reinterpret_cast<const float4*>(p + base);
            *reinterpret_cast<float4*>(ema + base) =
                make_float4(a.x * omw + w * b.x, a.y * omw + w * b.y, a.z * omw + w * b.z, a.w * omw + w * b.w);
        } else {
            const int64_t end = base + W < n ? base + W : n;
            for (int64_t i = base; i < end; ++i) ema[i] = ema[i] * omw + w * p[i];
        }
    }
}

__global__ void k_ema_count_end(double* count, double decay) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *count = *count * decay + 1.0;
}

// gradient accumulation (fqss.h: fqss_grad_accum): the four moves between the gradient arena g and the window's accumulator acc.
// Thread i owns float4 i of both: one fp32 add per element, no order to depend on.
template <int MODE>
__global__ __launch_bounds__(256) void k_grad_accum(float4* __restrict__ acc, float4* __restrict__ g, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        if (MODE == 0) {
            acc[i] = g[i];
        } else if (MODE == 3) {
            g[i] = acc[i];
        } else {
            const float4 a = acc[i], b = g[i];
            const float4 s = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
            if (MODE == 1) acc[i] = s;
            else g[i] = s;
        }
    }
}

__global__ void k_step_end(int32_t* step_t, const double* sumsq, float grad_scale, float* gnorm_out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        *step_t = *step_t + 1;
        if (gnorm_out) *gnorm_out = (float)(sqrt(*sumsq) * (double)grad_scale);
    }
}

}  // namespace fqss

using namespace fqss;

static int kd_loss_impl(const char* who, const float* est, const float* fest, const float* tgt, int B, int64_t T, float kd_lambda,
                        double* stats, float* out, float* w_out, float* sisdr_out, float* gest, int per_sample, int use_threshold,
                        float threshold, fqss_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(stats, 0, sizeof(double) * kStatStride * B, s) != hipSuccess) return launch_status(who);
    int64_t nb = cdiv(T, 256 * 8);
    if (nb > 64) nb = 64;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(k_kd_moments, dim3((unsigned)nb, (unsigned)B), dim3(256), 0, s, est, fest, tgt, T, stats);
    hipLaunchKernelGGL(k_kd_final, dim3(1), dim3(1024), 0, s, B, T, kd_lambda, stats, out, w_out, sisdr_out, per_sample, use_threshold,
                       threshold);
    if (gest) {
        int64_t ng = cdiv(T, 256 * 4);
        if (ng > 256) ng = 256;
        hipLaunchKernelGGL(k_kd_grad, dim3((unsigned)ng, (unsigned)(2 * B)), dim3(256), 0, s, est, fest, tgt, T, stats, gest);
    }
    return launch_status(who);
}

extern "C" int fqss_kd_loss(const float* est, const float* fest, const float* tgt, int B, int64_t T, float kd_lambda,
                            double* stats, float* out, float* w_out, float* sisdr_out, float* gest,
                            fqss_stream_t stream) {
    FQSS_REQUIRE(est && fest && tgt && stats && out && w_out && sisdr_out, "null tensor");
    FQSS_REQUIRE(B > 0 && B <= 1024 && T > 0, "B must be in 1..1024");
    return kd_loss_impl("fqss_kd_loss", est, fest, tgt, B, T, kd_lambda, stats, out, w_out, sisdr_out, gest, 0, 0, 0.0f, stream);
}

extern "C" int fqss_kd_loss_per_sample(const float* est, const float* fest, const float* tgt, int B, int64_t T, float kd_lambda,
                                       int use_threshold, float threshold, double* stats, float* out, float* w_out, float* sisdr_out,
                                       float* gest, fqss_stream_t stream) {
    FQSS_REQUIRE(est && fest && tgt && stats && out && w_out && sisdr_out, "null tensor");
    FQSS_REQUIRE(T > 0 && B > 0, "bad shape");
    FQSS_REQUIRE(B <= 2, "the per-sample KD weights broadcast [1, n_src, n_src] * [1, B]: B must be 1 or n_src = 2 (the reference raises otherwise)");
    return kd_loss_impl("fqss_kd_loss_per_sample", est, fest, tgt, B, T, kd_lambda, stats, out, w_out, sisdr_out, gest, 1,
                        use_threshold ? 1 : 0, threshold, stream);
}

extern "C" int fqss_pit_sisdr_loss(const float* est, const float* tgt, int B, int64_t T, double* stats, float* out, float* w_out,
                                   float* sisdr_out, float* gest, fqss_stream_t stream) {
    FQSS_REQUIRE(est && tgt && stats && out && w_out && sisdr_out, "null tensor");
    FQSS_REQUIRE(B > 0 && B <= 1024 && T > 0, "B must be in 1..1024");
    return kd_loss_impl("fqss_pit_sisdr_loss", est, tgt, tgt, B, T, 0.0f, stats, out, w_out, sisdr_out, gest, 2, 0, 0.0f, stream);
}

extern "C" int fqss_kd_moments(const float* est, const float* fest, const float* tgt, int B, int64_t T, double* stats,
                               fqss_stream_t stream) {
    FQSS_REQUIRE(est && fest && tgt && stats, "null tensor");
    FQSS_REQUIRE(B > 0 && T > 0, "bad shape");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(stats, 0, sizeof(double) * kStatStride * B, s) != hipSuccess) return launch_status("fqss_kd_moments(memset)");
    int64_t nb = cdiv(T, 256 * 8);
    if (nb > 64) nb = 64;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(k_kd_moments, dim3((unsigned)nb, (unsigned)B), dim3(256), 0, s, est, fest, tgt, T, stats);
    return launch_status("fqss_kd_moments");
}

// ---- S = 1..3 sources (the kernels templated on S above)
template <int S>
static void kd_launch_n(const float* est, const float* fest, const float* tgt, int B, int64_t T, float kd_lambda, int mode, int use_threshold,
                        float threshold, double* stats, float* out, float* w_out, float* sisdr_out, bool final_pass, hipStream_t s) {
    int64_t nb = cdiv(T, 256 * 8);
    if (nb > 64) nb = 64;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(k_kd_moments_n<S>, dim3((unsigned)nb, (unsigned)B), dim3(256), 0, s, est, fest, tgt, T, stats);
    if (final_pass)
        hipLaunchKernelGGL(k_kd_final_n<S>, dim3(1), dim3(1024), 0, s, B, T, kd_lambda, stats, out, w_out, sisdr_out, mode, use_threshold,
                           threshold);
}

extern "C" int fqss_kd_loss_n(const float* est, const float* fest, const float* tgt, int B, int S, int64_t T, float kd_lambda, int mode,
                              int use_threshold, float threshold, double* stats, float* out, float* w_out, float* sisdr_out, float* gest,
                              fqss_stream_t stream) {
    FQSS_REQUIRE(est && fest && tgt && stats && out && w_out && sisdr_out, "null tensor");
    FQSS_REQUIRE(S >= 1 && S <= 3, "n_src must be in 1..3");
    FQSS_REQUIRE(B > 0 && B <= 1024 && T > 0, "B must be in 1..1024");
    FQSS_REQUIRE(mode >= 0 && mode <= 2, "mode must be 0 (asteroid), 1 (per sample) or 2 (teacher-free PIT SI-SDR)");
    FQSS_REQUIRE(mode != 1 || B == 1 || B == S,
                 "the per-sample KD weights broadcast [1, n_src, n_src] * [1, B]: B must be 1 or n_src (the reference raises otherwise)");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(stats, 0, sizeof(double) * kStatStrideN * B, s) != hipSuccess) return launch_status("fqss_kd_loss_n(memset)");
    const int ut = use_threshold ? 1 : 0;
    if (S == 1) kd_launch_n<1>(est, fest, tgt, B, T, kd_lambda, mode, ut, threshold, stats, out, w_out, sisdr_out, true, s);
    else if (S == 2) kd_launch_n<2>(est, fest, tgt, B, T, kd_lambda, mode, ut, threshold, stats, out, w_out, sisdr_out, true, s);
    else kd_launch_n<3>(est, fest, tgt, B, T, kd_lambda, mode, ut, threshold, stats, out, w_out, sisdr_out, true, s);
    if (gest) {
        int64_t ng = cdiv(T, 256 * 4);
        if (ng > 256) ng = 256;
        hipLaunchKernelGGL(k_kd_grad_n, dim3((unsigned)ng, (unsigned)(S * B)), dim3(256), 0, s, est, fest, tgt, S, T, stats, gest);
    }
    return launch_status("fqss_kd_loss_n");
}

extern "C" int fqss_kd_moments_n(const float* est, const float* fest, const float* tgt, int B, int S, int64_t T, double* stats,
                                 fqss_stream_t stream) {
    FQSS_REQUIRE(est && fest && tgt && stats, "null tensor");
    FQSS_REQUIRE(S >= 1 && S <= 3, "n_src must be in 1..3");
    FQSS_REQUIRE(B > 0 && B <= 1024 && T > 0, "B must be in 1..1024");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(stats, 0, sizeof(double) * kStatStrideN * B, s) != hipSuccess) return launch_status("fqss_kd_moments_n(memset)");
    if (S == 1) kd_launch_n<1>(est, fest, tgt, B, T, 0.0f, 0, 0, 0.0f, stats, nullptr, nullptr, nullptr, false, s);
    else if (S == 2) kd_launch_n<2>(est, fest, tgt, B, T, 0.0f, 0, 0, 0.0f, stats, nullptr, nullptr, nullptr, false, s);
    else kd_launch_n<3>(est, fest, tgt, B, T, 0.0f, 0, 0, 0.0f, stats, nullptr, nullptr, nullptr, false, s);
    return launch_status("fqss_kd_moments_n");
}

// ---- FQSS_DETERMINISTIC=1 (fqss_dev.h: grad_add): the control blocks of every TU, the finish pass
static std::vector<det_setter_t>& det_setters() {
    static std::vector<det_setter_t> v;      // built on first use: TUs register from their static initialisers, in any order
    return v;
}
void fqss::det_register(det_setter_t fn) { det_setters().push_back(fn); }

// g[i] += the integer sums of its two shadow words, rounded once (thread i -> element i: no order to depend on); shadow cleared
__global__ __launch_bounds__(256) void k_det_finish(float* __restrict__ g, long long* __restrict__ sh, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const longlong2 w = *reinterpret_cast<const longlong2*>(sh + 2 * i);
        if (w.x != 0 || w.y != 0) {
            const double v = (double)w.x * 0x1p-30 + (double)w.y * 0x1p-80;
            g[i] = g[i] + (float)v;
            *reinterpret_cast<longlong2*>(sh + 2 * i) = make_longlong2(0, 0);
        }
    }
}

static DetCtl g_det_ctl{};      // host copy of the control block (slot 0 must be set for the mode to be on)

extern "C" int fqss_set_deterministic(int slot, const float* grad_base, int64_t n, void* shadow) {
    FQSS_REQUIRE(slot >= 0 && slot < kDetSlots, "slot: 0 (parameter gradients), 1 (dL/dW_q arena) or 2 (temporaries)");
    FQSS_REQUIRE((shadow == nullptr) || (grad_base != nullptr && n > 0 && aligned16(shadow)), "bad args");
    g_det_ctl.shadow[slot] = (long long*)shadow;
    g_det_ctl.base[slot] = shadow ? grad_base : nullptr;
    g_det_ctl.n[slot] = shadow ? (long long)n : 0;
    if (hipDeviceSynchronize() != hipSuccess) return launch_status("fqss_set_deterministic");     // no kernel may be reading the old block
    for (det_setter_t fn : det_setters()) {
        const int rc = fn(&g_det_ctl);
        if (rc != 0) {      // a TU still on the old control block would mix float and integer atomics on one arena: refuse loudly
            set_error("fqss_set_deterministic: hipMemcpyToSymbol: %s", hipGetErrorString((hipError_t)rc));
            return FQSS_ELAUNCH;
        }
    }
    return launch_status("fqss_set_deterministic");
}

extern "C" int fqss_det_finish(float* grad_base, int64_t n, void* shadow, fqss_stream_t stream) {
    FQSS_REQUIRE(grad_base && shadow && n >= 0 && aligned16(shadow), "bad args");
    if (n == 0) return FQSS_OK;
    int64_t nb = cdiv(n, 256 * 4);
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_det_finish, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, grad_base, (long long*)shadow, n);
    return launch_status("fqss_det_finish");
}

extern "C" int fqss_sumsq(const float* g, int64_t n, double* sumsq, fqss_stream_t stream) {
    FQSS_REQUIRE(g && sumsq && n >= 0, "bad args");
    if (n == 0) return FQSS_OK;
    int64_t nb = cdiv(n, 256 * 8);
    if (nb > 1024) nb = 1024;
    hipLaunchKernelGGL(k_sumsq, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, g, n, sumsq);
    return launch_status("fqss_sumsq");
}

extern "C" int fqss_grad_accum(float* acc, float* g, int64_t n, int mode, fqss_stream_t stream) {
    FQSS_REQUIRE(acc && g, "null pointer");
    FQSS_REQUIRE(mode >= 0 && mode <= 3, "mode: 0 (acc = g), 1 (acc += g), 2 (g += acc) or 3 (g = acc)");
    FQSS_REQUIRE(n >= 0 && n % 4 == 0 && aligned16(acc) && aligned16(g), "n must be a multiple of 4 floats and both pointers 16-B aligned");
    FQSS_REQUIRE(acc + n <= g || g + n <= acc, "acc and g overlap");
    if (n == 0) return FQSS_OK;
    const int64_t n4 = n / 4;
    int64_t nb = cdiv(n4, 256);
    if (nb > 2048) nb = 2048;
    hipStream_t s = (hipStream_t)stream;
    float4* a4 = reinterpret_cast<float4*>(acc);
    float4* g4 = reinterpret_cast<float4*>(g);
    if (mode == 0) hipLaunchKernelGGL(k_grad_accum<0>, dim3((unsigned)nb), dim3(256), 0, s, a4, g4, n4);
    else if (mode == 1) hipLaunchKernelGGL(k_grad_accum<1>, dim3((unsigned)nb), dim3(256), 0, s, a4, g4, n4);
    else if (mode == 2) hipLaunchKernelGGL(k_grad_accum<2>, dim3((unsigned)nb), dim3(256), 0, s, a4, g4, n4);
    else hipLaunchKernelGGL(k_grad_accum<3>, dim3((unsigned)nb), dim3(256), 0, s, a4, g4, n4);
    return launch_status("fqss_grad_accum");
}

extern "C" int fqss_adam_clip(float* p, const float* g, float* m, float* v, int64_t n, const double* sumsq,
                              float max_norm, float grad_scale, float lr, float beta1, float beta2, float eps,
                              int32_t* step_t, const int32_t* t0, float* gnorm_out, fqss_stream_t stream) {
    FQSS_REQUIRE(p && g && m && v && sumsq && step_t && n >= 0, "bad args");
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) {
        int64_t nb = cdiv(n, 256 * 4);
        if (nb > 2048) nb = 2048;
        hipLaunchKernelGGL(k_adam_clip, dim3((unsigned)nb), dim3(256), 0, s, p, g, m, v, n, sumsq, max_norm, grad_scale,
                           lr, beta1, beta2, eps, step_t, t0);
    }
    hipLaunchKernelGGL(k_step_end, dim3(1), dim3(64), 0, s, step_t, sumsq, grad_scale, gnorm_out);
    return launch_status("fqss_adam_clip");
}

template <int KIND>
static void launch_optim(bool vec, unsigned nb, hipStream_t s, float* p, const float* g, float* m, float* v, int64_t n,
                         const double* sumsq, float max_norm, float grad_scale, float lr, float beta1, float beta2, float eps,
                         const int32_t* step_t, const int32_t* t0, float wd, const float* wd_slot, float mu, int nesterov) {
    if (vec)
        hipLaunchKernelGGL((k_optim_clip<KIND, 4>), dim3(nb), dim3(256), 0, s, p, g, m, v, n, sumsq, max_norm, grad_scale, lr, beta1,
                           beta2, eps, step_t, t0, wd, wd_slot, mu, nesterov);
    else
        hipLaunchKernelGGL((k_optim_clip<KIND, 1>), dim3(nb), dim3(256), 0, s, p, g, m, v, n, sumsq, max_norm, grad_scale, lr, beta1,
                           beta2, eps, step_t, t0, wd, wd_slot, mu, nesterov);
}

extern "C" int fqss_optim_clip(float* p, const float* g, float* m, float* v, int64_t n, const double* sumsq, float max_norm,
                               float grad_scale, float lr, float beta1, float beta2, float eps, int32_t* step_t, const int32_t* t0,
                               float* gnorm_out, int kind, float weight_decay, const float* wd_slot, float momentum, int nesterov,
                               fqss_stream_t stream) {
    FQSS_REQUIRE(kind == FQSS_OPT_ADAM || kind == FQSS_OPT_ADAMW || kind == FQSS_OPT_SGD, "kind: FQSS_OPT_ADAM, FQSS_OPT_ADAMW or FQSS_OPT_SGD");
    FQSS_REQUIRE(p && g && sumsq && step_t && n >= 0, "bad args");
    FQSS_REQUIRE(weight_decay >= 0.0f, "weight_decay must be >= 0");
    FQSS_REQUIRE(momentum >= 0.0f && momentum < 1.0f, "momentum must lie in [0, 1)");
    FQSS_REQUIRE(nesterov == 0 || (nesterov == 1 && momentum > 0.0f), "nesterov: 0 or 1, and 1 needs a momentum > 0");
    FQSS_REQUIRE(kind == FQSS_OPT_SGD ? (m || momentum == 0.0f) : (m && v), "null moment buffer");
    FQSS_REQUIRE(!wd_slot || n % 64 == 0, "a decay table needs n to be a multiple of 64 floats");
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) {
        const bool vec = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(t0);
        int64_t nb = cdiv(cdiv(n, vec ? 4 : 1), 256);
        if (nb > 2048) nb = 2048;
        if (kind == FQSS_OPT_ADAM)
            launch_optim<FQSS_OPT_ADAM>(vec, (unsigned)nb, s, p, g, m, v, n, sumsq, max_norm, grad_scale, lr, beta1, beta2, eps, step_t, t0,
                                        weight_decay, wd_slot, momentum, nesterov);
        else if (kind == FQSS_OPT_ADAMW)
            launch_optim<FQSS_OPT_ADAMW>(vec, (unsigned)nb, s, p, g, m, v, n, sumsq, max_norm, grad_scale, lr, beta1, beta2, eps, step_t, t0,
                                         weight_decay, wd_slot, momentum, nesterov);
        else
            launch_optim<FQSS_OPT_SGD>(vec, (unsigned)nb, s, p, g, m, v, n, sumsq, max_norm, grad_scale, lr, beta1, beta2, eps, step_t, t0,
                                       weight_decay, wd_slot, momentum, nesterov);
    }
    hipLaunchKernelGGL(k_step_end, dim3(1), dim3(64), 0, s, step_t, sumsq, grad_scale, gnorm_out);
    return launch_status("fqss_optim_clip");
}

static int ema_impl(const char* who, float* ema, const float* p, int64_t n, float w, double decay, double* count, fqss_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    const bool vec = aligned16(ema) && aligned16(p);
    int64_t nb = cdiv(cdiv(n, vec ? 4 : 1), 256);
    if (nb > 2048) nb = 2048;
    if (vec) hipLaunchKernelGGL(k_ema_update<4>, dim3((unsigned)nb), dim3(256), 0, s, ema, p, n, w, decay, (const double*)count);
    else hipLaunchKernelGGL(k_ema_update<1>, dim3((unsigned)nb), dim3(256), 0, s, ema, p, n, w, decay, (const double*)count);
    if (count) hipLaunchKernelGGL(k_ema_count_end, dim3(1), dim3(64), 0, s, count, decay);
    return launch_status(who);
}

extern "C" int fqss_ema_update(float* ema, const float* p, int64_t n, float w, fqss_stream_t stream) {
    FQSS_REQUIRE(ema && p && n >= 0, "null pointer");
    FQSS_REQUIRE(w >= 0.0f && w <= 1.0f, "w must lie in [0, 1]");
    FQSS_REQUIRE(ema + n <= p || p + n <= ema, "ema and p overlap");
    if (n == 0) return FQSS_OK;
    return ema_impl("fqss_ema_update", ema, p, n, w, 0.0, nullptr, stream);
}

extern "C" int fqss_ema_update_dev(float* ema, const float* p, int64_t n, double decay, double* count, fqss_stream_t stream) {
    FQSS_REQUIRE(ema && p && count && n >= 0, "null pointer");
    FQSS_REQUIRE(decay >= 0.0 && decay < 1.0, "decay must lie in [0, 1)");
    FQSS_REQUIRE(ema + n <= p || p + n <= ema, "ema and p overlap");
    if (n == 0) return FQSS_OK;
    return ema_impl("fqss_ema_update_dev", ema, p, n, 0.0f, decay, count, stream);
}
