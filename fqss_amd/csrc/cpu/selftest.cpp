// Driver of the sanitizer build (make asan): every entry point of fqss_cpu.cpp on small RAGGED shapes (row strides > columns, odd sizes,
// empty inputs), buffers sized exactly, a few identities checked.  AddressSanitizer / UBSan do the rest.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fqss.h"
#define CHECK(x) do { if (!(x)) { printf("FAILED: %s (line %d): %s\n", #x, __LINE__, fqss_last_error()); return 1; } } while (0)
static std::vector<float> rnd(size_t n, float s = 1.0f) {
    std::vector<float> v(n);
    for (auto& x : v) x = s * ((float)rand() / RAND_MAX - 0.5f);
    return v;
}
int main() {
    const int B = 2, C = 5, M = 37, ld = 40, Co = 7;
    auto x = rnd((size_t)B * C * ld), g = rnd((size_t)B * C * ld);
    std::vector<float> y((size_t)B * C * ld), gz((size_t)B * C * ld);
    std::vector<uint8_t> idx((size_t)B * C * 48);
    float lo = -0.4f, hi = 0.45f, slope = 0.25f;
    uint32_t obs[2];
    CHECK(fqss_obs_reset(obs, 1, nullptr) == 0);
    CHECK(fqss_actq_fwd(x.data(), y.data(), nullptr, B * C, M, ld, ld, 0, FQSS_ACT_PRELU, &slope, FQSS_Q_OBSERVE, nullptr, nullptr, obs, nullptr) == 0);
    CHECK(fqss_observer_ema(&lo, &hi, obs, 0.9, nullptr) == 0);
    CHECK(fqss_actq_fwd(x.data(), y.data(), idx.data(), B * C, M, ld, ld, 48, FQSS_ACT_RELU, nullptr, FQSS_Q_QUANT, &lo, &hi, nullptr, nullptr) == 0);
    std::vector<float> y2(y.size());
    CHECK(fqss_actq_fwd(y.data(), y2.data(), nullptr, B * C, M, ld, ld, 0, FQSS_ACT_NONE, nullptr, FQSS_Q_QUANT, &lo, &hi, nullptr, nullptr) == 0);
    for (int r = 0; r < B * C; ++r)
        for (int m = 0; m < M; ++m) CHECK(y[r * ld + m] == y2[r * ld + m]);      // the quantizer is idempotent on its own grid
    std::vector<double> gacc(FQSS_GACC_SLOTS * 3, 0.0);
    std::vector<float> gb(C, 0.f);
    float gmin = 0, gmax = 0, gsl = 0;
    CHECK(fqss_actq_bwd(x.data(), g.data(), gz.data(), B * C, M, ld, ld, ld, FQSS_ACT_PRELU, &slope, FQSS_Q_QUANT, &lo, &hi, gacc.data(), gb.data(), C, nullptr) == 0);
    CHECK(fqss_gacc_flush(gacc.data(), &gmin, &gmax, &gsl, nullptr) == 0);
    CHECK(fqss_actq_fwd(nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == 0);      // empty input
    CHECK(fqss_minmax(x.data(), B * C, M, ld, obs, nullptr) == 0);
    // weight quantizer, both channel axes
    auto w = rnd((size_t)Co * C * 3);
    std::vector<float> wq(w.size()), gw(w.size()), qlo(C), qhi(C), glo(C), ghi(C);
    std::vector<int8_t> wi(w.size());
    CHECK(fqss_wq_observe(w.data(), Co, C, 3, qlo.data(), qhi.data(), nullptr) == 0);
    CHECK(fqss_wq_fwd(w.data(), wq.data(), wi.data(), Co, C, 3, qlo.data(), qhi.data(), nullptr) == 0);
    CHECK(fqss_wq_bwd(w.data(), wq.data(), gw.data(), glo.data(), ghi.data(), Co, C, 3, qlo.data(), qhi.data(), 0, nullptr) == 0);
    // ... at every supported width: codes stay inside the width's range; widths outside 2..8 are refused
    for (int nb = FQSS_WQ_MIN_BITS; nb <= FQSS_WQ_MAX_BITS; ++nb) {
        CHECK(fqss_wq_fwd_bits(w.data(), wq.data(), wi.data(), Co, C, 3, qlo.data(), qhi.data(), nb, nullptr) == 0);
        for (size_t k = 0; k < wi.size(); ++k) CHECK(wi[k] >= -(1 << (nb - 1)) && wi[k] <= (1 << (nb - 1)) - 1);
        CHECK(fqss_wq_bwd_bits(w.data(), wq.data(), gw.data(), glo.data(), ghi.data(), Co, C, 3, qlo.data(), qhi.data(), 0, nb, nullptr) == 0);
    }
    CHECK(fqss_wq_fwd_bits(w.data(), wq.data(), wi.data(), Co, C, 3, qlo.data(), qhi.data(), 1, nullptr) == FQSS_EINVAL);
    CHECK(fqss_wq_bwd_bits(w.data(), wq.data(), gw.data(), glo.data(), ghi.data(), Co, C, 3, qlo.data(), qhi.data(), 0, 9, nullptr) == FQSS_EINVAL);
    // pointwise conv and its gradients; <gz, W x> == <W^T gz, x>
    auto pw = rnd((size_t)Co * C), bias = rnd(Co), gzc = rnd((size_t)B * Co * ld);
    std::vector<float> z((size_t)B * Co * ld), gx((size_t)B * C * ld), gpw((size_t)Co * C, 0.f);
    CHECK(fqss_pwconv_fwd_x3(x.data(), pw.data(), nullptr, z.data(), B, C, Co, M, ld, ld, nullptr) == 0);
    CHECK(fqss_pwconv_bwd_x(gzc.data(), pw.data(), gx.data(), B, C, Co, M, ld, ld, nullptr) == 0);
    CHECK(fqss_pwconv_bwd_w(gzc.data(), x.data(), gpw.data(), B, C, Co, M, ld, ld, nullptr) == 0);
    double a = 0, b2 = 0;
    for (int b = 0; b < B; ++b) {
        for (int co = 0; co < Co; ++co) for (int m = 0; m < M; ++m) a += (double)gzc[(b * Co + co) * ld + m] * z[(b * Co + co) * ld + m];
        for (int ci = 0; ci < C; ++ci) for (int m = 0; m < M; ++m) b2 += (double)gx[(b * C + ci) * ld + m] * x[(b * C + ci) * ld + m];
    }
    CHECK(fabs(a - b2) <= 1e-4 * (fabs(a) + 1.0));
    CHECK(fqss_pwconv_fwd(x.data(), pw.data(), bias.data(), z.data(), B, C, Co, M, ld, ld, nullptr) == 0);
    // depthwise conv, GroupNorm
    auto dw = rnd((size_t)C * 3), db = rnd(C);
    std::vector<float> gdw((size_t)C * 3, 0.f), mr(2 * B), gg(C, 0.f), gbt(C, 0.f);
    CHECK(fqss_dwconv_fwd(x.data(), dw.data(), db.data(), y.data(), B, C, M, 3, 4, 4, ld, ld, nullptr) == 0);
    CHECK(fqss_dwconv_bwd_x(g.data(), dw.data(), gz.data(), B, C, M, 3, 4, 4, ld, ld, nullptr) == 0);
    CHECK(fqss_dwconv_bwd_w(g.data(), x.data(), gdw.data(), B, C, M, 3, 4, 4, ld, ld, nullptr) == 0);
    auto gam = rnd(C), bet = rnd(C);
    CHECK(fqss_gn_fwd(x.data(), gam.data(), bet.data(), y.data(), mr.data(), B, C, M, ld, ld, 1e-8f, nullptr, nullptr) == 0);
    CHECK(fqss_gn_bwd(g.data(), x.data(), gam.data(), mr.data(), gz.data(), gg.data(), gbt.data(), B, C, M, ld, ld, ld, nullptr, nullptr) == 0);
    // element-wise, masking product
    CHECK(fqss_axpby(x.data(), g.data(), 1.0f, -1.0f, y.data(), B * C, M, ld, ld, ld, nullptr) == 0);
    const int S = 2;
    auto mask = rnd((size_t)B * S * C * ld);
    std::vector<float> mz(mask.size()), gmask(mask.size()), gfeat((size_t)B * C * ld);
    CHECK(fqss_mul_bcast_fwd(mask.data(), x.data(), mz.data(), B, S, C, M, ld, ld, ld, nullptr) == 0);
    CHECK(fqss_mul_bcast_bwd(mz.data(), mask.data(), x.data(), gmask.data(), gfeat.data(), B, S, C, M, ld, ld, ld, ld, ld, nullptr) == 0);
    // splitter, framing conv, overlap-add, weight gradients
    const int K = 16, st = 8;
    const int64_t T = (int64_t)(M - 1) * st + K;
    auto sig = rnd((size_t)B * T, 1.8f);
    std::vector<float> sp((size_t)B * 2 * T), enc((size_t)B * Co * ld), dec((size_t)B * T), gwe((size_t)Co * 2 * K, 0.f), gwd((size_t)Co * K, 0.f);
    CHECK(fqss_obs_reset(obs, 1, nullptr) == 0 && fqss_minmax(sig.data(), B, T, T, obs, nullptr) == 0);
    CHECK(fqss_splitter2(sig.data(), sp.data(), B, T, obs, nullptr) == 0);
    auto ew = rnd((size_t)Co * 2 * K);
    CHECK(fqss_frames_conv_fwd(sp.data(), ew.data(), enc.data(), B, 2, Co, T, K, st, M, ld, nullptr) == 0);
    CHECK(fqss_ola_convtr_fwd(enc.data(), ew.data(), dec.data(), B, Co, M, ld, K, st, T, nullptr) == 0);
    CHECK(fqss_frames_wgrad(enc.data(), sp.data(), gwe.data(), B, Co, 2, M, ld, T, K, st, nullptr) == 0);
    CHECK(fqss_frames_wgrad1(enc.data(), dec.data(), gwd.data(), B, Co, M, ld, T, K, st, nullptr) == 0);
    CHECK(fqss_frames_wgrad1s(enc.data(), sp.data() + T, 2 * T, gwe.data() + K, 2 * K, B, Co, M, ld, T, K, st, nullptr) == 0);
    // loss, clip + Adam
    const int64_t TT = 301;
    auto est = rnd((size_t)B * 2 * TT), fe = rnd((size_t)B * 2 * TT), tg = rnd((size_t)B * 2 * TT);
    std::vector<float> out(4), wv(B), si(B), ge((size_t)B * 2 * TT);
    CHECK(fqss_kd_loss(est.data(), fe.data(), tg.data(), B, TT, 0.1f, nullptr, out.data(), wv.data(), si.data(), ge.data(), nullptr) == 0);
    CHECK(std::isfinite(out[0]) && std::isfinite(ge[5]));
    // the same loss at 1 and 3 sources: every mode, the moment pass alone, the refused arguments
    for (int NS : {1, 3}) {
        const int64_t TN = 257;
        const int BN = 3;
        auto en = rnd((size_t)BN * NS * TN), fn = rnd((size_t)BN * NS * TN), tn = rnd((size_t)BN * NS * TN);
        std::vector<double> stn((size_t)BN * FQSS_KD_STATS_STRIDE_N);
        std::vector<float> on(4), wn(BN), sn(BN), gn_((size_t)BN * NS * TN);
        for (int mode = 0; mode < 3; ++mode) {
            const int Bm = (mode == 1) ? NS : BN;
            CHECK(fqss_kd_loss_n(en.data(), fn.data(), tn.data(), Bm, NS, TN, 0.1f, mode, mode == 1, -30.0f, stn.data(), on.data(), wn.data(),
                                 sn.data(), gn_.data(), nullptr) == 0);
            CHECK(std::isfinite(on[0]) && std::isfinite(gn_[(size_t)Bm * NS * TN - 1]));
        }
        CHECK(fqss_kd_loss_n(en.data(), fn.data(), tn.data(), 1, NS, TN, 0.1f, 1, 0, 0.0f, stn.data(), on.data(), wn.data(), sn.data(), nullptr,
                             nullptr) == 0);
        CHECK(fqss_kd_moments_n(en.data(), fn.data(), tn.data(), BN, NS, TN, stn.data(), nullptr) == 0);
        CHECK(std::isfinite(stn[(size_t)(BN - 1) * FQSS_KD_STATS_STRIDE_N + 6 * NS + 3 * NS * NS - 1]));
        CHECK(fqss_kd_loss_n(en.data(), fn.data(), tn.data(), 2, 3, TN, 0.1f, 1, 0, 0.0f, stn.data(), on.data(), wn.data(), sn.data(), nullptr,
                             nullptr) == FQSS_EINVAL);
        CHECK(fqss_kd_loss_n(en.data(), fn.data(), tn.data(), 1, 4, TN, 0.1f, 0, 0, 0.0f, stn.data(), on.data(), wn.data(), sn.data(), nullptr,
                             nullptr) == FQSS_EINVAL);
        CHECK(fqss_kd_moments_n(en.data(), fn.data(), tn.data(), BN, 0, TN, stn.data(), nullptr) == FQSS_EINVAL);
    }
    const int64_t n = 1001;
    auto p = rnd(n), gp = rnd(n);
    std::vector<float> m1(n, 0.f), v1(n, 0.f);
    std::vector<int32_t> t0(n, 0);
    t0[7] = INT32_MAX;
    double ss = 0.0;
    int32_t stp = 0;
    float gn = 0.f;
    CHECK(fqss_sumsq(gp.data(), n, &ss, nullptr) == 0);
    const float p7 = p[7];
    CHECK(fqss_adam_clip(p.data(), gp.data(), m1.data(), v1.data(), n, &ss, 5.0f, 1.0f, 1e-3f, 0.9f, 0.999f, 1e-8f, &stp, t0.data(), &gn, nullptr) == 0);
    CHECK(stp == 1 && p[7] == p7 && fabs(gn - sqrt(ss)) < 1e-3);
    // gradient accumulation: the four modes on a 16-B aligned pair, the refused arguments
    {
        alignas(16) float ac[8] = {1, 2, 3, 4, 5, 6, 7, 8}, gg[8] = {.5f, .5f, .5f, .5f, -1, -1, -1, -1};
        CHECK(fqss_grad_accum(ac, gg, 8, 1, nullptr) == 0 && ac[0] == 1.5f && ac[7] == 7.0f && gg[7] == -1.0f);
        CHECK(fqss_grad_accum(ac, gg, 8, 2, nullptr) == 0 && gg[0] == 2.0f && gg[7] == 6.0f && ac[7] == 7.0f);
        CHECK(fqss_grad_accum(ac, gg, 8, 0, nullptr) == 0 && ac[3] == gg[3] && fqss_grad_accum(ac, gg, 8, 3, nullptr) == 0 && gg[4] == ac[4]);
        CHECK(fqss_grad_accum(ac, gg, 0, 1, nullptr) == 0);
        CHECK(fqss_grad_accum(ac, gg, 6, 1, nullptr) == FQSS_EINVAL && fqss_grad_accum(ac + 1, gg, 4, 1, nullptr) == FQSS_EINVAL);
        CHECK(fqss_grad_accum(ac, gg, 8, 4, nullptr) == FQSS_EINVAL && fqss_grad_accum(nullptr, gg, 8, 1, nullptr) == FQSS_EINVAL);
    }
    // signal-to-distortion ratio: pitched rows, a signal shorter than the filter, a silent target, refused arguments
    {
        const int P = 3, ldp = 310;
        const int64_t Ls = 300;
        auto pe = rnd((size_t)P * ldp), pr = rnd((size_t)P * ldp);
        for (int64_t i = 0; i < Ls; ++i) {
            pe[i] = pr[i] + 0.1f * pe[i];
            pr[ldp + i] = 0.0f;
        }
        for (int F : {1, 7, 512}) {
            std::vector<double> wsd((size_t)fqss_sdr_ws_doubles(P, Ls, F)), dbv(P, 0.0);
            CHECK(wsd.size() == (size_t)P * (2 * F + 4));
            CHECK(fqss_sdr(pe.data(), pr.data(), wsd.data(), (int64_t)wsd.size(), dbv.data(), P, Ls, ldp, ldp, F, F == 7, F == 7 ? 1e-3 : -1.0, nullptr) == 0);
            CHECK(std::isfinite(dbv[0]) && dbv[0] > 10.0 && std::isnan(dbv[1]) == (F != 7) && std::isfinite(dbv[2]));
            CHECK(fqss_sdr(pe.data(), pr.data(), wsd.data(), (int64_t)wsd.size() - 1, dbv.data(), P, Ls, ldp, ldp, F, 0, -1.0, nullptr) == FQSS_EINVAL);
        }
        std::vector<double> wsd(4096), dbv(P);
        CHECK(fqss_sdr(pe.data(), pr.data(), wsd.data(), 4096, dbv.data(), P, Ls, ldp, ldp, 513, 0, -1.0, nullptr) == FQSS_EINVAL);
        CHECK(fqss_sdr(pe.data(), pr.data(), wsd.data(), 4096, dbv.data(), P, Ls, Ls - 1, ldp, 8, 0, -1.0, nullptr) == FQSS_EINVAL);
        CHECK(fqss_sdr_ws_doubles(P, 0, 8) == 0);
    }
    // batched chunked inference: a group that runs past the last (short) chunk, per-row splitter, per-chunk maps, gather-form overlap-add
    {
        const int64_t Lc = 310, seg = 100, hop = 75, Nc = 5;      // chunk 4 holds 10 samples
        const int G = 3, Sc = 2;
        auto mixc = rnd((size_t)Lc), tgt = rnd((size_t)Sc * (Lc + 3));
        std::vector<float> rows((size_t)G * seg), sp2((size_t)G * 2 * seg), ck((size_t)(Nc + 1) * Sc * seg), dbc((size_t)G * Sc * Sc), oc((size_t)Sc * Lc);
        std::vector<int> mpc((size_t)(Nc + 1) * Sc * 2);
        std::vector<uint32_t> rmax(G, 0u);
        CHECK(fqss_chunk_gather(mixc.data(), rows.data(), Lc, seg, hop, 3, G, nullptr) == 0);
        for (int64_t t = 0; t < seg; ++t) CHECK(rows[seg + t] == (t < 10 ? mixc[4 * hop + t] : 0.0f) && rows[2 * seg + t] == rows[seg + t]);
        CHECK(fqss_splitter2_rows(rows.data(), sp2.data(), G, seg, rmax.data(), nullptr) == 0);
        for (auto v : sp2) CHECK(v >= -1.0f && v < 1.0f);
        for (int64_t k = 0; k < Nc + 1; ++k)      // est = the targets swapped, so every full chunk's map is (1, -1), (0, -1)
            for (int s2 = 0; s2 < Sc; ++s2)
                for (int64_t t = 0; t < seg; ++t) {
                    const int64_t i = (k < Nc ? k : Nc - 1) * hop + t;
                    ck[(k * Sc + s2) * seg + t] = i < Lc ? tgt[(1 - s2) * (Lc + 3) + i] : 0.0f;
                }
        for (int64_t k0 = 0; k0 < Nc; k0 += G)
            CHECK(fqss_sisnr_chunks(ck.data() + k0 * Sc * seg, tgt.data(), dbc.data(), mpc.data() + k0 * Sc * 2, G, Sc, seg, hop, k0, Lc, Lc + 3, nullptr) == 0);
        for (int64_t k = 0; k < Nc; ++k) CHECK(mpc[k * 4] == 1 && mpc[k * 4 + 1] == -1 && mpc[k * 4 + 2] == 0 && mpc[k * 4 + 3] == -1);
        CHECK(fqss_infer_ola_chunks(ck.data(), mpc.data(), oc.data(), Sc, 1, Lc, seg, hop, seg, Lc, nullptr) == 0);
        for (int64_t t = 0; t < Lc; ++t) CHECK(fabsf(oc[t] + tgt[t]) <= 1e-6f && fabsf(oc[Lc + t] + tgt[Lc + 3 + t]) <= 1e-6f);
        CHECK(fqss_infer_ola_chunks(ck.data(), nullptr, oc.data(), Sc, 1, Lc, seg, hop, seg, Lc, nullptr) == 0);
        CHECK(fqss_chunk_gather(mixc.data(), rows.data(), Lc, seg, hop, Nc, G, nullptr) == FQSS_EINVAL);
        CHECK(fqss_chunk_gather(mixc.data(), rows.data(), Lc, seg, seg + 1, 0, G, nullptr) == FQSS_EINVAL);
        CHECK(fqss_sisnr_chunks(ck.data(), tgt.data(), dbc.data(), mpc.data(), G, 17, seg, hop, 0, Lc, Lc + 3, nullptr) == FQSS_EINVAL);
        CHECK(fqss_infer_ola_chunks(ck.data(), nullptr, oc.data(), Sc, 1, Lc, seg, 0, seg, Lc, nullptr) == FQSS_EINVAL);
        CHECK(fqss_splitter2_rows(rows.data(), sp2.data(), G, seg, nullptr, nullptr) == FQSS_EINVAL);
    }
    CHECK(fqss_version() == FQSS_VERSION);
    printf("selftest ok\n");
    return 0;
}
