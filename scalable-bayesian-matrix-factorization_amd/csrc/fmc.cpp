// fmc.cpp -- libFM's MCMC / ALS chain on the host (fmc.h): the draws, the sweep and the
// read-outs shared by the two-attribute learner (fmm.cpp) and the general one (fmg.cpp).
#include "fmc.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "fmg.h"
#include "fmm.h"
#include "kernels.h"

namespace sbmf {

// the Philox streams of the w and v passes' normals and of the initial model
enum : uint32_t { TAG_FMC_W = 8, TAG_FMC_V = 9, TAG_FMC_INIT = 10 };

FMChain::~FMChain() {
    for (auto& e : ev) event_destroy(e);
}

template <class R>
static double gaussian(R& g, double mean, double stdev) {  // random.h:166-172
    if (stdev == 0.0 || std::isnan(stdev)) return mean;
    return mean + stdev * leva_normal(g);
}

// fm_model::init (fm_model.h:87-96: v, f-major) then w (libfm.cpp:412)
template <class R>
void FMChain::init_model(R& g, std::vector<double>& h_w, std::vector<double>& h_v) {
    const double sd = cfg.init_stdev >= 0 ? cfg.init_stdev : 0.1;
    h_v.resize((size_t)K * p);
    h_w.resize(p);
    for (double& x : h_v) x = gaussian(g, 0.0, sd);
    for (double& x : h_w) x = gaussian(g, 0.0, sd);
}

// fm_learn_mcmc.h:931-1007: draw_w_lambda over every group, then draw_w_mu over every group.  Per
// group g with cnt[g] attributes: gm = beta_0 (w_mu[g] - mu_0)^2 + gamma_0 + sum_{i in g} (w_i -
// w_mu[g])^2 and m = sum_{i in g} w_i come from the device, each summed over the group's
// attributes in ascending id, the order the reference's one loop over all attributes gives every
// group.  A NaN / inf draw restores the value and ends that function (the reference returns): the
// groups after it keep their values and consume no variate.
template <class R>
void FMChain::draw_hyper_w(R& g) {
    const double alpha_0 = 1.0, beta_0 = 1.0, mu_0 = 0.0;
    if (!do_multilevel) {
        std::fill(w_mu.begin(), w_mu.end(), mu_0);
        return;
    }
    const double* hs = h_hs.data() + 2 * (size_t)K * G;
    for (uint32_t q = 0; q < G; ++q) {
        const double gm = hs[2 * q];
        const double a = alpha_0 + cnt[q] + 1;
        const double old = w_lambda[q];
        w_lambda[q] = do_sample ? mt_gamma(g, a / 2.0) / (gm / 2.0) : a / gm;
        if (std::isnan(w_lambda[q]) || std::isinf(w_lambda[q])) {
            w_lambda[q] = old;
            break;
        }
    }
    for (uint32_t q = 0; q < G; ++q) {
        double m = hs[2 * q + 1];
        m = (m + beta_0 * mu_0) / (cnt[q] + beta_0);
        const double s2 = 1.0 / ((cnt[q] + beta_0) * w_lambda[q]);
        const double om = w_mu[q];
        w_mu[q] = do_sample ? gaussian(g, m, std::sqrt(s2)) : m;
        if (std::isnan(w_mu[q]) || std::isinf(w_mu[q])) {
            w_mu[q] = om;
            break;
        }
    }
}

// fm_learn_mcmc.h:1011-1089: draw_v_lambda for f, for g, then draw_v_mu for f, for g (a NaN / inf
// ends that function: every later factor and group keeps its value); the sums over each column's
// groups as for w: gm from beta_0 (mu_gf - mu_0)^2 + gamma_0 adding (v_fi - mu_gf)^2, m = sum v_fi
template <class R>
void FMChain::draw_hyper_v(R& g) {
    const double alpha_0 = 1.0, beta_0 = 1.0, mu_0 = 0.0;
    if (!do_multilevel) {
        std::fill(v_mu.begin(), v_mu.end(), mu_0);
        return;
    }
    bool stop = false;
    for (uint32_t f = 0; f < K && !stop; ++f)
        for (uint32_t q = 0; q < G; ++q) {
            double& lam = v_lambda[(size_t)q * K + f];
            const double gm = h_hs[2 * ((size_t)f * G + q)];
            const double a = alpha_0 + cnt[q] + 1;
            const double old = lam;
            lam = do_sample ? mt_gamma(g, a / 2.0) / (gm / 2.0) : a / gm;
            if (std::isnan(lam) || std::isinf(lam)) {
                lam = old;
                stop = true;
                break;
            }
        }
    stop = false;
    for (uint32_t f = 0; f < K && !stop; ++f)
        for (uint32_t q = 0; q < G; ++q) {
            double& mu = v_mu[(size_t)q * K + f];
            double m = h_hs[2 * ((size_t)f * G + q) + 1];
            m = (m + beta_0 * mu_0) / (cnt[q] + beta_0);
            const double s2 = 1.0 / ((cnt[q] + beta_0) * v_lambda[(size_t)q * K + f]);
            const double old = mu;
            mu = do_sample ? gaussian(g, m, std::sqrt(s2)) : m;
            if (std::isnan(mu) || std::isinf(mu)) {
                mu = old;
                stop = true;
                break;
            }
        }
}

// The groups' member lists for the grouped sums kernel (built once; without a group table one
// contiguous group of every attribute)
void FMChain::ensure_group_lists() {
    if (d_gptr.p) return;
    std::vector<uint32_t> gptr((size_t)G + 1, 0), gfirst(G, 0xffffffffu), gidx(std::max<uint32_t>(p, 1), 0);
    for (uint32_t a = 0; a < p; ++a) gptr[(grp.empty() ? 0 : grp[a]) + 1]++;
    for (uint32_t q = 0; q < G; ++q) gptr[q + 1] += gptr[q];
    std::vector<uint32_t> fill(gptr.begin(), gptr.end() - 1);
    for (uint32_t a = 0; a < p; ++a) gidx[fill[grp.empty() ? 0 : grp[a]]++] = a;
    for (uint32_t q = 0; q < G; ++q) {
        const uint32_t b = gptr[q], n = gptr[q + 1] - b;
        if (n == 0 || gidx[b + n - 1] - gidx[b] == n - 1) gfirst[q] = n ? gidx[b] : 0;
    }
    upload(d_gptr, gptr, st);
    upload(d_gfirst, gfirst, st);
    upload(d_gidx, gidx, st);
    HIPCHK(hipStreamSynchronize(st));  // the vectors are locals
}

// {mu, gm's initial value} of every (column, group) up, the sums, {gm, m} down (not waited for)
void FMChain::launch_hsums() {
    const double beta_0 = 1.0, gamma_0 = 1.0, mu_0 = 0.0;
    for (uint32_t c = 0; c <= K; ++c)
        for (uint32_t q = 0; q < G; ++q) {
            const double mu = c < K ? v_mu[(size_t)q * K + c] : w_mu[q];
            h_mg[2 * ((size_t)c * G + q)] = mu;
            h_mg[2 * ((size_t)c * G + q) + 1] = beta_0 * (mu - mu_0) * (mu - mu_0) + gamma_0;
        }
    HIPCHK(hipMemcpyAsync(d_hmg.p, h_mg.data(), h_mg.size() * sizeof(double), hipMemcpyHostToDevice, st));
    if (d_gptr.p)
        HIPCHK(fmg_group_sums(d_v.as<double>(), d_w.as<double>(), p, K, G, d_gptr.as<uint32_t>(), d_gidx.as<uint32_t>(),
                              d_gfirst.as<uint32_t>(), d_hmg.as<double2>(), d_hsum.as<double2>(), st));
    else
        HIPCHK(fmm_hsums(d_v.as<double>(), d_w.as<double>(), p, K, d_hmg.as<double2>(), d_hsum.as<double2>(), st));
    HIPCHK(hipMemcpyAsync(h_hs.data(), d_hsum.p, h_hs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
}

void FMChain::group_sums(double* out) {
    HIPCHK(hipStreamSynchronize(st));
    ensure_group_lists();
    const std::vector<double> keep = h_hs;  // a sweep's sums are read before the next launch: restored anyway
    launch_hsums();
    HIPCHK(hipStreamSynchronize(st));
    std::copy(h_hs.begin(), h_hs.end(), out);
    h_hs = keep;
    if (G == 1 && grp.empty()) {  // an ungrouped chain keeps calling k_fmm_hsums
        d_gptr.release();
        d_gidx.release();
        d_gfirst.release();
    }
}

void FMChain::upload_priors(bool vcols) {
    if (!d_lm.p) return;
    const uint32_t c0 = vcols ? 0 : K, c1 = vcols ? K : K + 1;
    if (c0 == c1) return;
    for (uint32_t c = c0; c < c1; ++c)
        for (uint32_t q = 0; q < G; ++q) {
            h_lm[2 * ((size_t)c * G + q)] = c < K ? v_lambda[(size_t)q * K + c] : w_lambda[q];
            h_lm[2 * ((size_t)c * G + q) + 1] = c < K ? v_mu[(size_t)q * K + c] : w_mu[q];
        }
    HIPCHK(hipMemcpyAsync(d_lm.as<double>() + 2 * (size_t)c0 * G, h_lm.data() + 2 * (size_t)c0 * G,
                          2 * (size_t)(c1 - c0) * G * sizeof(double), hipMemcpyHostToDevice, st));
}

// the normals of a pass, d[a * cols + f]: libFM consumes one per drawn attribute, f-major
template <class R>
void FMChain::fill_normals(R& g, DBuf& d, uint32_t cols, uint32_t tag) {
    if (cfg.rng_mode != SBMF_RNG_REFERENCE) {
        HIPCHK(launch_philox_fill<double>(d.as<double>(), cols, 0, p, cfg.seed, it, tag, st));
        return;
    }
    std::vector<double> z((size_t)p * cols);
    for (uint32_t f = 0; f < cols; ++f)
        for (uint32_t a = 0; a < p; ++a) z[(size_t)a * cols + f] = leva_normal(g);
    HIPCHK(hipMemcpyAsync(d.p, z.data(), z.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // z is a local
}

template <class R>
void FMChain::sweep_draws(R& g) {
    // ---- alpha and w0 (fm_learn_mcmc.h:901-929, :627-668)
    double s[2];
    residual_sums(s);
    if (do_multilevel) {
        // the hyperparameter draws' column sums (fm_learn_mcmc.h:931-1089) on the device, in
        // the host loops' order: w and v do not change before the draws that read them
        launch_hsums();
        ++n_launch;
    }
    HIPCHK(hipStreamSynchronize(st));
    n_launch += 2;
    if (!do_multilevel) {
        alpha = 1.0;  // alpha_0
    } else {
        const double an = 1.0 + (double)N, gn = 1.0 + s[0];
        const double old = alpha;
        alpha = mt_gamma(g, an / 2.0) / (gn / 2.0);
        if (std::isnan(alpha) || std::isinf(alpha)) alpha = old;
    }
    if (k0) {
        const double reg0 = cfg.reg0;
        const double s2 = 1.0 / (reg0 + alpha * (double)N);
        const double m = -s2 * (alpha * s[1] - 0.0 * reg0);
        const double old = w0;
        w0 = do_sample ? gaussian(g, m, std::sqrt(s2)) : m;
        if (std::isnan(w0) || std::isinf(w0)) {
            w0 = old;
        } else {
            shift_residuals(old - w0);
            ++n_launch;
        }
    }
    start_passes();
    // ---- w (:422-457): group hyperparameters, then every attribute
    if (k1) {
        draw_hyper_w(g);
        upload_priors(false);
        if (do_sample) fill_normals(g, d_zw, 1, TAG_FMC_W);
        w_pass();
    }
    // ---- v (:497-621): group hyperparameters of every factor, then factor by factor
    if (K) {
        draw_hyper_v(g);
        upload_priors(true);
        if (do_sample) fill_normals(g, d_zv, K, TAG_FMC_V);
        for (uint32_t f = 0; f < K; ++f) v_pass(f);
    }
    sync_users();
}

void FMChain::predict_train() {
    HIPCHK(fmm_transpose(d_v.as<double>(), d_vT.as<double>(), K, Kp, p, st));
    predict_train_cases();
    n_launch += 2;
}

void FMChain::run(uint32_t iters, sbmf_sweep_cb cb, void* user) {
    double* res = d_res.as<double>();
    for (uint32_t k = 0; k < iters; ++k) {
        n_launch = 0;
        HIPCHK(hipEventRecord(ev[0], st));
        if (cfg.rng_mode == SBMF_RNG_REFERENCE) {
            sweep_draws(grand);
        } else {
            PhiloxStream ps(cfg.seed, it, 3);
            sweep_draws(ps);
        }
        HIPCHK(hipEventRecord(ev[1], st));
        if (classify()) {
            sbmf_sweep_info info{};
            evaluate_class(info);
            float ms0 = 0.f, ms1 = 0.f;
            HIPCHK(hipEventElapsedTime(&ms0, ev[0], ev[1]));
            HIPCHK(hipEventElapsedTime(&ms1, ev[1], ev[2]));
            info.sweep = it;
            info.collected = 1;
            info.rmse_train = info.rmse_avg = info.rmse_this = NAN;
            info.tau = alpha;
            info.ms_sweep = ms0;
            info.ms_eval = ms1;
            ++it;
            if (cb && cb(&info, user)) break;
            continue;
        }
        // ---- predict train and test, evaluate (fm_learn_mcmc_simultaneous.h:134-245)
        predict_train();
        train_sum(res + 2);
        if (T) {
            predict_test((double)(it + 1));
            HIPCHK(launch_sum_cols(d_tpart.as<double>(), (uint32_t)((T + 255) / 256), 2, res + 3, st));
            n_launch += 2;
        }
        if (query) score_queries();
        HIPCHK(hipEventRecord(ev[2], st));
        double h[3] = {0, 0, 0};
        HIPCHK(hipMemcpyAsync(h, res + 2, sizeof h, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        gather_train_sum(h);  // test: every rank has all
        float ms0 = 0.f, ms1 = 0.f;
        HIPCHK(hipEventElapsedTime(&ms0, ev[0], ev[1]));
        HIPCHK(hipEventElapsedTime(&ms1, ev[1], ev[2]));
        sbmf_sweep_info info{};
        info.sweep = it;
        info.collected = 1;
        info.rmse_train = std::sqrt(h[0] / (double)N);
        info.rmse_avg = T ? std::sqrt(h[1] / (double)T) : NAN;
        info.rmse_this = T ? std::sqrt(h[2] / (double)T) : NAN;
        info.acc_train = info.acc_avg = info.acc_this = info.ll_this = NAN;
        info.tau = alpha;
        info.ms_sweep = ms0;
        info.ms_eval = ms1;
        ++it;
        if (cb && cb(&info, user)) break;
    }
}

// Classification's evaluate step (fm_learn_mcmc_simultaneous.h:176-222, :262-275): the test frame,
// then the train frame, which also forms the new latent targets; the counts summed as integers.
// Records ev[2] and waits for the stream.
void FMChain::evaluate_class(sbmf_sweep_info& info) {
    HIPCHK(fmm_transpose(d_v.as<double>(), d_vT.as<double>(), K, Kp, p, st));
    ++n_launch;
    const uint32_t nbt = (uint32_t)((T + 255) / 256), nb = (uint32_t)((N + 255) / 256);
    unsigned long long* cres = d_cres.as<unsigned long long>();
    double* ll = d_tpart.as<double>();
    uint32_t* tcnt = reinterpret_cast<uint32_t*>(ll + nbt);
    if (T) {
        class_test((double)(it + 1), tcnt, ll);
        HIPCHK(fm_count_sums(tcnt, nbt, 2, cres + 1, st));
        HIPCHK(launch_sum_cols(ll, nbt, 1, reinterpret_cast<double*>(cres + 3), st));
        n_launch += 3;
    }
    FMTargetArgs ta{};
    ta.mode = !do_sample ? FM_TGT_ALS : cfg.rng_mode == SBMF_RNG_REFERENCE ? FM_TGT_HOST : FM_TGT_PHILOX;
    ta.seed = cfg.seed;
    ta.it = it;
    ta.yhat = d_tgt.as<double>();
    ta.cnt = d_part.as<uint32_t>();
    class_train(ta);
    HIPCHK(fm_count_sums(ta.cnt, nb, 1, cres, st));
    n_launch += 2;
    if (ta.mode == FM_TGT_HOST) {
        // the reference's stream, in the train file's order (this mode is for parity: a round
        // trip of N doubles and a serial host loop per iteration)
        std::vector<double> t(N);
        HIPCHK(hipMemcpyAsync(t.data(), d_tgt.p, N * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (uint64_t c = 0; c < N; ++c) {
            const uint64_t q = pos_of_file.empty() ? c : pos_of_file[c];
            t[q] = y_pos[q] >= 0.0f ? ran_left_tgaussian(grand, 0.0, t[q], 1.0) : ran_right_tgaussian(grand, 0.0, t[q], 1.0);
        }
        HIPCHK(hipMemcpyAsync(d_tgt.p, t.data(), N * sizeof(double), hipMemcpyHostToDevice, st));
        sub_targets(d_tgt.as<double>());
        ++n_launch;
        HIPCHK(hipStreamSynchronize(st));  // t is a local
    }
    if (query) score_queries();
    HIPCHK(hipEventRecord(ev[2], st));
    unsigned long long h[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(h, cres, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    double llsum;
    std::memcpy(&llsum, &h[3], sizeof llsum);
    info.acc_train = (double)h[0] / (double)N;
    info.acc_avg = T ? (double)h[1] / (double)T : NAN;
    info.acc_this = T ? (double)h[2] / (double)T : NAN;
    info.ll_this = T ? llsum / (double)T : NAN;
}

void FMChain::setup(const sbmf_config& c, hipStream_t stream, uint32_t num_attr, uint64_t n, uint64_t nl, uint64_t nt,
                    const float* y) {
    cfg = c;
    st = stream;
    K = c.num_factor;
    Kp = (K + 15) / 16 * 16;
    p = num_attr;
    N = n;
    T = nt;
    k0 = (c.libfm_dim & 1u) ? 1 : 0;
    k1 = (c.libfm_dim & 2u) ? 1 : 0;
    const bool als = c.method == SBMF_METHOD_ALS;
    do_sample = als ? 0 : 1;  // libfm.cpp:132-136
    do_multilevel = als ? 0 : 1;
    // the train target range (Data.h:200-203)
    float mn = 3.4028234663852886e38f, mx = -3.4028234663852886e38f;
    for (uint64_t x = 0; x < n; ++x) {
        mn = std::min(y[x], mn);
        mx = std::max(y[x], mx);
    }
    lo = mn;
    hi = mx;
    d_w.alloc((size_t)p * sizeof(double));
    d_v.alloc(std::max<size_t>((size_t)K * p, 1) * sizeof(double));
    d_vT.alloc(std::max<size_t>((size_t)p * Kp, 1) * sizeof(double));
    HIPCHK(hipMemsetAsync(d_vT.p, 0, d_vT.bytes, st));
    d_zw.alloc((size_t)p * sizeof(double));
    d_zv.alloc(std::max<size_t>((size_t)K * p, 1) * sizeof(double));
    d_pthis.alloc(std::max<uint64_t>(nt, 1) * sizeof(double));
    d_sum.alloc(std::max<uint64_t>(nt, 1) * sizeof(double));
    HIPCHK(hipMemsetAsync(d_sum.p, 0, d_sum.bytes, st));
    d_part.alloc((std::max<uint64_t>((nl + 255) / 256, 2 * ((nl + 1023) / 1024)) + 2) * sizeof(double));
    d_tpart.alloc((2 * ((nt + 255) / 256) + 2) * sizeof(double));
    d_res.alloc(8 * sizeof(double));
    if (classify()) {
        // {train votes, running-mean test votes, this sweep's test votes} as 64-bit counts, then the ll sum
        d_cres.alloc(4 * sizeof(double));
        HIPCHK(hipMemsetAsync(d_cres.p, 0, d_cres.bytes, st));
        if (y_pos.empty()) y_pos.assign(y, y + n);
        if (!file_of_pos.empty()) {
            pos_of_file.resize(n);
            for (uint64_t q = 0; q < n; ++q) pos_of_file[file_of_pos[q]] = (uint32_t)q;
        }
        if (do_sample && c.rng_mode == SBMF_RNG_REFERENCE)
            d_tgt.alloc(n * sizeof(double));
        else if (do_sample && !file_of_pos.empty())
            upload(d_fidx, file_of_pos, st);
    }
    // the groups a learner set before this call (grp: [p], G = max + 1; empty: one group)
    if (grp.empty()) G = 1;
    cnt.assign(G, 0);
    for (uint32_t a = 0; a < p; ++a) cnt[grp.empty() ? 0 : grp[a]]++;
    d_hmg.alloc(2 * ((size_t)K + 1) * G * sizeof(double));
    d_hsum.alloc(2 * ((size_t)K + 1) * G * sizeof(double));
    h_mg.assign(2 * ((size_t)K + 1) * G, 0.0);
    h_hs.assign(2 * ((size_t)K + 1) * G, 0.0);
    if (!grp.empty()) {
        ensure_group_lists();
        grp_bytes = G <= 0x100u ? 1 : G <= 0x10000u ? 2 : 4;
        const std::vector<uint8_t> g8(grp_bytes == 1 ? grp.begin() : grp.end(), grp.end());
        const std::vector<uint16_t> g16(grp_bytes == 2 ? grp.begin() : grp.end(), grp.end());
        if (grp_bytes == 1)
            upload(d_grp, g8, st);
        else if (grp_bytes == 2)
            upload(d_grp, g16, st);
        else
            upload(d_grp, grp, st);
        HIPCHK(hipStreamSynchronize(st));  // the narrowed copies are locals
        d_lm.alloc(2 * ((size_t)K + 1) * G * sizeof(double));
        h_lm.assign(2 * ((size_t)K + 1) * G, 0.0);
    }
    d_scratch.alloc(((nl + 255) / 256 / 1024 + 16) * 2 * sizeof(double));
    w_mu.assign(G, 0.0);
    v_mu.assign((size_t)G * K, 0.0);
    // fm_learn_mcmc::init (:1099-1116) and the -regular values (libfm.cpp:484-521): per group
    w_lambda.assign(G, c.regw);
    v_lambda.assign((size_t)G * K, c.regv);
    for (uint32_t q = 0; q < G && !greg_w.empty(); ++q) {
        w_lambda[q] = greg_w[q];
        std::fill(v_lambda.begin() + (size_t)q * K, v_lambda.begin() + (size_t)(q + 1) * K, greg_v[q]);
    }
    // model init and the starting predictions (fm_learn_mcmc_simultaneous.h:75-93)
    std::vector<double> h_w, h_v;  // host copies for the upload only
    if (c.rng_mode == SBMF_RNG_REFERENCE) {
        grand.seed_((unsigned)c.seed);  // libfm.cpp:124 srand(time) -- here the pinned seed
        init_model(grand, h_w, h_v);
    } else {
        PhiloxStream ps(c.seed, 0xffffffffu, TAG_FMC_INIT);
        init_model(ps, h_w, h_v);
    }
    HIPCHK(hipMemcpyAsync(d_w.p, h_w.data(), (size_t)p * sizeof(double), hipMemcpyHostToDevice, st));
    if (K) HIPCHK(hipMemcpyAsync(d_v.p, h_v.data(), h_v.size() * sizeof(double), hipMemcpyHostToDevice, st));
    predict_train();
    HIPCHK(hipStreamSynchronize(st));
    for (auto& e : ev) event_create(&e);
}

// fm_learn_mcmc::predict (:357-380): the running sum over the iterations run
// (MCMC) or the last prediction (ALS), clamped to the train range -- in classification the
// probabilities, clipped to [0, 1]
void FMChain::predict_out(double* out) {
    HIPCHK(hipStreamSynchronize(st));
    if (!T) return;
    HIPCHK(hipMemcpy(out, (do_sample ? d_sum : d_pthis).p, T * sizeof(double), hipMemcpyDeviceToHost));
    for (uint64_t t = 0; t < T; ++t) {
        double o = do_sample ? out[t] / std::max(1u, it) : out[t];
        o = std::min(classify() ? 1.0 : hi, o);
        o = std::max(classify() ? 0.0 : lo, o);
        out[t] = o;
    }
}

void FMChain::hyper_out(double* h4k, double* alpha_out) {
    if (h4k) {
        if (G > 1) fail(SBMF_E_STATE, "sbmf_get_hyper: this context has %u attribute groups; read them with sbmf_get_fm_groups", G);
        std::fill(h4k, h4k + 4 * (size_t)K, 0.0);
        std::copy(v_lambda.begin(), v_lambda.end(), h4k);
        std::copy(v_mu.begin(), v_mu.end(), h4k + K);
        h4k[2 * K] = w_lambda[0];
        if (K > 1) h4k[2 * K + 1] = w_mu[0];
    }
    if (alpha_out) *alpha_out = alpha;
}

void FMChain::model(double* w0_out, double* w, double* v) {
    HIPCHK(hipStreamSynchronize(st));
    if (w0_out) *w0_out = w0;
    if (w) HIPCHK(hipMemcpy(w, d_w.p, (size_t)p * sizeof(double), hipMemcpyDeviceToHost));
    if (v && K) HIPCHK(hipMemcpy(v, d_v.p, (size_t)K * p * sizeof(double), hipMemcpyDeviceToHost));
}

// items past libFM's attribute count (sbmf_set_dims with trailing unrated ids) have no factors and no bias: 0
void FMChain::factors(double* U, double* V) {
    if (!I) fail(SBMF_E_STATE, "a context given cases has no user / item tables: read the model with sbmf_get_fm");
    std::vector<double> h((size_t)K * p);
    model(nullptr, nullptr, h.data());
    for (uint32_t f = 0; f < K; ++f) {
        if (U)
            for (uint32_t a = 0; a < I; ++a) U[(size_t)a * K + f] = h[(size_t)f * p + a];
        if (V)
            for (uint32_t a = 0; a < J; ++a) V[(size_t)a * K + f] = I + a < p ? h[(size_t)f * p + I + a] : 0.0;
    }
}

void FMChain::biases(double* bu, double* bv, double* b0) {
    if (!I) fail(SBMF_E_STATE, "a context given cases has no user / item biases: read the model with sbmf_get_fm");
    std::vector<double> h(p);
    model(b0, h.data(), nullptr);
    if (bu) std::copy(h.begin(), h.begin() + I, bu);
    if (bv)
        for (uint32_t a = 0; a < J; ++a) bv[a] = I + a < p ? h[I + a] : 0.0;
}

void fm_long_bounds(uint32_t& longb, uint32_t& chunk) {
    longb = chunk = 4096;
    if (const char* e = std::getenv("SBMF_FMM_LONG")) longb = (uint32_t)std::max(256, std::atoi(e));
    if (const char* e = std::getenv("SBMF_FMM_CHUNK")) chunk = (uint32_t)std::max(0, std::atoi(e));
}

void fm_bin_rows(const std::vector<uint32_t>& ptr, uint32_t r0, uint32_t r1, uint32_t longb, std::vector<uint32_t> b[3]) {
    for (uint32_t k = r0; k < r1; ++k) {
        const uint32_t len = ptr[k + 1] - ptr[k];
        b[len <= 256 ? 0 : len <= longb ? 1 : 2].push_back(k);
    }
    for (int j = 0; j < 3; ++j)
        std::stable_sort(b[j].begin(), b[j].end(),
                         [&](uint32_t x, uint32_t y) { return ptr[x + 1] - ptr[x] > ptr[y + 1] - ptr[y]; });
}

void fm_cut_chunks(const std::vector<uint32_t>& ptr, const uint32_t* rows, uint32_t nrows, uint32_t chunk,
                   std::vector<uint4>& chunks, std::vector<uint32_t>& cfirst) {
    const uint32_t first = (uint32_t)chunks.size();
    cfirst.push_back(0);
    for (uint32_t i = 0; i < nrows; ++i) {
        const uint32_t r = rows[i], c0 = ptr[r], len = ptr[r + 1] - c0;
        const uint32_t nch = (len + chunk - 1) / chunk;
        for (uint32_t c = 0; c < nch; ++c) {
            const uint32_t cb = c0 + (uint32_t)((uint64_t)len * c / nch);
            const uint32_t ce = c0 + (uint32_t)((uint64_t)len * (c + 1) / nch);
            chunks.push_back(make_uint4(r, cb, ce - cb, i));
        }
        cfirst.push_back((uint32_t)chunks.size() - first);
    }
}

}  // namespace sbmf
