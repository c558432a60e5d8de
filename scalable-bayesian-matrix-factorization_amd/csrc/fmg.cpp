// fmg.cpp -- host side of the general libFM MCMC / ALS learner (fmg.h): the reference's
// fm_learn_mcmc chain (fm_learn_mcmc.h:411-623, fm_learn_mcmc_simultaneous.h:96-245) on
// cases with any number of features.
//
// Per iteration, in libFM's order:
//   1. alpha, w0                                  (device sums over the e of the cache, host draws)
//   2. w group hyperparameters (host), then every w: range by range, bin by bin
//   3. v group hyperparameters of every factor (host), then per factor f: the cache's q
//      (k_fmg_q), and every v[f][.] range by range
//   4. re-predict train (e = prediction - target, q = 0) and test
// The host draws the scalars and, in reference RNG mode, the one normal per attribute of the
// w and v passes in libFM's consumption order (as fmm.cpp does for the two-attribute learner);
// Philox mode fills them on the device.  ALS draws nothing.
#include "fmg.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "common.h"
#include "fmm.h"
#include "kernels.h"
#include "rng.h"

namespace sbmf {

enum : uint32_t { TAG_FMG_W = 8, TAG_FMG_V = 9, TAG_FMG_INIT = 10 };  // the two-attribute learner's streams

// The greedy cut of sbmf_fm_ranges: ascending ids, per case the start of the last range
// that touched it; a new range opens at the first attribute with a case the current one holds.
void fm_ranges(const sbmf_cases& tr, uint32_t p, std::vector<uint32_t>& bounds) {
    bounds.assign(1, 0);
    if (p == 0) return;
    // attribute-major lists of cases (counting sort)
    std::vector<uint64_t> ap((size_t)p + 1, 0);
    for (uint64_t k = 0; k < tr.nnz; ++k) ap[tr.attr[k] + 1]++;
    for (uint32_t a = 0; a < p; ++a) ap[a + 1] += ap[a];
    std::vector<uint32_t> cs(tr.nnz);
    {
        std::vector<uint64_t> fill(ap.begin(), ap.end() - 1);
        for (uint64_t c = 0; c < tr.n; ++c)
            for (uint64_t k = tr.ptr[c]; k < tr.ptr[c + 1]; ++k) cs[fill[tr.attr[k]]++] = (uint32_t)c;
    }
    std::vector<uint32_t> last(tr.n, 0xffffffffu);
    uint32_t start = 0;
    for (uint32_t a = 0; a < p; ++a) {
        bool hit = false;
        for (uint64_t k = ap[a]; k < ap[a + 1] && !hit; ++k) hit = last[cs[k]] == start;
        if (hit) {
            start = a;
            bounds.push_back(a);
        }
        for (uint64_t k = ap[a]; k < ap[a + 1]; ++k) last[cs[k]] = start;
    }
    bounds.push_back(p);
}

// One launch of a pass: rows [r0, r0 + nrows) of d_rows with tpr threads each, or the long rows
// of a range in chunks
struct FGLaunch {
    uint32_t r0 = 0, nrows = 0;
    int tpr = 64;
    // chunked: chunks [c0, c0 + nchunks), long-row slots from l0, the rows' chunk offsets from f0
    uint32_t c0 = 0, nchunks = 0, l0 = 0, f0 = 0;
};

struct FGLearner {
    sbmf_config cfg{};
    uint32_t K = 0, Kp = 0, p = 0, nranges = 0;
    uint64_t N = 0, T = 0;
    int k0 = 1, k1 = 1, do_sample = 1, do_multilevel = 1;
    double lo = 1.0, hi = 5.0;
    double alpha = 1.0, w0 = 0.0, w_mu = 0.0, w_lambda = 0.0;
    std::vector<double> v_mu, v_lambda;
    uint32_t it = 0, n_launch = 0;
    GlibcRand grand{1};
    hipStream_t st = nullptr;
    hipEvent_t ev[3] = {};
    std::vector<FGLaunch> launches;
    DBuf d_rows, d_chunks, d_cfirst, d_csums, d_cdelta;
    DBuf d_cptr, d_cattr, d_cx, d_y, d_aptr, d_ent, d_eq;
    DBuf d_tptr, d_tattr, d_tx, d_ty, d_pthis, d_sum;
    DBuf d_w, d_v, d_vT, d_zw, d_zv, d_part, d_tpart, d_res, d_scratch, d_hmg, d_hsum;
    std::vector<double> h_mg, h_hs;

    ~FGLearner() {
        for (auto& e : ev) event_destroy(e);
    }

    template <class G>
    double gaussian(G& g, double mean, double stdev) {  // random.h:166-172
        if (stdev == 0.0 || std::isnan(stdev)) return mean;
        return mean + stdev * leva_normal(g);
    }
    // fm_learn_mcmc.h:951-1009 (one group: every attribute); the sums from k_fmm_hsums
    template <class G>
    void draw_hyper_w(G& g) {
        const double alpha_0 = 1.0, beta_0 = 1.0, mu_0 = 0.0;
        if (!do_multilevel) {
            w_mu = mu_0;
            return;
        }
        const double gm = h_hs[2 * K];
        const double a = alpha_0 + p + 1;
        const double old = w_lambda;
        w_lambda = do_sample ? mt_gamma(g, a / 2.0) / (gm / 2.0) : a / gm;
        if (std::isnan(w_lambda) || std::isinf(w_lambda)) w_lambda = old;
        double m = h_hs[2 * K + 1];
        m = (m + beta_0 * mu_0) / (p + beta_0);
        const double s2 = 1.0 / ((p + beta_0) * w_lambda);
        const double om = w_mu;
        w_mu = do_sample ? gaussian(g, m, std::sqrt(s2)) : m;
        if (std::isnan(w_mu) || std::isinf(w_mu)) w_mu = om;
    }
    // fm_learn_mcmc.h:1011-1089 (a NaN / inf ends that draw's factor loop)
    template <class G>
    void draw_hyper_v(G& g) {
        const double alpha_0 = 1.0, beta_0 = 1.0, mu_0 = 0.0;
        if (!do_multilevel) {
            std::fill(v_mu.begin(), v_mu.end(), mu_0);
            return;
        }
        for (uint32_t f = 0; f < K; ++f) {
            const double gm = h_hs[2 * f];
            const double a = alpha_0 + p + 1;
            const double old = v_lambda[f];
            v_lambda[f] = do_sample ? mt_gamma(g, a / 2.0) / (gm / 2.0) : a / gm;
            if (std::isnan(v_lambda[f]) || std::isinf(v_lambda[f])) {
                v_lambda[f] = old;
                break;
            }
        }
        for (uint32_t f = 0; f < K; ++f) {
            double m = h_hs[2 * f + 1];
            m = (m + beta_0 * mu_0) / (p + beta_0);
            const double s2 = 1.0 / ((p + beta_0) * v_lambda[f]);
            const double old = v_mu[f];
            v_mu[f] = do_sample ? gaussian(g, m, std::sqrt(s2)) : m;
            if (std::isnan(v_mu[f]) || std::isinf(v_mu[f])) {
                v_mu[f] = old;
                break;
            }
        }
    }

    // every launch of one pass, ranges ascending
    void run_pass(FGPassArgs a, bool vpass) {
        a.aptr = d_aptr.as<uint32_t>();
        a.ent = d_ent.as<uint2>();
        a.eq = d_eq.as<double2>();
        a.alpha = alpha;
        a.do_sample = do_sample;
        for (const FGLaunch& l : launches) {
            a.rows = d_rows.as<uint32_t>() + l.r0;
            a.nrows = l.nrows;
            a.xmode = 0;
            a.chunks = nullptr;
            if (l.nchunks) {
                // the chunks' sums, the draw per row (chunk sums in chunk order), every chunk's update
                FGPassArgs c = a;
                c.chunks = d_chunks.as<uint4>() + l.c0;
                c.nrows = l.nchunks;
                c.xmode = 1;
                c.sums = d_csums.as<double2>() + l.c0;
                HIPCHK(vpass ? fmg_vpass(c, l.tpr, st) : fmg_wpass(c, l.tpr, st));
                HIPCHK(fmg_chunk_draw(a, a.rows, d_cfirst.as<uint32_t>() + l.f0, l.nrows,
                                      d_csums.as<double2>() + l.c0, vpass ? 1 : 0, d_cdelta.as<double4>() + l.l0, st));
                c.xmode = 2;
                c.delta = d_cdelta.as<double4>() + l.l0;
                HIPCHK(vpass ? fmg_vpass(c, l.tpr, st) : fmg_wpass(c, l.tpr, st));
                n_launch += 3;
                continue;
            }
            HIPCHK(vpass ? fmg_vpass(a, l.tpr, st) : fmg_wpass(a, l.tpr, st));
            ++n_launch;
        }
    }

    FGPredictArgs predict_args(bool train) {
        FGPredictArgs a{};
        a.cptr = (train ? d_cptr : d_tptr).as<uint32_t>();
        a.cattr = (train ? d_cattr : d_tattr).as<uint32_t>();
        a.cx = (train ? d_cx : d_tx).as<float>();
        a.y = (train ? d_y : d_ty).as<float>();
        a.n = train ? N : T;
        a.vT = d_vT.as<double>();
        a.w = d_w.as<double>();
        a.w0 = w0;
        a.K = K;
        a.Kp = Kp;
        a.k0 = k0;
        a.k1 = k1;
        a.lo = lo;
        a.hi = hi;
        return a;
    }
    void predict_train() {
        HIPCHK(fmm_transpose(d_v.as<double>(), d_vT.as<double>(), K, Kp, p, st));
        HIPCHK(fmg_predict_train(predict_args(true), d_eq.as<double2>(), d_part.as<double>(), st));
        n_launch += 2;
    }

    template <class G>
    void sweep_draws(G& g) {
        double* res = d_res.as<double>();
        const bool ref = cfg.rng_mode == SBMF_RNG_REFERENCE;
        // ---- alpha and w0 (fm_learn_mcmc.h:901-929, :627-668)
        const uint64_t nb = (N + 1023) / 1024;
        double s[2];
        HIPCHK(fmg_esums(d_eq.as<double2>(), N, w0, d_part.as<double>(), st));
        HIPCHK(launch_sum_cols(d_part.as<double>(), (uint32_t)nb, 2, res, st));
        HIPCHK(hipMemcpyAsync(s, res, sizeof s, hipMemcpyDeviceToHost, st));
        if (do_multilevel) {
            // the hyperparameter draws' column sums (:951-1089) on the device, in the host loops' order
            const double beta_0 = 1.0, gamma_0 = 1.0, mu_0 = 0.0;
            for (uint32_t c = 0; c <= K; ++c) {
                const double mu = c < K ? v_mu[c] : w_mu;
                h_mg[2 * c] = mu;
                h_mg[2 * c + 1] = beta_0 * (mu - mu_0) * (mu - mu_0) + gamma_0;
            }
            HIPCHK(hipMemcpyAsync(d_hmg.p, h_mg.data(), h_mg.size() * sizeof(double), hipMemcpyHostToDevice, st));
            HIPCHK(fmm_hsums(d_v.as<double>(), d_w.as<double>(), p, K, d_hmg.as<double2>(), d_hsum.as<double2>(), st));
            HIPCHK(hipMemcpyAsync(h_hs.data(), d_hsum.p, h_hs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
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
                HIPCHK(fmg_shift(d_eq.as<double2>(), N, old - w0, st));
                ++n_launch;
            }
        }
        // ---- w (:422-457): group hyperparameters, then every attribute in ascending ranges
        if (k1) {
            draw_hyper_w(g);
            if (do_sample) {
                if (ref) {
                    std::vector<double> z(p);
                    for (uint32_t a = 0; a < p; ++a) z[a] = leva_normal(g);
                    HIPCHK(hipMemcpyAsync(d_zw.p, z.data(), p * sizeof(double), hipMemcpyHostToDevice, st));
                    HIPCHK(hipStreamSynchronize(st));  // z is a local
                } else {
                    HIPCHK(launch_philox_fill<double>(d_zw.as<double>(), 1, 0, p, cfg.seed, it, TAG_FMG_W, st));
                }
            }
            FGPassArgs a{};
            a.own = d_w.as<double>();
            a.z = d_zw.as<double>();
            a.zs = 1;
            a.zoff = 0;
            a.mu = w_mu;
            a.lambda = w_lambda;
            run_pass(a, false);
        }
        // ---- v (:497-577): per factor the cache's q, then every attribute in ascending ranges
        if (K) {
            draw_hyper_v(g);
            if (do_sample) {
                if (ref) {
                    std::vector<double> z((size_t)p * K);  // [a][K], drawn f-major (the reference's order)
                    for (uint32_t f = 0; f < K; ++f)
                        for (uint32_t a = 0; a < p; ++a) z[(size_t)a * K + f] = leva_normal(g);
                    HIPCHK(hipMemcpyAsync(d_zv.p, z.data(), z.size() * sizeof(double), hipMemcpyHostToDevice, st));
                    HIPCHK(hipStreamSynchronize(st));
                } else {
                    HIPCHK(launch_philox_fill<double>(d_zv.as<double>(), K, 0, p, cfg.seed, it, TAG_FMG_V, st));
                }
            }
            for (uint32_t f = 0; f < K; ++f) {
                double* col = d_v.as<double>() + (size_t)f * p;
                HIPCHK(fmg_q(d_cptr.as<uint32_t>(), d_cattr.as<uint32_t>(), d_cx.as<float>(), N, col,
                             d_eq.as<double2>(), st));
                ++n_launch;
                FGPassArgs a{};
                a.own = col;
                a.z = d_zv.as<double>();
                a.zs = K;
                a.zoff = f;
                a.mu = v_mu[f];
                a.lambda = v_lambda[f];
                run_pass(a, true);
            }
        }
    }

    void run(uint32_t iters, sbmf_sweep_cb cb, void* user) {
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
            // ---- predict train and test, evaluate (fm_learn_mcmc_simultaneous.h:134-245)
            predict_train();
            HIPCHK(launch_sum(d_part.as<double>(), (N + 255) / 256, res + 2, d_scratch.as<double>(), st));
            const uint64_t tb = (T + 255) / 256;
            if (T) {
                HIPCHK(fmg_predict_test(predict_args(false), (double)(it + 1), d_pthis.as<double>(), d_sum.as<double>(),
                                        d_tpart.as<double>(), st));
                HIPCHK(launch_sum_cols(d_tpart.as<double>(), (uint32_t)tb, 2, res + 3, st));
                n_launch += 2;
            }
            HIPCHK(hipEventRecord(ev[2], st));
            double h[3] = {0, 0, 0};
            HIPCHK(hipMemcpyAsync(h, res + 2, sizeof h, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            float ms0 = 0.f, ms1 = 0.f;
            HIPCHK(hipEventElapsedTime(&ms0, ev[0], ev[1]));
            HIPCHK(hipEventElapsedTime(&ms1, ev[1], ev[2]));
            sbmf_sweep_info info{};
            info.sweep = it;
            info.collected = 1;
            info.rmse_train = std::sqrt(h[0] / (double)N);
            info.rmse_avg = T ? std::sqrt(h[1] / (double)T) : NAN;
            info.rmse_this = T ? std::sqrt(h[2] / (double)T) : NAN;
            info.tau = alpha;
            info.ms_sweep = ms0;
            info.ms_eval = ms1;
            ++it;
            if (cb && cb(&info, user)) break;
        }
    }
};

// The cases in the order of their first (smallest) attribute, file order within it (cases without
// features last): the records {e, q} follow the cases, so the passes of that attribute's field
// -- the users of a users-first file -- read and write them front to back instead of one memory
// line per case.  The order of the cases is a labelling: no draw depends on it.
struct OrderedCases {
    std::vector<uint64_t> ptr;
    std::vector<uint32_t> attr;
    std::vector<float> x, y;
    bool build(const sbmf_cases& in, sbmf_cases& out) {
        auto key = [&](uint64_t c) { return in.ptr[c + 1] > in.ptr[c] ? in.attr[in.ptr[c]] : in.num_attr; };
        bool sorted = true;
        for (uint64_t c = 1; c < in.n && sorted; ++c) sorted = key(c - 1) <= key(c);
        if (sorted) return false;
        std::vector<uint64_t> pos((size_t)in.num_attr + 2, 0);
        for (uint64_t c = 0; c < in.n; ++c) pos[key(c) + 1]++;
        for (size_t k = 0; k + 1 < pos.size(); ++k) pos[k + 1] += pos[k];
        std::vector<uint32_t> order(in.n);
        for (uint64_t c = 0; c < in.n; ++c) order[pos[key(c)]++] = (uint32_t)c;
        ptr.assign(in.n + 1, 0);
        attr.resize(in.nnz);
        x.resize(in.nnz);
        y.resize(in.n);
        uint64_t at = 0;
        for (uint64_t k = 0; k < in.n; ++k) {
            const uint64_t c = order[k], b = in.ptr[c], m = in.ptr[c + 1] - b;
            ptr[k] = at;
            std::copy(in.attr + b, in.attr + b + m, attr.begin() + at);
            std::copy(in.x + b, in.x + b + m, x.begin() + at);
            y[k] = in.target[c];
            at += m;
        }
        ptr[in.n] = at;
        out = in;
        out.ptr = ptr.data();
        out.attr = attr.data();
        out.x = x.data();
        out.target = y.data();
        return true;
    }
};

FGLearner* fmg_create(const sbmf_config& c, const sbmf_cases& tr_file, const sbmf_cases& te, hipStream_t st) {
    if (tr_file.n == 0) fail(SBMF_E_STATE, "no training cases");
    if (tr_file.n >= 0xffffffffull || te.n >= 0xffffffffull || tr_file.nnz >= 0xffffffffull || te.nnz >= 0xffffffffull)
        fail(SBMF_E_ARG, "more than 2^32-1 cases or features are not supported");
    OrderedCases oc;
    sbmf_cases tr_ordered{};
    const sbmf_cases& tr = oc.build(tr_file, tr_ordered) ? tr_ordered : tr_file;
    std::unique_ptr<FGLearner> L(new FGLearner());
    L->cfg = c;
    L->st = st;
    L->K = c.num_factor;
    L->Kp = (L->K + 15) / 16 * 16;
    L->N = tr.n;
    L->T = te.n;
    L->k0 = (c.libfm_dim & 1u) ? 1 : 0;
    L->k1 = (c.libfm_dim & 2u) ? 1 : 0;
    const bool als = c.method == SBMF_METHOD_ALS;
    L->do_sample = als ? 0 : 1;  // libfm.cpp:132-136
    L->do_multilevel = als ? 0 : 1;
    // num_all_attribute = max(train, test num_feature) + 1 (libfm.cpp:328)
    if (std::max(tr.num_attr, te.num_attr) >= 0xfffffffeu) fail(SBMF_E_ARG, "attribute id too large");
    L->p = std::max(tr.num_attr, te.num_attr) + 1;
    const uint32_t p = L->p, K = L->K;
    // the train target range (Data.h:200-203)
    float mn = 3.4028234663852886e38f, mx = -3.4028234663852886e38f;
    for (uint64_t x = 0; x < tr.n; ++x) {
        mn = std::min(tr.target[x], mn);
        mx = std::max(tr.target[x], mx);
    }
    L->lo = mn;
    L->hi = mx;
    // ---- the ranges (SBMF_FMG_SERIAL=1: one attribute per range, literally libFM's loop)
    std::vector<uint32_t> bounds;
    const char* ser = std::getenv("SBMF_FMG_SERIAL");
    if (ser && std::atoi(ser) != 0) {
        bounds.resize((size_t)p + 1);
        for (uint32_t a = 0; a <= p; ++a) bounds[a] = a;
    } else {
        fm_ranges(tr, p, bounds);
    }
    L->nranges = (uint32_t)bounds.size() - 1;
    // ---- the attribute-major copy (libFM's data_t): cases ascending within an attribute
    std::vector<uint32_t> aptr((size_t)p + 1, 0);
    for (uint64_t k = 0; k < tr.nnz; ++k) aptr[tr.attr[k] + 1]++;
    for (uint32_t a = 0; a < p; ++a) aptr[a + 1] += aptr[a];
    std::vector<uint2> ent(tr.nnz);
    {
        std::vector<uint32_t> fill(aptr.begin(), aptr.end() - 1);
        for (uint64_t cs = 0; cs < tr.n; ++cs)
            for (uint64_t k = tr.ptr[cs]; k < tr.ptr[cs + 1]; ++k) {
                uint32_t xb;
                std::memcpy(&xb, &tr.x[k], 4);
                ent[fill[tr.attr[k]]++] = make_uint2((uint32_t)cs, xb);
            }
    }
    // ---- launches: per range, rows binned by length (<= 256 entries 64 threads, <= longb 256,
    // longer 1024 or in chunks), longest first within a bin.  The bin of a row depends on its
    // length alone, so its sums have the same order under any partition into ranges.
    uint32_t longb = 4096, chunk = 4096;
    if (const char* e = std::getenv("SBMF_FMM_LONG")) longb = (uint32_t)std::max(256, std::atoi(e));
    if (const char* e = std::getenv("SBMF_FMM_CHUNK")) chunk = (uint32_t)std::max(0, std::atoi(e));
    std::vector<uint32_t> rows, cfirst;
    std::vector<uint4> chunks;
    uint32_t nlong = 0;
    rows.reserve(p);
    for (uint32_t r = 0; r + 1 < bounds.size(); ++r) {
        std::vector<uint32_t> b[3];
        for (uint32_t a = bounds[r]; a < bounds[r + 1]; ++a) {
            const uint32_t len = aptr[a + 1] - aptr[a];
            b[len <= 256 ? 0 : len <= longb ? 1 : 2].push_back(a);
        }
        for (int j = 2; j >= 0; --j) {  // the long rows first: they set the range's tail
            if (b[j].empty()) continue;
            std::stable_sort(b[j].begin(), b[j].end(), [&](uint32_t x, uint32_t y) {
                return aptr[x + 1] - aptr[x] > aptr[y + 1] - aptr[y];
            });
            FGLaunch l;
            l.r0 = (uint32_t)rows.size();
            l.nrows = (uint32_t)b[j].size();
            l.tpr = j == 0 ? 64 : j == 1 ? 256 : 1024;
            rows.insert(rows.end(), b[j].begin(), b[j].end());
            if (j == 2 && chunk) {
                l.c0 = (uint32_t)chunks.size();
                l.l0 = nlong;
                // cfirst: per launch nrows + 1 offsets relative to the launch's first chunk
                l.f0 = (uint32_t)cfirst.size();
                cfirst.push_back(0);
                for (uint32_t i = 0; i < l.nrows; ++i) {
                    const uint32_t a = b[j][i], c0 = aptr[a], len = aptr[a + 1] - c0;
                    const uint32_t nch = (len + chunk - 1) / chunk;
                    for (uint32_t cc = 0; cc < nch; ++cc) {
                        const uint32_t cb = c0 + (uint32_t)((uint64_t)len * cc / nch);
                        const uint32_t ce = c0 + (uint32_t)((uint64_t)len * (cc + 1) / nch);
                        chunks.push_back(make_uint4(a, cb, ce - cb, i));
                    }
                    cfirst.push_back((uint32_t)chunks.size() - l.c0);
                }
                l.nchunks = (uint32_t)chunks.size() - l.c0;
                nlong += l.nrows;
            }
            L->launches.push_back(l);
        }
    }
    upload(L->d_rows, rows, st);
    upload(L->d_chunks, chunks, st);
    upload(L->d_cfirst, cfirst, st);
    L->d_csums.alloc(std::max<size_t>(chunks.size(), 1) * sizeof(double2));
    L->d_cdelta.alloc(std::max<size_t>(nlong, 1) * sizeof(double4));
    // ---- the case-major copies
    auto up_cases = [&](const sbmf_cases& cs, DBuf& dp, DBuf& da, DBuf& dx, DBuf& dy) {
        std::vector<uint32_t> ptr(cs.n + 1, 0);
        for (uint64_t x = 0; x <= cs.n && cs.ptr; ++x) ptr[x] = (uint32_t)cs.ptr[x];
        upload(dp, ptr, st);
        HIPCHK(hipStreamSynchronize(st));  // ptr is a local
        da.alloc(std::max<uint64_t>(cs.nnz, 1) * sizeof(uint32_t));
        dx.alloc(std::max<uint64_t>(cs.nnz, 1) * sizeof(float));
        dy.alloc(std::max<uint64_t>(cs.n, 1) * sizeof(float));
        if (cs.nnz) {
            HIPCHK(hipMemcpy(da.p, cs.attr, cs.nnz * sizeof(uint32_t), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(dx.p, cs.x, cs.nnz * sizeof(float), hipMemcpyHostToDevice));
        }
        if (cs.n) HIPCHK(hipMemcpy(dy.p, cs.target, cs.n * sizeof(float), hipMemcpyHostToDevice));
    };
    up_cases(tr, L->d_cptr, L->d_cattr, L->d_cx, L->d_y);
    up_cases(te, L->d_tptr, L->d_tattr, L->d_tx, L->d_ty);
    upload(L->d_aptr, aptr, st);
    upload(L->d_ent, ent, st);
    const uint64_t n = tr.n, nt = te.n;
    L->d_eq.alloc(n * sizeof(double2));
    L->d_w.alloc((size_t)p * sizeof(double));
    L->d_v.alloc(std::max<size_t>((size_t)K * p, 1) * sizeof(double));
    L->d_vT.alloc(std::max<size_t>((size_t)p * L->Kp, 1) * sizeof(double));
    HIPCHK(hipMemsetAsync(L->d_vT.p, 0, L->d_vT.bytes, st));
    L->d_zw.alloc((size_t)p * sizeof(double));
    L->d_zv.alloc(std::max<size_t>((size_t)K * p, 1) * sizeof(double));
    L->d_pthis.alloc(std::max<uint64_t>(nt, 1) * sizeof(double));
    L->d_sum.alloc(std::max<uint64_t>(nt, 1) * sizeof(double));
    HIPCHK(hipMemsetAsync(L->d_sum.p, 0, L->d_sum.bytes, st));
    L->d_part.alloc((std::max<uint64_t>((n + 255) / 256, 2 * ((n + 1023) / 1024)) + 2) * sizeof(double));
    L->d_tpart.alloc((2 * ((nt + 255) / 256) + 2) * sizeof(double));
    L->d_res.alloc(8 * sizeof(double));
    L->d_hmg.alloc(2 * ((size_t)K + 1) * sizeof(double));
    L->d_hsum.alloc(2 * ((size_t)K + 1) * sizeof(double));
    L->h_mg.assign(2 * ((size_t)K + 1), 0.0);
    L->h_hs.assign(2 * ((size_t)K + 1), 0.0);
    L->d_scratch.alloc(((n + 255) / 256 / 1024 + 16) * 2 * sizeof(double));
    L->v_mu.assign(K, 0.0);
    // fm_learn_mcmc::init (:1099-1116) and the -regular values (libfm.cpp:484-513)
    L->w_lambda = c.regw;
    L->v_lambda.assign(K, c.regv);
    // fm_model::init (fm_model.h:87-96: v, f-major) then w (libfm.cpp:412)
    std::vector<double> h_v((size_t)K * p), h_w(p);
    const double sd = c.init_stdev >= 0 ? c.init_stdev : 0.1;
    auto init = [&](auto& g) {
        for (size_t x = 0; x < h_v.size(); ++x) h_v[x] = L->gaussian(g, 0.0, sd);
        for (uint32_t a = 0; a < p; ++a) h_w[a] = L->gaussian(g, 0.0, sd);
    };
    if (c.rng_mode == SBMF_RNG_REFERENCE) {
        L->grand.seed_((unsigned)c.seed);  // libfm.cpp:124 srand(time) -- here the pinned seed
        init(L->grand);
    } else {
        PhiloxStream ps(c.seed, 0xffffffffu, TAG_FMG_INIT);
        init(ps);
    }
    HIPCHK(hipMemcpyAsync(L->d_w.p, h_w.data(), (size_t)p * sizeof(double), hipMemcpyHostToDevice, st));
    if (K) HIPCHK(hipMemcpyAsync(L->d_v.p, h_v.data(), h_v.size() * sizeof(double), hipMemcpyHostToDevice, st));
    // the starting predictions (fm_learn_mcmc_simultaneous.h:75-93)
    L->predict_train();
    HIPCHK(hipStreamSynchronize(st));
    L->n_launch = 0;
    for (auto& e : L->ev) event_create(&e);
    return L.release();
}

void fmg_destroy(FGLearner* L) { delete L; }
void fmg_run(FGLearner* L, uint32_t iters, sbmf_sweep_cb cb, void* user) { L->run(iters, cb, user); }

// fm_learn_mcmc::predict (:357-380)
void fmg_predict_out(FGLearner* L, double* out) {
    HIPCHK(hipStreamSynchronize(L->st));
    if (!L->T) return;
    HIPCHK(hipMemcpy(out, (L->do_sample ? L->d_sum : L->d_pthis).p, L->T * sizeof(double), hipMemcpyDeviceToHost));
    for (uint64_t t = 0; t < L->T; ++t) {
        double o = L->do_sample ? out[t] / std::max(1u, L->it) : out[t];
        o = std::min(L->hi, o);
        o = std::max(L->lo, o);
        out[t] = o;
    }
}
void fmg_model(FGLearner* L, double* w0, double* w, double* v) {
    HIPCHK(hipStreamSynchronize(L->st));
    if (w0) *w0 = L->w0;
    if (w) HIPCHK(hipMemcpy(w, L->d_w.p, (size_t)L->p * sizeof(double), hipMemcpyDeviceToHost));
    if (v && L->K) HIPCHK(hipMemcpy(v, L->d_v.p, (size_t)L->K * L->p * sizeof(double), hipMemcpyDeviceToHost));
}
void fmg_hyper_out(FGLearner* L, double* h4k, double* alpha) {
    const uint32_t K = L->K;
    if (h4k) {
        std::fill(h4k, h4k + 4 * (size_t)K, 0.0);
        std::copy(L->v_lambda.begin(), L->v_lambda.end(), h4k);
        std::copy(L->v_mu.begin(), L->v_mu.end(), h4k + K);
        h4k[2 * K] = L->w_lambda;
        if (K > 1) h4k[2 * K + 1] = L->w_mu;
    }
    if (alpha) *alpha = L->alpha;
}
uint32_t fmg_launches(const FGLearner* L) { return L->n_launch; }
uint32_t fmg_num_attribute(const FGLearner* L) { return L->p; }
uint32_t fmg_num_ranges(const FGLearner* L) { return L->nranges; }

}  // namespace sbmf
