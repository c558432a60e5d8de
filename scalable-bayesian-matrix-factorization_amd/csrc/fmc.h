// fmc.h -- the host side of libFM's MCMC / ALS chain (fm_learn_mcmc.h:411-623 draw_all,
// fm_learn_mcmc_simultaneous.h:96-245), written once for the two data layouts: the
// two-attribute learner (fmm.cpp: one user and one item per case, several ranks) and the
// general one (fmg.cpp: cases with any number of features, exact by ranges).
//
// Per iteration, in libFM's order:
//   1. alpha ~ Gamma((alpha_0 + N)/2, (gamma_0 + sum e^2)/2)          (device sums, host draw)
//   2. w0 ~ N(...), e -= w0_old - w0                                    (device sum, host draw)
//   3. w group hyperparameters (host, sums on the device), then every w (the layout's pass)
//   4. v group hyperparameters of every factor (host), then per factor f every v[f][.]
//   5. re-predict train and test, running-mean test RMSE
// With attribute groups (libFM's -meta; the general learner only) steps 3 and 4 draw one set of
// hyperparameters per group, group by group in libFM's order, and every attribute is drawn
// from its own group's prior.
// Reference RNG mode replays the reference's glibc rand() stream draw for draw (rng.h): the
// host draws the scalars in consumption order and fills the one normal per attribute of the w
// and v passes ahead of the launches.  Philox mode fills those normals on the device.  ALS
// (do_sample = do_multilevel = 0) draws nothing: alpha = 1, the draws take their posterior means.
//
// Classification (cfg.task, libFM's -task c; fm_target.h): the targets are -1 / +1, each train
// case keeps a latent Gaussian target on its label's side of 0, and step 5 becomes: predict,
// p = cdf_gaussian(prediction), count the correct votes, form the case's new latent target (ALS:
// its expected value; MCMC: a truncated-normal draw) and store e = prediction - latent target --
// one launch over the train cases -- and report accuracies in place of RMSEs.  Steps 1-4 do not
// look at targets: they are the same draws in the same order.
//
// FMChain owns the model, the hyperparameter state, the generator and every buffer the two
// layouts share; a learner derives from it and supplies what depends on how the cases are
// stored, through the hooks below.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/sbmf.h"
#include "common.h"
#include "fm_target.h"
#include "rng.h"

namespace sbmf {

struct FMQueryList;

struct FMChain {
    sbmf_config cfg{};
    uint32_t K = 0, Kp = 0, p = 0;  // p: libFM's num_attribute
    uint64_t N = 0, T = 0;          // train cases (all ranks), test cases
    int k0 = 1, k1 = 1, do_sample = 1, do_multilevel = 1;
    double lo = 1.0, hi = 5.0;  // the train target range (min/max_target)
    double alpha = 1.0, w0 = 0.0;
    // libFM's attribute groups (-meta, fm_learn_mcmc.h:931-1089): G groups, grp[a] the group of
    // attribute a (empty: one group, every attribute), cnt[g] its attributes over all p ids.
    // Hyperparameters per group: w_mu[g], w_lambda[g], v_mu[g * K + f], v_lambda[g * K + f].
    // greg_w / greg_v: the groups' -regular precisions ([G] each; empty: cfg.regw / cfg.regv).
    uint32_t G = 1;
    std::vector<uint32_t> grp, cnt;
    std::vector<double> w_mu, w_lambda, v_mu, v_lambda, greg_w, greg_v;
    uint32_t it = 0, n_launch = 0;
    uint32_t nranges = 0;   // the general learner's ranges (the two-attribute learner has none: 0)
    uint32_t I = 0, J = 0;  // users-first layout (user u -> attribute u, item i -> I + i); I = 0: cases, no such view
    // the general learner's relations (libFM's -relation), in the order given: where a relation's
    // attributes and groups sit in the joined spaces, its block rows and the ranges of its table
    struct RelInfo {
        uint32_t attr_offset, num_attr, block_rows, nranges, group_offset, G;
    };
    std::vector<RelInfo> rel_info;
    GlibcRand grand{1};
    hipStream_t st = nullptr;
    hipEvent_t ev[3] = {};
    DBuf d_w, d_v, d_vT, d_zw, d_zv, d_pthis, d_sum, d_part, d_tpart, d_res, d_scratch;
    // the hyperparameter draws' sums (k_fmm_hsums; with groups k_fmg_gsums): per v column f and
    // for w (index K), and within a column per group -- index c * G + g --, {mu, gm's initial
    // value} in, {gm, m} out
    DBuf d_hmg, d_hsum;
    std::vector<double> h_mg, h_hs;
    // with groups (G > 1): the members of every group ascending (d_gidx, group g's at
    // [gptr[g], gptr[g+1])), d_gfirst[g] the first member of a contiguous group (its members
    // are a plain range) or 0xffffffff, the attributes' groups in the narrowest integer that
    // holds G (d_grp, grp_bytes wide), and the passes' priors {lambda, mu} of (column c, group
    // g) at d_lm[c * G + g], uploaded after the hyperparameter draws
    DBuf d_gptr, d_gidx, d_gfirst, d_grp, d_lm;
    int grp_bytes = 0;
    std::vector<double> h_lm;

    virtual ~FMChain();

    // ---- what a learner supplies.  A hook counts its own launches in n_launch unless said otherwise.
    // {sum e^2, sum (e - w0)} over every rank's residuals into s, valid after the next wait on
    // the stream; d_res[0..1] is the hook's to use (the chain counts two launches)
    virtual void residual_sums(double* s) = 0;
    // e -= d over this rank's cases (the chain counts the launch)
    virtual void shift_residuals(double d) = 0;
    virtual void start_passes() {}  // before the w pass
    virtual void w_pass() = 0;      // draw_w (:670-719) of every attribute, normals d_zw[a]
    virtual void v_pass(uint32_t f) = 0;  // draw_v (:780-835) of factor f, normals d_zv[a * K + f]
    virtual void sync_users() {}    // after the last v pass
    // predict_data_and_write_to_eterms of the train set from d_vT / d_w: e = prediction - target,
    // the blocks' squared errors to d_part (the chain counts the launch) ...
    virtual void predict_train_cases() = 0;
    // ... their sum to `out` (device), and what the other ranks add to it (h, after the wait)
    virtual void train_sum(double* out) = 0;
    virtual void gather_train_sum(double* h) {}
    // the test set: d_pthis, d_sum and d_tpart as fmm_predict_test writes them (the chain counts the launch)
    virtual void predict_test(double it1) = 0;
    // classification: the train frame (the chain fills ta but fidx, which is the learner's;
    // one launch), the test frame (d_pthis, d_sum; cnt[2b], cnt[2b + 1], ll[b] per 256-case block)
    // and e[q] -= t[q] over the train cases by position
    virtual void class_train(FMTargetArgs ta) = 0;
    virtual void class_test(double it1, uint32_t* cnt, double* ll) = 0;
    virtual void sub_targets(const double* t) = 0;
    // the query list (fmq.h; the general learner with relations): this iteration's scores of the
    // registered queries into the list's sums, last in the evaluate step.  query null: no list --
    // nothing is launched or recorded.
    FMQueryList* query = nullptr;
    virtual void score_queries() {}

    // ---- what the chain does
    // the shared set-up, last in a learner's create (its data uploaded): the flags, the target
    // range of the train targets y[N], the buffers (nl: this rank's train cases), the initial
    // model in either RNG mode and the starting predictions
    void setup(const sbmf_config& c, hipStream_t stream, uint32_t num_attr, uint64_t n, uint64_t nl, uint64_t nt,
               const float* y);
    bool classify() const { return cfg.task == SBMF_TASK_CLASSIFICATION; }
    // classification: a learner that keeps its train cases in another order than the train file's
    // sets, before setup, file_of_pos[q] = the file index of the case at position q (empty: the
    // position) and y_pos[q] = its -1 / +1 target.  The Philox draws are keyed by the file index
    // and the reference stream is consumed in file order, so no draw depends on the layout.
    std::vector<uint32_t> file_of_pos, pos_of_file;  // pos_of_file: the inverse, built by setup
    std::vector<float> y_pos;
    DBuf d_fidx, d_tgt, d_cres;
    void predict_train();
    void run(uint32_t iters, sbmf_sweep_cb cb, void* user);
    void predict_out(double* out);                 // the -out predictions
    void hyper_out(double* h4k, double* alpha_out);  // [v_lambda | v_mu | w_lambda,w_mu,0.. | 0]; one group only
    // the column sums of the hyperparameter draws on the current model and mu through the grouped
    // kernel (any G): out[(c * G + g) * 2 + {0: gm, 1: m}]
    void group_sums(double* out);
    void model(double* w0_out, double* w, double* v);  // w[p], v[K][p]
    // the users-first layout read by user and item: v as [I][K] and [J][K], w as [I] and [J]
    // (rows at or past p read 0), w0; refused when the learner was given cases (I = 0)
    void factors(double* U, double* V);
    void biases(double* bu, double* bv, double* b0);

protected:
    // the priors of the w pass (c = K) or of every v pass (c = 0..K-1) to d_lm; a no-op without groups
    void upload_priors(bool vcols);

private:
    void evaluate_class(sbmf_sweep_info& info);
    void ensure_group_lists();
    void launch_hsums();
    template <class R>
    void init_model(R& g, std::vector<double>& h_w, std::vector<double>& h_v);
    template <class R>
    void draw_hyper_w(R& g);
    template <class R>
    void draw_hyper_v(R& g);
    template <class R>
    void fill_normals(R& g, DBuf& d, uint32_t cols, uint32_t tag);
    template <class R>
    void sweep_draws(R& g);
};

// ---- rows by length, for both learners' pass launches
// SBMF_FMM_LONG moves the long-row bound (default 4096, at least 256), SBMF_FMM_CHUNK the chunk
// size (default 4096: the 1024-thread workgroup's four cases per thread; 0 turns chunks off)
void fm_long_bounds(uint32_t& longb, uint32_t& chunk);
static const int fm_bin_tpr[3] = {64, 256, 1024};  // threads per row of bin 0, 1, 2
// rows [r0, r1) of ptr binned by length: <= 256 entries bin 0, <= longb bin 1, longer bin 2; the
// longest first within a bin: blocks start roughly in index order, so a long row dispatched
// late would set the launch's tail (rows are independent: the order changes no result)
void fm_bin_rows(const std::vector<uint32_t>& ptr, uint32_t r0, uint32_t r1, uint32_t longb, std::vector<uint32_t> b[3]);
// rows[0..nrows) cut into chunks of at most `chunk` entries {row, first entry, entries, i},
// a row's chunks consecutive, appended to chunks; cfirst gets nrows + 1 chunk offsets relative
// to the first chunk appended
void fm_cut_chunks(const std::vector<uint32_t>& ptr, const uint32_t* rows, uint32_t nrows, uint32_t chunk,
                   std::vector<uint4>& chunks, std::vector<uint32_t>& cfirst);

}  // namespace sbmf
