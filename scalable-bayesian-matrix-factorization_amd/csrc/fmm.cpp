// fmm.cpp -- host side of the libFM-order MCMC / ALS learner (fmm.h):
// the reference's `bin/libFM -method mcmc` / `-method als` chain
// (src/libfm/src/fm_learn_mcmc.h, fm_learn_mcmc_simultaneous.h, set up by
// libfm.cpp:124-136,386-513) on rating data in libFM's users-first layout.
//
// The chain itself -- the draws, the sweep, the read-outs -- is FMChain's (fmc.h); this file
// holds the data in user and item order, the passes over them and the rank logic.
//
// Several ranks (one process per GPU), as the online VB learner: rank k owns
// the users sbmf_partition_rows gives it and every case of those users.  User
// rows are drawn locally; an item pass writes each item row's local sums, one
// all-gather delivers every rank's, and every rank draws every item the same
// way (sums added in rank order) and forwards the change to its own cases.
// The scalar sums (alpha, w0, the train RMSE) are all-gathered per rank; the
// owned users' w and v are broadcast after each sweep's passes, so the host
// hyperparameter draws, the test predictions and the factors see every
// attribute.  The host draws every variate on every rank (the same stream).
#include "fmm.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "comm.h"
#include "common.h"
#include "fmc.h"
#include "kernels.h"

namespace sbmf {

struct FMBin {
    std::vector<uint32_t> rows;
    DBuf d_rows;
    int tpr;
    // one rank, the long-row bin: each row cut into chunks of at most fmm_chunk cases
    // {row, first case, cases, row index in this bin}; row i owns [cfirst[i], cfirst[i+1])
    std::vector<uint4> chunks;
    std::vector<uint32_t> cfirst;
    DBuf d_chunks, d_cfirst, d_csums, d_cdelta, d_cqq;
};

struct FMLearner : FMChain {
    uint32_t RI = 0;  // item-side rows (p - I)
    uint64_t NL = 0;  // this rank's train cases
    FMBin ubins[3], ibins[3];
    // device
    DBuf d_uptr, d_upart, d_uperm, d_uown, d_uy, d_iptr, d_ipart, d_iperm;
    DBuf d_eu, d_ei, d_vold, d_su, d_si, d_sy;
    // several ranks
    Comm* comm = nullptr;
    int R = 1;
    // one rank: residuals in both orders updated in place (FMPassArgs::e_io), the
    // attributes' last draws in d_rec; the pass each side must apply on read
    DBuf d_rec;
    int pend_u = 0, pend_i = 0;
    std::vector<uint64_t> ubounds;
    DBuf d_sums, d_recvg, d_delta, d_recv;

    // R ranks: every rank's `n` doubles at d (device) -> host, summed in rank order
    void gather_sums(const double* d, int n, double* out) {
        comm->allgather(d, n * sizeof(double), d_recv.p, st);
        std::vector<double> h((size_t)R * n);
        HIPCHK(hipMemcpyAsync(h.data(), d_recv.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int k = 0; k < n; ++k) {
            double t = 0.0;
            for (int r = 0; r < R; ++r) t += h[(size_t)r * n + k];
            out[k] = t;
        }
    }
    // R ranks: the owned users' fresh w and v to every rank
    void sync_users() override {
        if (R <= 1) return;
        comm->group_begin();
        comm->bcast_ranges(d_w.p, sizeof(double), ubounds, st);
        for (uint32_t f = 0; f < K; ++f) comm->bcast_ranges(d_v.as<double>() + (size_t)f * p, sizeof(double), ubounds, st);
        comm->group_end();
    }

    FMPassArgs pass_args(bool items) {
        FMPassArgs a{};
        a.ptr = (items ? d_iptr : d_uptr).as<uint32_t>();
        a.part = (items ? d_ipart : d_upart).as<uint32_t>();
        a.perm = (items ? d_iperm : d_uperm).as<uint32_t>();
        a.e_in = (items ? d_ei : d_eu).as<double>();
        a.e_out = (items ? d_eu : d_ei).as<double>();
        a.a0 = items ? I : 0;
        a.pa0 = items ? 0 : I;
        a.alpha = alpha;
        a.do_sample = do_sample;
        a.item_side = items ? 1 : 0;
        if (R == 1) {
            a.e_io = (items ? d_ei : d_eu).as<double>();
            a.rec = d_rec.as<double2>();
            a.pend = items ? pend_i : pend_u;
        }
        return a;
    }
    // one rank: the item-order copy of the residuals from the user-order one (after the
    // train re-prediction and the w0 shift); nothing is pending on either side
    void start_passes() override {
        if (R != 1) return;
        if (NL) HIPCHK(launch_unpack<double>(d_eu.as<double>(), d_uperm.as<uint32_t>(), NL, d_ei.as<double>(), st));
        ++n_launch;
        pend_u = pend_i = 0;
    }
    void run_bins(FMPassArgs a, bool items, bool vpass) {
        auto launch = [&](int xmode) {
            a.xmode = xmode;
            for (FMBin& b : items ? ibins : ubins) {
                if (b.rows.empty()) continue;
                a.rows = b.d_rows.as<uint32_t>();
                a.nrows = (uint32_t)b.rows.size();
                if (xmode == 0 && !b.chunks.empty()) {
                    // one rank, long rows in chunks: the chunks' sums, the draw per row (chunk
                    // sums in chunk order), then every chunk's residual update -- the row's
                    // cases spread over many workgroups instead of one
                    FMPassArgs c = a;
                    c.chunks = b.d_chunks.as<uint4>();
                    c.nrows = (uint32_t)b.chunks.size();
                    c.xmode = 1;
                    c.sums = b.d_csums.as<double2>();
                    HIPCHK(vpass ? fmm_vpass(c, b.tpr, st) : fmm_wpass(c, b.tpr, st));
                    HIPCHK(fmm_chunk_draw(a, b.d_rows.as<uint32_t>(), b.d_cfirst.as<uint32_t>(), a.nrows,
                                          b.d_csums.as<double2>(), vpass ? 1 : 0, b.d_cdelta.as<double4>(),
                                          b.d_cqq.as<double2>(), st));
                    c.xmode = 2;
                    c.delta = b.d_cdelta.as<double4>();
                    c.qq = b.d_cqq.as<double2>();
                    HIPCHK(vpass ? fmm_vpass(c, b.tpr, st) : fmm_wpass(c, b.tpr, st));
                    n_launch += 3;
                    continue;
                }
                HIPCHK(vpass ? fmm_vpass(a, b.tpr, st) : fmm_wpass(a, b.tpr, st));
                ++n_launch;
            }
        };
        if (!(items && R > 1)) {
            launch(0);
            // one rank: the other side applies this pass on read
            if (items)
                pend_u = vpass ? 2 : 1;
            else
                pend_i = vpass ? 2 : 1;
            return;
        }
        // several ranks: local sums of every item row -> all-gather -> the same draw everywhere
        a.sums = d_sums.as<double2>();
        launch(1);
        comm->allgather(d_sums.p, (size_t)RI * sizeof(double2), d_recvg.p, st);
        HIPCHK(fmm_item_update(a, d_recvg.as<double2>(), R, RI, vpass ? 1 : 0, d_delta.as<double4>(), st));
        a.delta = d_delta.as<double4>();
        launch(2);
        ++n_launch;
    }
    FMPredictArgs predict_args() {
        FMPredictArgs a{};
        a.vT = d_vT.as<double>();
        a.w = d_w.as<double>();
        a.w0 = w0;
        a.K = K;
        a.Kp = Kp;
        a.I = I;
        a.k0 = k0;
        a.k1 = k1;
        a.lo = lo;
        a.hi = hi;
        return a;
    }
    void predict_train_cases() override {
        HIPCHK(fmm_predict_train(predict_args(), d_uown.as<uint32_t>(), d_upart.as<uint32_t>(), d_uy.as<float>(), NL,
                                 d_eu.as<double>(), d_part.as<double>(), st));
    }
    void train_sum(double* out) override {
        if (NL)
            HIPCHK(launch_sum(d_part.as<double>(), (NL + 255) / 256, out, d_scratch.as<double>(), st));
        else
            HIPCHK(hipMemsetAsync(out, 0, sizeof(double), st));
    }
    void gather_train_sum(double* h) override {
        if (R > 1) gather_sums(d_res.as<double>() + 2, 1, h);
    }
    void predict_test(double it1) override {
        HIPCHK(fmm_predict_test(predict_args(), d_su.as<uint32_t>(), d_si.as<uint32_t>(), d_sy.as<float>(), T, it1,
                                d_pthis.as<double>(), d_sum.as<double>(), d_tpart.as<double>(), st));
    }
    void class_train(FMTargetArgs ta) override {
        ta.fidx = d_fidx.as<uint32_t>();
        HIPCHK(fmm_class_train(predict_args(), ta, d_uown.as<uint32_t>(), d_upart.as<uint32_t>(), d_uy.as<float>(), NL,
                               d_eu.as<double>(), st));
    }
    void class_test(double it1, uint32_t* cnt, double* ll) override {
        HIPCHK(fmm_class_test(predict_args(), d_su.as<uint32_t>(), d_si.as<uint32_t>(), d_sy.as<float>(), T, it1,
                              d_pthis.as<double>(), d_sum.as<double>(), cnt, ll, st));
    }
    void sub_targets(const double* t) override { HIPCHK(fmm_sub_targets(d_eu.as<double>(), NL, t, st)); }
    void residual_sums(double* s) override {
        double* res = d_res.as<double>();
        if (NL) {
            HIPCHK(fmm_esums(d_eu.as<double>(), NL, w0, d_part.as<double>(), st));
            HIPCHK(launch_sum_cols(d_part.as<double>(), (uint32_t)((NL + 1023) / 1024), 2, res, st));
        } else {
            HIPCHK(hipMemsetAsync(res, 0, 2 * sizeof(double), st));
        }
        if (R > 1)
            gather_sums(res, 2, s);  // every rank's sums, rank order
        else
            HIPCHK(hipMemcpyAsync(s, res, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    void shift_residuals(double d) override { HIPCHK(fmm_shift(d_eu.as<double>(), NL, d, st)); }
    // users, then items
    void w_pass() override {
        for (int side = 0; side < 2; ++side) {
            FMPassArgs a = pass_args(side == 1);
            a.own = d_w.as<double>();
            a.z = d_zw.as<double>();
            a.zs = 1;
            a.zoff = 0;
            a.mu = w_mu[0];
            a.lambda = w_lambda[0];
            run_bins(a, side == 1, false);
        }
    }
    void v_pass(uint32_t f) override {
        double* col = d_v.as<double>() + (size_t)f * p;
        if (R > 1)  // one rank: the item pass reads the users' old values from d_rec
            HIPCHK(hipMemcpyAsync(d_vold.p, col, (size_t)I * sizeof(double), hipMemcpyDeviceToDevice, st));
        for (int side = 0; side < 2; ++side) {
            FMPassArgs a = pass_args(side == 1);
            a.own = col;
            a.partner_col = col;
            a.vold_u = d_vold.as<double>();
            a.z = d_zv.as<double>();
            a.zs = K;
            a.zoff = f;
            a.mu = v_mu[f];
            a.lambda = v_lambda[f];
            run_bins(a, side == 1, true);
        }
    }
};

FMChain* fmm_create(const sbmf_config& c, uint64_t n, const uint32_t* u, const uint32_t* i, const double* r,
                    uint64_t nt, const uint32_t* tu, const uint32_t* ti, const double* tr, uint32_t I, uint32_t J,
                    hipStream_t st, Comm* comm) {
    std::unique_ptr<FMLearner> L(new FMLearner());
    if (comm && comm->nranks() > 1) {
        L->comm = comm;
        L->R = comm->nranks();
    }
    L->I = I;
    L->J = J;
    const bool classify = c.task == SBMF_TASK_CLASSIFICATION;
    if (classify && L->R > 1)
        fail(SBMF_E_STATE, "classification (task = SBMF_TASK_CLASSIFICATION) runs on one rank: the latent targets and "
                           "the vote counts of the train frame are not exchanged between the user ranges of %d ranks",
             L->R);
    if (n >= 0xffffffffull) fail(SBMF_E_ARG, "more than 2^32-1 ratings are not supported");
    // libFM attribute layout: user u -> u, item i -> I + i; num_feature = largest id + 1 (Data.h:221),
    // num_all_attribute = max(train, test) + 1 (libfm.cpp:330)
    uint32_t imax_tr = 0, imax_te = 0;
    for (uint64_t x = 0; x < n; ++x) imax_tr = std::max(imax_tr, i[x]);
    for (uint64_t x = 0; x < nt; ++x) imax_te = std::max(imax_te, ti[x]);
    const uint32_t p = std::max(I + imax_tr + 1, nt ? I + imax_te + 1 : 0) + 1;
    L->RI = p - I;
    // DATA_FLOAT targets (fm_data.h:25)
    std::vector<float> y(r, r + n), ys(tr, tr + nt);
    if (classify)  // the learner's own copy: <= 0 to -1, the others to +1 (libfm.cpp:454-455)
        for (std::vector<float>* v : {&y, &ys})
            for (float& t : *v) t = t <= 0.0f ? -1.0f : 1.0f;
    // several ranks: the user ranges (sbmf_partition_rows over the users' rating counts);
    // a rank keeps the cases of its users only
    L->ubounds.assign(L->R + 1, 0);
    L->ubounds[L->R] = I;
    uint32_t u0 = 0, u1 = I;
    std::vector<uint8_t> mine(n, 1);
    L->NL = n;
    if (L->R > 1) {
        std::vector<uint32_t> cnt(I + 1, 0);
        for (uint64_t x = 0; x < n; ++x) cnt[u[x] + 1]++;
        for (uint32_t k = 0; k < I; ++k) cnt[k + 1] += cnt[k];
        if (sbmf_partition_rows(cnt.data(), I, L->R, L->ubounds.data()) != SBMF_OK)
            fail(SBMF_E_ARG, "libFM learner: user partition failed");
        u0 = (uint32_t)L->ubounds[comm->rank()];
        u1 = (uint32_t)L->ubounds[comm->rank() + 1];
        L->NL = 0;
        for (uint64_t x = 0; x < n; ++x) {
            mine[x] = u[x] >= u0 && u[x] < u1;
            L->NL += mine[x];
        }
    }
    const uint64_t nl = L->NL;
    // user order (CSR over users, cases in file order) and item order (CSC over item rows [0, RI)),
    // over this rank's cases
    std::vector<uint32_t> uptr(I + 1, 0), iptr(L->RI + 1, 0);
    for (uint64_t x = 0; x < n; ++x) {
        if (!mine[x]) continue;
        uptr[u[x] + 1]++;
        iptr[i[x] + 1]++;
    }
    for (uint32_t k = 0; k < I; ++k) uptr[k + 1] += uptr[k];
    for (uint32_t k = 0; k < L->RI; ++k) iptr[k + 1] += iptr[k];
    std::vector<uint32_t> upos(n), ipos(n), uown(nl), upart(nl), ipart(nl), uperm(nl), iperm(nl);
    std::vector<float> uy(nl);
    {
        std::vector<uint32_t> fu(uptr.begin(), uptr.end() - 1), fi(iptr.begin(), iptr.end() - 1);
        for (uint64_t x = 0; x < n; ++x) {
            if (!mine[x]) continue;
            upos[x] = fu[u[x]]++;
            ipos[x] = fi[i[x]]++;
        }
    }
    for (uint64_t x = 0; x < n; ++x) {
        if (!mine[x]) continue;
        uown[upos[x]] = u[x];
        upart[upos[x]] = i[x];
        uy[upos[x]] = y[x];
        uperm[upos[x]] = ipos[x];
        ipart[ipos[x]] = u[x];
        iperm[ipos[x]] = upos[x];
    }
    // rows binned by length (users: this rank's range; items: every item row, each rank over
    // its own cases); one rank: the long-row bin's rows in chunks
    uint32_t longb, chunk;
    fm_long_bounds(longb, chunk);
    for (FMBin* bs : {L->ubins, L->ibins}) {
        const bool users = bs == L->ubins;
        const std::vector<uint32_t>& pt = users ? uptr : iptr;
        std::vector<uint32_t> rows[3];
        fm_bin_rows(pt, users ? u0 : 0, users ? u1 : L->RI, longb, rows);
        for (int k = 0; k < 3; ++k) {
            bs[k].tpr = fm_bin_tpr[k];
            bs[k].rows.swap(rows[k]);
            upload(bs[k].d_rows, bs[k].rows, st);
        }
        FMBin& b = bs[2];
        if (L->R != 1 || !chunk || b.rows.empty()) continue;
        fm_cut_chunks(pt, b.rows.data(), (uint32_t)b.rows.size(), chunk, b.chunks, b.cfirst);
        upload(b.d_chunks, b.chunks, st);
        upload(b.d_cfirst, b.cfirst, st);
        b.d_csums.alloc(b.chunks.size() * sizeof(double2));
        b.d_cdelta.alloc(b.rows.size() * sizeof(double4));
        b.d_cqq.alloc(b.rows.size() * sizeof(double2));
    }
    upload(L->d_uptr, uptr, st);
    upload(L->d_iptr, iptr, st);
    upload(L->d_upart, upart, st);
    upload(L->d_ipart, ipart, st);
    upload(L->d_uperm, uperm, st);
    upload(L->d_iperm, iperm, st);
    upload(L->d_uown, uown, st);
    upload(L->d_uy, uy, st);
    std::vector<uint32_t> su(tu, tu + nt), si(ti, ti + nt);
    upload(L->d_su, su, st);
    upload(L->d_si, si, st);
    upload(L->d_sy, ys, st);
    L->d_eu.alloc(std::max<uint64_t>(nl, 1) * sizeof(double));
    L->d_ei.alloc(std::max<uint64_t>(nl, 1) * sizeof(double));
    if (L->R > 1) {
        L->d_sums.alloc((size_t)std::max(L->RI, 1u) * sizeof(double2));
        L->d_recvg.alloc((size_t)L->R * std::max(L->RI, 1u) * sizeof(double2));
        L->d_delta.alloc((size_t)std::max(L->RI, 1u) * sizeof(double4));
        L->d_recv.alloc((size_t)L->R * 4 * sizeof(double));
    }
    L->d_vold.alloc((size_t)std::max(I, 1u) * sizeof(double));
    L->d_rec.alloc((size_t)p * sizeof(double2));
    if (classify) {  // the residuals are in user order: the file index and the target of each position
        L->file_of_pos.resize(n);
        for (uint64_t x = 0; x < n; ++x) L->file_of_pos[upos[x]] = (uint32_t)x;
        L->y_pos = uy;
    }
    L->setup(c, st, p, n, nl, nt, y.data());
    return L.release();
}

}  // namespace sbmf
