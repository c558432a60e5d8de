// fmg.cpp -- host side of the general libFM MCMC / ALS learner (fmg.h): the reference's
// fm_learn_mcmc chain (fm_learn_mcmc.h:411-623, fm_learn_mcmc_simultaneous.h:96-245) on
// cases with any number of features.
//
// The chain itself -- the draws, the sweep, the read-outs -- is FMChain's (fmc.h); this file holds
// the cache, the two copies of the cases and the passes: every w, and per factor f the cache's q
// (k_fmg_q) then every v[f][.], range by range and within a range bin by bin.
#include "fmg.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "common.h"
#include "fmc.h"
#include "kernels.h"

namespace sbmf {

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

struct FGLearner : FMChain {
    std::vector<FGLaunch> launches;
    DBuf d_rows, d_chunks, d_cfirst, d_csums, d_cdelta;
    DBuf d_cptr, d_cattr, d_cx, d_y, d_aptr, d_ent, d_eq;
    DBuf d_tptr, d_tattr, d_tx, d_ty;

    // every launch of one pass, ranges ascending
    void run_pass(FGPassArgs a, bool vpass) {
        a.aptr = d_aptr.as<uint32_t>();
        a.ent = d_ent.as<uint2>();
        a.eq = d_eq.as<double2>();
        a.alpha = alpha;
        a.do_sample = do_sample;
        if (d_lm.p) {  // attribute groups: the row's own prior, column c's at d_lm[c * G ..]
            a.grp = d_grp.p;
            a.grp_bytes = grp_bytes;
            a.lm = d_lm.as<double2>() + (size_t)(vpass ? a.zoff : K) * G;
        }
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
    void predict_train_cases() override {
        HIPCHK(fmg_predict_train(predict_args(true), d_eq.as<double2>(), d_part.as<double>(), st));
    }
    void train_sum(double* out) override {
        HIPCHK(launch_sum(d_part.as<double>(), (N + 255) / 256, out, d_scratch.as<double>(), st));
    }
    void predict_test(double it1) override {
        HIPCHK(fmg_predict_test(predict_args(false), it1, d_pthis.as<double>(), d_sum.as<double>(), d_tpart.as<double>(),
                                st));
    }
    void class_train(FMTargetArgs ta) override {
        ta.fidx = d_fidx.as<uint32_t>();
        HIPCHK(fmg_class_train(predict_args(true), ta, d_eq.as<double2>(), st));
    }
    void class_test(double it1, uint32_t* cnt, double* ll) override {
        HIPCHK(fmg_class_test(predict_args(false), it1, d_pthis.as<double>(), d_sum.as<double>(), cnt, ll, st));
    }
    void sub_targets(const double* t) override { HIPCHK(fmg_sub_targets(d_eq.as<double2>(), N, t, st)); }
    void residual_sums(double* s) override {
        double* res = d_res.as<double>();
        HIPCHK(fmg_esums(d_eq.as<double2>(), N, w0, d_part.as<double>(), st));
        HIPCHK(launch_sum_cols(d_part.as<double>(), (uint32_t)((N + 1023) / 1024), 2, res, st));
        HIPCHK(hipMemcpyAsync(s, res, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    void shift_residuals(double d) override { HIPCHK(fmg_shift(d_eq.as<double2>(), N, d, st)); }
    void w_pass() override {
        FGPassArgs a{};
        a.own = d_w.as<double>();
        a.z = d_zw.as<double>();
        a.zs = 1;
        a.zoff = 0;
        a.mu = w_mu[0];
        a.lambda = w_lambda[0];
        run_pass(a, false);
    }
    void v_pass(uint32_t f) override {
        double* col = d_v.as<double>() + (size_t)f * p;
        HIPCHK(fmg_q(d_cptr.as<uint32_t>(), d_cattr.as<uint32_t>(), d_cx.as<float>(), N, col, d_eq.as<double2>(), st));
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
};

// The cases in the order of their first (smallest) attribute, file order within it (cases without
// features last): the records {e, q} follow the cases, so the passes of that attribute's field
// -- the users of a users-first file -- read and write them front to back instead of one memory
// line per case.  The order of the cases is a labelling: no draw depends on it.
struct OrderedCases {
    std::vector<uint64_t> ptr;
    std::vector<uint32_t> attr, order;  // order[k]: the file index of the case at position k
    std::vector<float> x, y;
    bool build(const sbmf_cases& in, sbmf_cases& out) {
        auto key = [&](uint64_t c) { return in.ptr[c + 1] > in.ptr[c] ? in.attr[in.ptr[c]] : in.num_attr; };
        bool sorted = true;
        for (uint64_t c = 1; c < in.n && sorted; ++c) sorted = key(c - 1) <= key(c);
        if (sorted) return false;
        std::vector<uint64_t> pos((size_t)in.num_attr + 2, 0);
        for (uint64_t c = 0; c < in.n; ++c) pos[key(c) + 1]++;
        for (size_t k = 0; k + 1 < pos.size(); ++k) pos[k + 1] += pos[k];
        order.resize(in.n);
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

FMChain* fmg_create(const sbmf_config& c, const sbmf_cases& tr_file, const sbmf_cases& te_in, hipStream_t st,
                    const FMGroups* groups) {
    if (tr_file.n == 0) fail(SBMF_E_STATE, "no training cases");
    if (tr_file.n >= 0xffffffffull || te_in.n >= 0xffffffffull || tr_file.nnz >= 0xffffffffull || te_in.nnz >= 0xffffffffull)
        fail(SBMF_E_ARG, "more than 2^32-1 cases or features are not supported");
    OrderedCases oc;
    sbmf_cases tr_ordered{};
    const sbmf_cases& tr_in = oc.build(tr_file, tr_ordered) ? tr_ordered : tr_file;
    // classification: the learner's own copy of the targets, <= 0 to -1 and the others to +1 (libfm.cpp:454-455)
    sbmf_cases tr = tr_in, te = te_in;
    std::vector<float> ytr, yte;
    if (c.task == SBMF_TASK_CLASSIFICATION) {
        auto map = [](const sbmf_cases& cs, std::vector<float>& y) {
            y.resize(cs.n);
            for (uint64_t x = 0; x < cs.n; ++x) y[x] = cs.target[x] <= 0.0f ? -1.0f : 1.0f;
            return y.data();
        };
        tr.target = map(tr_in, ytr);
        te.target = map(te_in, yte);
    }
    std::unique_ptr<FGLearner> L(new FGLearner());
    if (c.task == SBMF_TASK_CLASSIFICATION) L->file_of_pos = oc.order;
    // num_all_attribute = max(train, test num_feature) + 1 (libfm.cpp:328)
    if (std::max(tr.num_attr, te.num_attr) >= 0xfffffffeu) fail(SBMF_E_ARG, "attribute id too large");
    const uint32_t p = std::max(tr.num_attr, te.num_attr) + 1;
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
    uint32_t longb, chunk;
    fm_long_bounds(longb, chunk);
    std::vector<uint32_t> rows, cfirst;
    std::vector<uint4> chunks;
    uint32_t nlong = 0;
    rows.reserve(p);
    for (uint32_t r = 0; r + 1 < bounds.size(); ++r) {
        std::vector<uint32_t> b[3];
        fm_bin_rows(aptr, bounds[r], bounds[r + 1], longb, b);
        for (int j = 2; j >= 0; --j) {  // the long rows first: they set the range's tail
            if (b[j].empty()) continue;
            FGLaunch l;
            l.r0 = (uint32_t)rows.size();
            l.nrows = (uint32_t)b[j].size();
            l.tpr = fm_bin_tpr[j];
            rows.insert(rows.end(), b[j].begin(), b[j].end());
            if (j == 2 && chunk) {
                l.c0 = (uint32_t)chunks.size();
                l.l0 = nlong;
                // cfirst: per launch nrows + 1 offsets relative to the launch's first chunk
                l.f0 = (uint32_t)cfirst.size();
                fm_cut_chunks(aptr, b[j].data(), l.nrows, chunk, chunks, cfirst);
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
    L->d_eq.alloc(tr.n * sizeof(double2));
    if (groups && !groups->group.empty()) {
        // group[a] for every attribute of num_attribute; one group is the ungrouped chain
        if (groups->group.size() != p)
            fail(SBMF_E_ARG, "sbmf_set_attr_groups gave %zu group ids; this context has num_attribute = %u "
                             "(max(train, test num_attr) + 1)", groups->group.size(), p);
        L->G = *std::max_element(groups->group.begin(), groups->group.end()) + 1;
        if (L->G > 65535u) fail(SBMF_E_ARG, "%u attribute groups: at most 65535 are supported", L->G);
        if (L->G > 1) L->grp = groups->group;
    }
    if (groups && !groups->regw.empty()) {
        if (groups->regw.size() != L->G)
            fail(SBMF_E_ARG, "sbmf_set_group_regular gave %zu groups; the context has %u", groups->regw.size(), L->G);
        L->greg_w = groups->regw;
        L->greg_v = groups->regv;
    }
    L->setup(c, st, p, tr.n, tr.n, te.n, tr.target);
    L->n_launch = 0;
    return L.release();
}

}  // namespace sbmf
