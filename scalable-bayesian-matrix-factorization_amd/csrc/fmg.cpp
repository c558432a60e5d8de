// fmg.cpp -- host side of the general libFM MCMC / ALS learner (fmg.h): the reference's
// fm_learn_mcmc chain (fm_learn_mcmc.h:411-623, fm_learn_mcmc_simultaneous.h:96-245) on
// cases with any number of features.
//
// The chain itself -- the draws, the sweep, the read-outs -- is FMChain's (fmc.h); this file holds
// the cache, the two copies of the cases and the passes: every w, and per factor f the cache's q
// (k_fmg_q) then every v[f][.], range by range and within a range bin by bin.  A relation
// (libFM's -relation, FGRel) adds its own step after the main table's in both: gather, the passes
// over its attributes, sync.
#include "fmg.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "common.h"
#include "fmc.h"
#include "fmq.h"
#include "kernels.h"
#include "recommend.h"

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

// The ranges a learner launches by: sbmf_fm_ranges', or with SBMF_FMG_SERIAL=1 one attribute per
// range -- literally libFM's loop
static void fm_launch_bounds(const sbmf_cases& tr, uint32_t p, std::vector<uint32_t>& bounds) {
    const char* ser = std::getenv("SBMF_FMG_SERIAL");
    if (ser && std::atoi(ser) != 0) {
        bounds.resize((size_t)p + 1);
        for (uint32_t a = 0; a <= p; ++a) bounds[a] = a;
    } else {
        fm_ranges(tr, p, bounds);
    }
}

// One launch of a pass: rows [r0, r0 + nrows) of d_rows with tpr threads each, or the long rows
// of a range in chunks
struct FGLaunch {
    uint32_t r0 = 0, nrows = 0;
    int tpr = 64;
    // chunked: chunks [c0, c0 + nchunks), long-row slots from l0, the rows' chunk offsets from f0
    uint32_t c0 = 0, nchunks = 0, l0 = 0, f0 = 0;
};

// The launches of a pass over the rows of an attribute-major table: per range, rows binned by
// length (<= 256 entries 64 threads, <= longb 256, longer 1024 or in chunks), longest first
// within a bin.  The bin of a row depends on its length alone, so its sums have the same order
// under any partition into ranges.
struct FGPlan {
    std::vector<FGLaunch> launches;
    DBuf d_rows, d_chunks, d_cfirst, d_csums, d_cdelta;
    void build(const std::vector<uint32_t>& aptr, const std::vector<uint32_t>& bounds, hipStream_t st) {
        uint32_t longb, chunk;
        fm_long_bounds(longb, chunk);
        std::vector<uint32_t> rows, cfirst;
        std::vector<uint4> chunks;
        uint32_t nlong = 0;
        rows.reserve(aptr.size());
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
                launches.push_back(l);
            }
        }
        upload(d_rows, rows, st);
        upload(d_chunks, chunks, st);
        upload(d_cfirst, cfirst, st);
        d_csums.alloc(std::max<size_t>(chunks.size(), 1) * sizeof(double2));
        d_cdelta.alloc(std::max<size_t>(nlong, 1) * sizeof(double4));
        HIPCHK(hipStreamSynchronize(st));  // the vectors are locals
    }
};

// One relation on the device (fmg.h): the block table twice, like the cases -- a CSR by block row
// (q^B, the block predictions) and a CSC of {block row, x} entries by attribute (the passes) --,
// the block rows' records, the maps of the train / test cases, and per block row its train cases
// in ascending position with the gather's launches by case count.
struct FGRel {
    uint32_t off = 0, nattr = 0, nb = 0;
    FGPlan plan;
    DBuf d_aptr, d_ent, d_rptr, d_rattr, d_rx, d_rb, d_qbf, d_qs, d_map, d_tmap, d_bptr, d_bcase, d_grows;
    // a gather launch: block rows [r0, r0 + nrows) of d_grows, or (nchunks > 0) the long block rows
    // in chunks [c0, c0 + nchunks) with their chunk offsets from f0, then the combine
    struct Gather {
        uint32_t r0, nrows;
        int tpr;
        uint32_t c0, nchunks, f0;
    };
    std::vector<Gather> gather;
    DBuf d_gchunks, d_gcfirst, d_gsums;
};

struct FGLearner : FMChain {
    FGPlan plan;
    DBuf d_cptr, d_cattr, d_cx, d_y, d_aptr, d_ent, d_eq;
    DBuf d_tptr, d_tattr, d_tx, d_ty;
    std::vector<std::unique_ptr<FGRel>> rels;
    bool blocks_stale = true;  // the block rows' y / q^B terms are older than the model

    // every launch of one pass, ranges ascending: over the cases, or over relation `rel`'s block rows
    void run_pass(FGPassArgs a, bool vpass, FGRel* rel = nullptr) {
        const FGPlan& pl = rel ? rel->plan : plan;
        const uint32_t off = rel ? rel->off : 0;
        a.aptr = (rel ? rel->d_aptr : d_aptr).as<uint32_t>();
        a.ent = (rel ? rel->d_ent : d_ent).as<uint2>();
        a.eq = d_eq.as<double2>();
        a.rb = rel ? rel->d_rb.as<double4>() : nullptr;
        a.own += off;
        a.z += (size_t)off * a.zs;
        a.alpha = alpha;
        a.do_sample = do_sample;
        if (d_lm.p) {  // attribute groups: the row's own prior, column c's at d_lm[c * G ..]
            a.grp = static_cast<const char*>(d_grp.p) + (size_t)off * grp_bytes;
            a.grp_bytes = grp_bytes;
            a.lm = d_lm.as<double2>() + (size_t)(vpass ? a.zoff : K) * G;
        }
        auto pass = [&](const FGPassArgs& x, int tpr) {
            if (rel) return vpass ? fmg_rel_vpass(x, tpr, st) : fmg_rel_wpass(x, tpr, st);
            return vpass ? fmg_vpass(x, tpr, st) : fmg_wpass(x, tpr, st);
        };
        for (const FGLaunch& l : pl.launches) {
            a.rows = pl.d_rows.as<uint32_t>() + l.r0;
            a.nrows = l.nrows;
            a.xmode = 0;
            a.chunks = nullptr;
            if (l.nchunks) {
                // the chunks' sums, the draw per row (chunk sums in chunk order), every chunk's update
                FGPassArgs c = a;
                c.chunks = pl.d_chunks.as<uint4>() + l.c0;
                c.nrows = l.nchunks;
                c.xmode = 1;
                c.sums = pl.d_csums.as<double2>() + l.c0;
                HIPCHK(pass(c, l.tpr));
                // a relation's w draw takes old * s2 off m after the sums, as every v draw (fmg.hip)
                HIPCHK(fmg_chunk_draw(a, a.rows, pl.d_cfirst.as<uint32_t>() + l.f0, l.nrows,
                                      pl.d_csums.as<double2>() + l.c0, vpass || rel ? 1 : 0,
                                      pl.d_cdelta.as<double4>() + l.l0, st));
                c.xmode = 2;
                c.delta = pl.d_cdelta.as<double4>() + l.l0;
                HIPCHK(pass(c, l.tpr));
                n_launch += 3;
                continue;
            }
            HIPCHK(pass(a, l.tpr));
            ++n_launch;
        }
    }

    // a relation's step (:458-491, :579-620): gather with the un-sync, its attributes' draws, sync
    void rel_step(FGRel& r, const FGPassArgs& a, bool vpass) {
        FGRelArgs g{};
        g.bptr = r.d_bptr.as<uint32_t>();
        g.bcase = r.d_bcase.as<uint32_t>();
        g.rb = r.d_rb.as<double4>();
        g.eq = d_eq.as<double2>();
        for (const FGRel::Gather& l : r.gather) {
            g.rows = r.d_grows.as<uint32_t>() + l.r0;
            g.nrows = l.nrows;
            g.chunks = nullptr;
            if (l.nchunks) {  // every chunk's sums (and un-sync), then per block row its chunks in chunk order
                FGRelArgs c = g;
                c.chunks = r.d_gchunks.as<uint4>() + l.c0;
                c.nrows = l.nchunks;
                c.sums = r.d_gsums.as<double4>() + l.c0;
                HIPCHK(fmg_rel_gather(c, vpass ? 1 : 0, l.tpr, st));
                HIPCHK(fmg_rel_gather_combine(g.rows, r.d_gcfirst.as<uint32_t>() + l.f0, l.nrows, c.sums, vpass ? 1 : 0,
                                              g.rb, st));
                n_launch += 2;
                continue;
            }
            HIPCHK(fmg_rel_gather(g, vpass ? 1 : 0, l.tpr, st));
            ++n_launch;
        }
        run_pass(a, vpass, &r);
        HIPCHK(fmg_rel_sync(r.d_map.as<uint32_t>(), N, r.d_rb.as<double4>(), d_eq.as<double2>(), vpass ? 1 : 0, st));
        ++n_launch;
    }

    // the block rows' terms of the predictions, once per model
    void block_predict() {
        if (!blocks_stale) return;
        for (auto& r : rels) {
            HIPCHK(fmg_rel_block_predict(r->d_rptr.as<uint32_t>(), r->d_rattr.as<uint32_t>(), r->d_rx.as<float>(), r->nb,
                                         d_vT.as<double>() + (size_t)r->off * Kp, d_w.as<double>() + r->off, K, Kp, k1,
                                         r->d_qbf.as<double>(), r->d_qs.as<double>(), r->d_rb.as<double4>(), st));
            ++n_launch;
        }
        blocks_stale = false;
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
        a.nrel = (uint32_t)rels.size();
        for (uint32_t r = 0; r < a.nrel; ++r) {
            a.rel[r].map = (train ? rels[r]->d_map : rels[r]->d_tmap).as<uint32_t>();
            a.rel[r].qbf = rels[r]->d_qbf.as<double>();
            a.rel[r].qs = rels[r]->d_qs.as<double>();
        }
        return a;
    }
    void predict_train_cases() override {
        block_predict();
        HIPCHK(fmg_predict_train(predict_args(true), d_eq.as<double2>(), d_part.as<double>(), st));
    }
    void train_sum(double* out) override {
        HIPCHK(launch_sum(d_part.as<double>(), (N + 255) / 256, out, d_scratch.as<double>(), st));
    }
    void predict_test(double it1) override {
        block_predict();
        HIPCHK(fmg_predict_test(predict_args(false), it1, d_pthis.as<double>(), d_sum.as<double>(), d_tpart.as<double>(),
                                st));
    }
    void class_train(FMTargetArgs ta) override {
        ta.fidx = d_fidx.as<uint32_t>();
        block_predict();
        HIPCHK(fmg_class_train(predict_args(true), ta, d_eq.as<double2>(), st));
    }
    void class_test(double it1, uint32_t* cnt, double* ll) override {
        block_predict();
        HIPCHK(fmg_class_test(predict_args(false), it1, d_pthis.as<double>(), d_sum.as<double>(), cnt, ll, st));
    }
    void sub_targets(const double* t) override { HIPCHK(fmg_sub_targets(d_eq.as<double2>(), N, t, st)); }
    // The query list's three launches (fmq.h), after the frames: the block rows' terms are this
    // model's.  MCMC adds the iteration to the sums; ALS, whose result is the latest model (as its
    // predictions are), writes them and keeps the count at 1.
    void score_queries() override {
        FMQueryList& ql = *query;
        block_predict();
        FMQTermsArgs t{};
        t.nq = ql.nq;
        t.ptr = ql.d_ptr.as<uint32_t>();
        t.attr = ql.d_attr.as<uint32_t>();
        t.x = ql.d_x.as<float>();
        t.vT = d_vT.as<double>();
        t.w = d_w.as<double>();
        t.K = K;
        t.Kp = Kp;
        t.k1 = k1;
        for (uint32_t r = 0; r < rels.size(); ++r) {
            if (r == ql.rel) continue;
            t.rel[t.nrel++] = {ql.d_rows.as<uint32_t>() + (size_t)r * ql.nq, rels[r]->d_qbf.as<double>(),
                               rels[r]->d_qs.as<double>()};
        }
        t.s = ql.d_s.as<double>();
        t.a = ql.d_a.as<double>();
        const FGRel& R = *rels[ql.rel];
        HIPCHK(hipEventRecord(ql.ev[0], st));
        HIPCHK(fmq_terms(t, st));
        HIPCHK(fmq_operands(R.d_qbf.as<double>(), R.d_rb.as<double4>(), R.nb, K, Kp, ql.d_B.as<double>(),
                            ql.d_y.as<double>(), st));
        HIPCHK(hipEventRecord(ql.ev[1], st));
        const int epi = (classify() ? WATCH_EPI_CDF : 0) | (do_sample ? 0 : WATCH_EPI_SET);
        HIPCHK(launch_watch_accum_epi(epi, ql.ids, ql.nq, t.s, ql.d_B.as<double>(), R.nb, Kp, t.a, ql.d_y.as<double>(),
                                      k0 ? w0 : 0.0, classify() ? 0 : ql.clamp, lo, hi, ql.S1, ql.S2, st));
        HIPCHK(hipEventRecord(ql.ev[2], st));
        *ql.count = do_sample ? *ql.count + 1 : 1;
        n_launch += 3;
    }
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
        for (auto& r : rels) rel_step(*r, a, false);
        blocks_stale = true;
    }
    void v_pass(uint32_t f) override {
        double* col = d_v.as<double>() + (size_t)f * p;
        HIPCHK(fmg_q(d_cptr.as<uint32_t>(), d_cattr.as<uint32_t>(), d_cx.as<float>(), N, col, d_eq.as<double2>(), st));
        ++n_launch;
        for (auto& r : rels) {  // q^B per block row, added to its cases' q in relation order (:521-552)
            HIPCHK(fmg_rel_q(r->d_rptr.as<uint32_t>(), r->d_rattr.as<uint32_t>(), r->d_rx.as<float>(), r->nb, col + r->off,
                             r->d_rb.as<double4>(), st));
            HIPCHK(fmg_rel_addq(r->d_map.as<uint32_t>(), N, r->d_rb.as<double4>(), d_eq.as<double2>(), st));
            n_launch += 2;
        }
        FGPassArgs a{};
        a.own = col;
        a.z = d_zv.as<double>();
        a.zs = K;
        a.zoff = f;
        a.mu = v_mu[f];
        a.lambda = v_lambda[f];
        run_pass(a, true);
        for (auto& r : rels) rel_step(*r, a, true);
        blocks_stale = true;
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
    // by_row (a context with relations): by the block row of relation 0 instead, nkeys rows --
    // that relation's gather and sync then walk the records front to back
    bool build(const sbmf_cases& in, sbmf_cases& out, const uint32_t* by_row = nullptr, uint32_t nkeys = 0) {
        auto key = [&](uint64_t c) -> uint32_t {
            if (by_row) return by_row[c];
            return in.ptr[c + 1] > in.ptr[c] ? in.attr[in.ptr[c]] : in.num_attr;
        };
        bool sorted = true;
        for (uint64_t c = 1; c < in.n && sorted; ++c) sorted = key(c - 1) <= key(c);
        if (sorted) return false;
        std::vector<uint64_t> pos((size_t)(by_row ? nkeys : in.num_attr) + 2, 0);
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

// Relation r of a learner under construction: checked against the cases, laid out, uploaded
static std::unique_ptr<FGRel> build_relation(const FMRelation& in, uint32_t r, uint32_t off, uint64_t N, uint64_t T,
                                             const std::vector<uint32_t>& order, hipStream_t st, uint32_t& nranges) {
    std::unique_ptr<FGRel> R(new FGRel());
    const uint64_t nb64 = in.ptr.empty() ? 0 : in.ptr.size() - 1, nnz = in.attr.size();
    if (nb64 >= 0xffffffffull || nnz >= 0xffffffffull)
        fail(SBMF_E_ARG, "relation %u: more than 2^32-1 block rows or features are not supported", r);
    // (sbmf_add_relation checked the maps against the data it saw; the data may have been set again since)
    if (in.train_row.size() != N || in.test_row.size() != T)
        fail(SBMF_E_ARG, "relation %u: the maps hold %zu / %zu block-row indices, the train / test sets %llu / %llu cases",
             r, in.train_row.size(), in.test_row.size(), (unsigned long long)N, (unsigned long long)T);
    R->off = off;
    R->nattr = in.num_attr;
    R->nb = (uint32_t)nb64;
    const uint32_t nb = R->nb, pa = in.num_attr;
    // the train map by position (the cases' order on the device), each block row's cases ascending
    std::vector<uint32_t> map(N), bptr((size_t)nb + 1, 0), bcase(N);
    for (uint64_t q = 0; q < N; ++q) {
        map[q] = in.train_row[order.empty() ? q : order[q]];
        bptr[map[q] + 1]++;
    }
    for (uint32_t j = 0; j < nb; ++j) bptr[j + 1] += bptr[j];
    {
        std::vector<uint32_t> fill(bptr.begin(), bptr.end() - 1);
        for (uint64_t q = 0; q < N; ++q) bcase[fill[map[q]]++] = (uint32_t)q;
    }
    // the gather's launches: block rows binned by case count as the passes bin their rows
    uint32_t longb, chunk;
    fm_long_bounds(longb, chunk);
    std::vector<uint32_t> grows, gcfirst, gb[3];
    std::vector<uint4> gchunks;
    fm_bin_rows(bptr, 0, nb, longb, gb);
    for (int j = 2; j >= 0; --j) {
        if (gb[j].empty()) continue;
        FGRel::Gather l{(uint32_t)grows.size(), (uint32_t)gb[j].size(), fm_bin_tpr[j], 0, 0, 0};
        if (j == 2 && chunk) {
            l.c0 = (uint32_t)gchunks.size();
            l.f0 = (uint32_t)gcfirst.size();
            fm_cut_chunks(bptr, gb[j].data(), l.nrows, chunk, gchunks, gcfirst);
            l.nchunks = (uint32_t)gchunks.size() - l.c0;
        }
        R->gather.push_back(l);
        grows.insert(grows.end(), gb[j].begin(), gb[j].end());
    }
    upload(R->d_gchunks, gchunks, st);
    upload(R->d_gcfirst, gcfirst, st);
    R->d_gsums.alloc(std::max<size_t>(gchunks.size(), 1) * sizeof(double4));
    // the block table by block row and by attribute (block rows ascending within an attribute)
    std::vector<uint32_t> rptr((size_t)nb + 1), aptr((size_t)pa + 1, 0);
    for (uint32_t j = 0; j <= nb; ++j) rptr[j] = nb ? (uint32_t)in.ptr[j] : 0;
    for (uint64_t k = 0; k < nnz; ++k) aptr[in.attr[k] + 1]++;
    for (uint32_t a = 0; a < pa; ++a) aptr[a + 1] += aptr[a];
    std::vector<uint2> ent(nnz);
    {
        std::vector<uint32_t> fill(aptr.begin(), aptr.end() - 1);
        for (uint32_t j = 0; j < nb; ++j)
            for (uint32_t k = rptr[j]; k < rptr[j + 1]; ++k) {
                uint32_t xb;
                std::memcpy(&xb, &in.x[k], 4);
                ent[fill[in.attr[k]]++] = make_uint2(j, xb);
            }
    }
    // the ranges of the block table: two attributes that share no block row commute exactly
    std::vector<uint32_t> bounds;
    {
        std::vector<uint64_t> p64(in.ptr);
        if (p64.empty()) p64.assign(1, 0);
        sbmf_cases bt{};
        bt.n = nb;
        bt.nnz = nnz;
        bt.num_attr = pa;
        bt.ptr = p64.data();
        bt.attr = const_cast<uint32_t*>(in.attr.data());
        fm_launch_bounds(bt, pa, bounds);
    }
    nranges = (uint32_t)bounds.size() - 1;
    R->plan.build(aptr, bounds, st);
    // the records: wnum = the block row's train cases (:1217-1221), the rest 0
    std::vector<double4> rb(2 * (size_t)nb, make_double4(0.0, 0.0, 0.0, 0.0));
    for (uint32_t j = 0; j < nb; ++j) rb[2 * (size_t)j].z = (double)(bptr[j + 1] - bptr[j]);
    upload(R->d_rb, rb, st);
    upload(R->d_map, map, st);
    upload(R->d_tmap, in.test_row, st);
    upload(R->d_bptr, bptr, st);
    upload(R->d_bcase, bcase, st);
    upload(R->d_grows, grows, st);
    upload(R->d_rptr, rptr, st);
    upload(R->d_rattr, in.attr, st);
    upload(R->d_rx, in.x, st);
    upload(R->d_aptr, aptr, st);
    upload(R->d_ent, ent, st);
    HIPCHK(hipStreamSynchronize(st));  // the vectors are locals
    return R;
}

FMChain* fmg_create(const sbmf_config& c, const sbmf_cases& tr_file, const sbmf_cases& te_in, hipStream_t st,
                    const FMGroups* groups, const std::vector<FMRelation>* relations) {
    if (tr_file.n == 0) fail(SBMF_E_STATE, "no training cases");
    if (tr_file.n >= 0xffffffffull || te_in.n >= 0xffffffffull || tr_file.nnz >= 0xffffffffull || te_in.nnz >= 0xffffffffull)
        fail(SBMF_E_ARG, "more than 2^32-1 cases or features are not supported");
    OrderedCases oc;
    sbmf_cases tr_ordered{};
    const char* ord = std::getenv("SBMF_FMG_CASE_ORDER");
    // with relations the cases follow relation 0's block rows (measured: DESIGN 4.3d; SBMF_FMG_CASE_ORDER=attribute
    // keeps the order by first attribute)
    const bool by_rel = !(ord && std::strcmp(ord, "attribute") == 0) && relations && !relations->empty() &&
                        (*relations)[0].train_row.size() == tr_file.n;
    const sbmf_cases& tr_in = (by_rel ? oc.build(tr_file, tr_ordered, (*relations)[0].train_row.data(),
                                                 (uint32_t)((*relations)[0].ptr.size()))
                                      : oc.build(tr_file, tr_ordered))
                                  ? tr_ordered : tr_file;
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
    uint32_t p = std::max(tr.num_attr, te.num_attr) + 1;  // the main table's; the relations' are added below
    // ---- the ranges
    std::vector<uint32_t> bounds;
    fm_launch_bounds(tr, p, bounds);
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
    L->plan.build(aptr, bounds, st);
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
    // ---- relations: their attributes and groups follow the main table's (libfm.cpp:338-364)
    const size_t nrel = relations ? relations->size() : 0;
    if (nrel > FG_MAX_REL) fail(SBMF_E_ARG, "%zu relations: at most %u are supported", nrel, FG_MAX_REL);
    uint32_t ptot = p, gmain = 1;
    if (groups && !groups->group.empty()) {
        // group[a] for every attribute of the main table's num_attribute; one group is the ungrouped chain
        if (groups->group.size() != p)
            fail(SBMF_E_ARG, "sbmf_set_attr_groups gave %zu group ids; this context has num_attribute = %u "
                             "(max(train, test num_attr) + 1)", groups->group.size(), p);
        gmain = *std::max_element(groups->group.begin(), groups->group.end()) + 1;
    }
    L->G = gmain;
    for (size_t r = 0; r < nrel; ++r) {
        const FMRelation& in = (*relations)[r];
        if ((uint64_t)ptot + in.num_attr >= 0xfffffffeull) fail(SBMF_E_ARG, "relation %zu: attribute id too large", r);
        uint32_t nr = 0;
        L->rels.push_back(build_relation(in, (uint32_t)r, ptot, tr.n, te.n, oc.order, st, nr));
        FGRel& R = *L->rels.back();
        R.d_qbf.alloc(std::max<size_t>((size_t)R.nb * c.num_factor, 1) * sizeof(double));
        R.d_qs.alloc(std::max<size_t>(R.nb, 1) * sizeof(double));
        L->rel_info.push_back({ptot, in.num_attr, R.nb, nr, L->G, in.G});
        ptot += in.num_attr;
        L->G += in.G;
    }
    if (L->G > 65535u) fail(SBMF_E_ARG, "%u attribute groups: at most 65535 are supported", L->G);
    if (L->G > 1) {
        L->grp.assign(ptot, 0);
        if (groups && !groups->group.empty()) std::copy(groups->group.begin(), groups->group.end(), L->grp.begin());
        for (size_t r = 0; r < nrel; ++r) {
            const FMRelation& in = (*relations)[r];
            const FMChain::RelInfo& ri = L->rel_info[r];
            for (uint32_t a = 0; a < in.num_attr; ++a)
                L->grp[ri.attr_offset + a] = ri.group_offset + (in.group.empty() ? 0 : in.group[a]);
        }
    }
    if (groups && !groups->regw.empty()) {
        if (groups->regw.size() != L->G)
            fail(SBMF_E_ARG, "sbmf_set_group_regular gave %zu groups; the context has %u", groups->regw.size(), L->G);
        L->greg_w = groups->regw;
        L->greg_v = groups->regv;
    }
    p = ptot;
    L->setup(c, st, p, tr.n, tr.n, te.n, tr.target);
    L->n_launch = 0;
    return L.release();
}

}  // namespace sbmf
