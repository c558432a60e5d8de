// lists.cpp -- the score lists (ScoreList, ctx.h) and their entry points: the watch list
// (sbmf_watch_*, sbmf_recommend), the fold-in list (sbmf_foldin_*) and the libFM learner's query
// list (sbmf_fm_query_*, fmq.h); and what they share with the sample store (lists.h): the scope
// check, the top-N selection, one row's moments and the guests' CSR.
#include "ctx.h"

namespace sbmf {

// one real rank (`what`: the feature's noun), then prepared: two of the checks every scope makes
static void one_real_rank(const sbmf_ctx* c, const char* what, const char* fn) {
    if (c->virt) fail(SBMF_E_STATE, "%s: a virtual rank's numbers are not a chain; no %s there", fn, what);
    if (c->nranks > 1 || c->comm->active() || c->comm != &c->own_comm)
        fail(SBMF_E_STATE, "%s: the %s runs on one rank; this context joined a communicator", fn, what);
}
static void is_prepared(const sbmf_ctx* c, const char* fn) {
    if (!c->prepared) fail(SBMF_E_STATE, "%s: not prepared (sbmf_prepare)", fn);
}
void list_scope(const sbmf_ctx* c, const char* what, const char* fn, bool unbiased_only) {
    if (c->cfg.method != SBMF_METHOD_MCMC)
        fail(SBMF_E_STATE, "%s: the %s is offered by the SBPMF sampler (SBMF_METHOD_MCMC) only; this "
                           "context runs the %s learner", fn, what,
             c->cfg.method == SBMF_METHOD_VB ? "online VB" : c->cfg.method == SBMF_METHOD_ALS ? "ALS" : "libFM MCMC");
    if (unbiased_only && c->bias)
        fail(SBMF_E_STATE, "%s: the %s covers the unbiased quirk sets (final, sbpmf2, none); a guest of "
                           "the biased sampler (bias2 / bias22) would need a bias draw of its own", fn, what);
    one_real_rank(c, what, fn);
    is_prepared(c, fn);
}
void list_sync(sbmf_ctx* c) {
    HIPCHK(hipSetDevice(c->cfg.device));
    HIPCHK(hipStreamSynchronize(c->sto));
    HIPCHK(hipStreamSynchronize(c->st));
}

void TopnScratch::alloc(uint32_t rows, uint32_t topn, uint32_t J, bool exclude) {
    const size_t slots = (size_t)rows * topn;
    d_it.alloc(slots * sizeof(uint32_t));
    d_ms.alloc(2 * slots * sizeof(double));
    if (exclude) d_mask.alloc((size_t)rows * watch_jw(J) * sizeof(uint32_t));
}
void select_topn(TopnScratch& t, const uint32_t* d_ids, uint32_t m, const double* S1, const double* S2, uint32_t J,
                 uint32_t count, const uint32_t* csr_ptr, const uint32_t* csr_items, uint32_t topn, double risk, Span& span,
                 hipStream_t st, uint32_t* items, double* mean, double* stdev, bool given) {
    const uint32_t Jw = watch_jw(J);
    const size_t slots = (size_t)m * topn;
    uint32_t* mask = csr_ptr ? t.d_mask.as<uint32_t>() : nullptr;
    double* ms = t.d_ms.as<double>();
    span.begin(st);
    if (mask) {
        HIPCHK(hipMemsetAsync(mask, 0, (size_t)m * Jw * sizeof(uint32_t), st));
        HIPCHK(launch_watch_mask(d_ids, m, csr_ptr, csr_items, mask, Jw, st));
    }
    if (given) HIPCHK(launch_watch_select_given(m, S1, S2, J, risk, mask, topn, t.d_it.as<uint32_t>(), ms, ms + slots, st));
    else HIPCHK(launch_watch_select(m, S1, S2, J, (double)count, risk, mask, topn, t.d_it.as<uint32_t>(), ms, ms + slots, st));
    span.end(st);
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(items, t.d_it.p, slots * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(mean, ms, slots * sizeof(double), hipMemcpyDeviceToHost));
    if (stdev) HIPCHK(hipMemcpy(stdev, ms + slots, slots * sizeof(double), hipMemcpyDeviceToHost));
}
void row_moments(const double* S1, const double* S2, uint32_t J, uint32_t count, hipStream_t st, double* mean, double* stdev) {
    DBuf tmp;
    tmp.alloc((size_t)2 * J * sizeof(double));
    double* d = tmp.as<double>();
    HIPCHK(launch_watch_moments(S1, S2, J, (double)count, d, d + J, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(mean, d, (size_t)J * sizeof(double), hipMemcpyDeviceToHost));
    if (stdev) HIPCHK(hipMemcpy(stdev, d + J, (size_t)J * sizeof(double), hipMemcpyDeviceToHost));
}

void GuestCSR::check(const char* fn, uint32_t n, const uint32_t* ptr, const uint32_t* items, const double* ratings, uint32_t J) {
    if (n && !ptr) fail(SBMF_E_ARG, "%s: null ptr with n > 0", fn);
    if (n >= 0xfffffffeu) fail(SBMF_E_ARG, "%s: %u guests are too many", fn, n);
    for (uint32_t g = 0; g < n; ++g)
        if (ptr[g + 1] < ptr[g]) fail(SBMF_E_ARG, "%s: ptr decreases at guest %u (%u then %u)", fn, g, ptr[g], ptr[g + 1]);
    const uint32_t p0 = n ? ptr[0] : 0, nnz = n ? ptr[n] - p0 : 0;
    if (nnz && (!items || !ratings)) fail(SBMF_E_ARG, "%s: null items / ratings with ratings listed", fn);
    for (uint32_t q = 0; q < nnz; ++q)
        if (items[p0 + q] >= J)
            fail(SBMF_E_ARG, "%s: items[%u] = %u is not below the %u items", fn, p0 + q, items[p0 + q], J);
}
void GuestCSR::upload(uint32_t n_, const uint32_t* ptr, const uint32_t* items, const double* ratings, uint32_t rows_per_slice,
                      hipStream_t st, uint32_t* ids) {
    n = n_;
    const uint32_t p0 = ptr[0];
    nnz = ptr[n] - p0;
    std::vector<uint32_t> hp(n + 1), ident(n);
    for (uint32_t g = 0; g <= n; ++g) hp[g] = ptr[g] - p0;  // the device CSR starts at 0
    std::iota(ident.begin(), ident.end(), 0u);
    std::vector<uint32_t> order(ident);
    for (uint32_t off = 0; off < n; off += rows_per_slice)
        std::stable_sort(order.begin() + off, order.begin() + std::min(n, off + rows_per_slice),
                         [&](uint32_t x, uint32_t y) { return hp[x + 1] - hp[x] > hp[y + 1] - hp[y]; });
    d_E.alloc((size_t)nnz * sizeof(double));
    d_items.alloc((size_t)nnz * sizeof(uint32_t));
    d_ratings.alloc((size_t)nnz * sizeof(double));
    sbmf::upload(d_ptr, hp, st);
    sbmf::upload(d_order, order, st);
    if (ids) HIPCHK(hipMemcpyAsync(ids, ident.data(), ident.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    else sbmf::upload(d_ids, ident, st);
    if (nnz) {
        HIPCHK(hipMemcpyAsync(d_items.p, items + p0, (size_t)nnz * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_ratings.p, ratings + p0, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // the vectors are locals
}
void GuestCSR::drop() {
    for (DBuf* d : {&d_ptr, &d_items, &d_ratings, &d_order, &d_E, &d_ids}) d->release();
    n = nnz = 0;
}

}  // namespace sbmf

void ScoreList::alloc(uint32_t n_, uint32_t J_, int clamp_, hipStream_t st) {
    n = n_;
    J = J_;
    Jp = sbmf::watch_jp(J);
    clamp = clamp_;
    const size_t bytes = (size_t)n * Jp * sizeof(double);
    d_S1.alloc(bytes);
    d_S2.alloc(bytes);
    d_ids.alloc((size_t)n * sizeof(uint32_t));
    sel.create();
    HIPCHK(hipMemsetAsync(d_S1.p, 0, bytes, st));
    HIPCHK(hipMemsetAsync(d_S2.p, 0, bytes, st));
}
void ScoreList::drop() {
    for (sbmf::DBuf* d : {&d_ids, &d_S1, &d_S2}) d->release();
    sel.destroy();
    n = J = Jp = count = 0;
    clamp = 0;
    latest = false;
}
// this sample's scores of the list's rows of `rows` (a factor table: U, or the guests' G) against
// every item, added to the sums; the caller records the events around it
template <typename T>
void ScoreList::accumulate(sbmf_ctx* c, const T* rows, const double* bu, const double* bv, double b0, hipStream_t se) {
    HIPCHK(sbmf::launch_watch_accum<T>(d_ids.as<uint32_t>(), n, rows, c->d_V.as<T>(), c->J, c->Kp, bu, bv, b0, clamp,
                                       c->lo, c->hi, d_S1.as<double>(), d_S2.as<double>(), se));
    count++;
    c->launches++;
}
template void ScoreList::accumulate<float>(sbmf_ctx*, const float*, const double*, const double*, double, hipStream_t);
template void ScoreList::accumulate<double>(sbmf_ctx*, const double*, const double*, const double*, double, hipStream_t);
void ScoreList::scores(sbmf_ctx* c, const char* fn, uint32_t row, double* mean, double* stdev) {
    if (row >= n) sbmf::fail(SBMF_E_ARG, "%s: row %u of a %s of %u", fn, row, what, n);
    sbmf::row_moments(d_S1.as<double>() + (size_t)row * Jp, d_S2.as<double>() + (size_t)row * Jp, J, count, c->st, mean, stdev);
    if (stdev && latest) std::fill(stdev, stdev + J, 0.0);
}
// top-N of every row; "rated" items (flags bit 0 clear: left out) are those of the rows' CSR --
// the user side's for watched users, the guest CSR for guests
void ScoreList::recommend(sbmf_ctx* c, const uint32_t* csr_ptr, const uint32_t* csr_items, uint32_t topn,
                          uint32_t flags, double risk, uint32_t* items, double* mean, double* stdev) {
    const bool exclude = !(flags & 1u);
    sbmf::TopnScratch t;
    t.alloc(n, topn, J, exclude);
    sbmf::select_topn(t, d_ids.as<uint32_t>(), n, d_S1.as<double>(), d_S2.as<double>(), J, count, exclude ? csr_ptr : nullptr,
                      csr_items, topn, risk, sel, c->st, items, mean, stdev);
    if (stdev && latest)  // one sample: no spread (the empty slots keep their NaN)
        for (size_t q = 0, slots = (size_t)n * topn; q < slots; ++q)
            if (items[q] != 0xffffffffu) stdev[q] = 0.0;
}

extern "C" {

static void list_registered(const ScoreList& l, const char* fn) {
    if (!l.n) sbmf::fail(SBMF_E_STATE, "%s: no %s registered (%s)", fn, l.what, l.reg);
}
// registered, and (sums) at least one sweep accumulated; `note`: what else the caller has to say
// about a list with none
static void list_ready(sbmf_ctx* c, const ScoreList& l, const char* fn, bool sums = true, const char* note = "") {
    list_registered(l, fn);
    if (sums && !l.count)
        sbmf::fail(SBMF_E_STATE, "%s: no sweep accumulated since the %s was registered%s", fn, l.what, note);
    list_sync(c);
}
// the arguments sbmf_recommend and sbmf_foldin_recommend share
static void recommend_args(const char* fn, uint32_t topn, uint32_t flags, double risk) {
    if (topn < 1 || topn > 1024) sbmf::fail(SBMF_E_ARG, "%s: topn %u is not in 1..1024", fn, topn);
    if (flags & ~1u) sbmf::fail(SBMF_E_ARG, "%s: unknown flags 0x%x (bit 0 = keep rated items)", fn, flags & ~1u);
    if (!(risk == risk)) sbmf::fail(SBMF_E_ARG, "%s: risk is NaN", fn);
}

static void watch_drop(sbmf_ctx* c) {
    c->watch.drop();
    for (hipEvent_t& e : c->wev) sbmf::event_destroy(e);
}

int sbmf_watch_users(sbmf_ctx* ctx, uint32_t n, const uint32_t* users, uint32_t flags) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    list_scope(ctx, ctx->watch.what, "sbmf_watch_users", false);
    if (n && !users) sbmf::fail(SBMF_E_ARG, "null user list with n > 0");
    if (flags & ~1u) sbmf::fail(SBMF_E_ARG, "sbmf_watch_users: unknown flags 0x%x (bit 0 = clamp)", flags & ~1u);
    for (uint32_t w = 0; w < n; ++w)
        if (users[w] >= ctx->I)
            sbmf::fail(SBMF_E_ARG, "sbmf_watch_users: users[%u] = %u is not below the %u users", w, users[w], ctx->I);
    list_sync(ctx);
    watch_drop(ctx);
    if (n == 0) return SBMF_OK;
    try {
        ctx->watch.alloc(n, ctx->J, (int)(flags & 1u), ctx->st);
        for (hipEvent_t& e : ctx->wev) sbmf::event_create(&e);
        HIPCHK(hipMemcpyAsync(ctx->watch.d_ids.p, users, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->st));
        HIPCHK(hipStreamSynchronize(ctx->st));
    } catch (...) {
        watch_drop(ctx);
        throw;
    }
    API_END(ctx)
}

int sbmf_watch_scores(sbmf_ctx* ctx, uint32_t w, double* mean, double* stdev) {
    API_BEGIN
    if (!ctx || !mean) sbmf::fail(SBMF_E_ARG, "null argument");
    list_scope(ctx, ctx->watch.what, "sbmf_watch_scores", false);
    list_ready(ctx, ctx->watch, "sbmf_watch_scores");
    ctx->watch.scores(ctx, "sbmf_watch_scores", w, mean, stdev);
    API_END(ctx)
}

int sbmf_recommend(sbmf_ctx* ctx, uint32_t topn, uint32_t flags, double risk, uint32_t* items, double* mean,
                   double* stdev) {
    API_BEGIN
    if (!ctx || !items || !mean) sbmf::fail(SBMF_E_ARG, "null argument");
    list_scope(ctx, ctx->watch.what, "sbmf_recommend", false);
    recommend_args("sbmf_recommend", topn, flags, risk);
    list_ready(ctx, ctx->watch, "sbmf_recommend");
    ctx->watch.recommend(ctx, ctx->d_uptr.as<uint32_t>(), ctx->d_upart.as<uint32_t>(), topn, flags, risk, items, mean,
                         stdev);
    API_END(ctx)
}

int sbmf_watch_timing(sbmf_ctx* ctx, double* ms_score, double* ms_select) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    list_scope(ctx, ctx->watch.what, "sbmf_watch_timing", false);
    list_registered(ctx->watch, "sbmf_watch_timing");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    if (ms_score) {
        *ms_score = 0.0;
        if (ctx->watch.count) {
            HIPCHK(hipEventSynchronize(ctx->wev[1]));
            *ms_score = sbmf::ev_ms(ctx->wev[0], ctx->wev[1]);
        }
    }
    if (ms_select) *ms_select = ctx->watch.sel.ms();
    API_END(ctx)
}

// --- fold-in list ----------------------------------------------------------------------------
static void foldin_drop(sbmf_ctx* c) {
    c->guests.drop();
    c->fcsr.drop();
    c->d_fG.release();
    c->d_fhyp.release();
    sbmf::pinned_free(c->h_fhyp, c->h_fhyp_bytes);
    c->h_fhyp_bytes = 0;
    for (hipEvent_t& e : c->fev) sbmf::event_destroy(e);
    c->fdrawn = 0;
}
static void foldin_ready(sbmf_ctx* c, const char* fn, bool sums) {
    if (c->guests.n && !c->fdrawn)
        sbmf::fail(SBMF_E_STATE, "%s: no sweep drawn since the fold-in list was registered", fn);
    list_ready(c, c->guests, fn, sums, " (burn-in sweeps draw the rows but are not collected)");
}

int sbmf_foldin_users(sbmf_ctx* ctx, uint32_t n, const uint32_t* ptr, const uint32_t* items, const double* ratings,
                      uint32_t flags) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    list_scope(ctx, ctx->guests.what, "sbmf_foldin_users", true);
    if (flags & ~1u) sbmf::fail(SBMF_E_ARG, "sbmf_foldin_users: unknown flags 0x%x (bit 0 = clamp)", flags & ~1u);
    sbmf::GuestCSR::check("sbmf_foldin_users", n, ptr, items, ratings, ctx->J);
    const uint32_t nnz = n ? ptr[n] - ptr[0] : 0;
    list_sync(ctx);
    foldin_drop(ctx);
    if (n == 0) return SBMF_OK;
    const uint32_t Jp = sbmf::watch_jp(ctx->J), Kp = ctx->Kp;
    const size_t ts = sbmf::tsize(ctx);
    const size_t b_sum = (size_t)n * Jp * sizeof(double), b_G = ((size_t)n + 2) * Kp * ts;
    const size_t b_tot = 2 * b_sum + b_G + ((size_t)n + 1 + 2 * (size_t)n + nnz) * sizeof(uint32_t) +
                         ((size_t)2 * nnz + 2 * Kp) * sizeof(double);
    try {
        hipStream_t st = ctx->st;
        ctx->guests.alloc(n, ctx->J, (int)(flags & 1u), st);
        ctx->d_fG.alloc(b_G);
        ctx->d_fhyp.alloc((size_t)2 * Kp * sizeof(double));
        sbmf::pinned_alloc((void**)&ctx->h_fhyp, (size_t)2 * Kp * sizeof(double));
        ctx->h_fhyp_bytes = (size_t)2 * Kp * sizeof(double);
        for (hipEvent_t& e : ctx->fev) sbmf::event_create(&e);
        HIPCHK(hipMemsetAsync(ctx->d_fG.p, 0, b_G, st));
        // one slice: the whole list in one launch (the upload's synchronisation covers the memsets)
        ctx->fcsr.upload(n, ptr, items, ratings, n, st, ctx->guests.d_ids.as<uint32_t>());
    } catch (const sbmf::Error& e) {
        foldin_drop(ctx);
        if (e.code == SBMF_E_NOMEM)
            sbmf::fail(SBMF_E_NOMEM, "sbmf_foldin_users: %u guests with %u ratings need %zu bytes of device memory: %s", n,
                       nnz, b_tot, e.msg.c_str());
        throw;
    } catch (...) {
        foldin_drop(ctx);
        throw;
    }
    API_END(ctx)
}

int sbmf_foldin_factors(sbmf_ctx* ctx, double* rows) {
    API_BEGIN
    if (!ctx || !rows) sbmf::fail(SBMF_E_ARG, "null argument");
    list_scope(ctx, ctx->guests.what, "sbmf_foldin_factors", true);
    foldin_ready(ctx, "sbmf_foldin_factors", false);
    sbmf::download_table(ctx, ctx->d_fG, rows, ctx->guests.n);
    API_END(ctx)
}

int sbmf_foldin_scores(sbmf_ctx* ctx, uint32_t g, double* mean, double* stdev) {
    API_BEGIN
    if (!ctx || !mean) sbmf::fail(SBMF_E_ARG, "null argument");
    list_scope(ctx, ctx->guests.what, "sbmf_foldin_scores", true);
    foldin_ready(ctx, "sbmf_foldin_scores", true);
    ctx->guests.scores(ctx, "sbmf_foldin_scores", g, mean, stdev);
    API_END(ctx)
}

int sbmf_foldin_recommend(sbmf_ctx* ctx, uint32_t topn, uint32_t flags, double risk, uint32_t* items, double* mean,
                          double* stdev) {
    API_BEGIN
    if (!ctx || !items || !mean) sbmf::fail(SBMF_E_ARG, "null argument");
    list_scope(ctx, ctx->guests.what, "sbmf_foldin_recommend", true);
    recommend_args("sbmf_foldin_recommend", topn, flags, risk);
    foldin_ready(ctx, "sbmf_foldin_recommend", true);
    // "rated": the guest's own items (the guest CSR in the user-side CSR's place)
    ctx->guests.recommend(ctx, ctx->fcsr.d_ptr.as<uint32_t>(), ctx->fcsr.d_items.as<uint32_t>(), topn, flags, risk, items, mean,
                          stdev);
    API_END(ctx)
}

int sbmf_foldin_timing(sbmf_ctx* ctx, double* ms_draw, double* ms_score, double* ms_select) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    list_scope(ctx, ctx->guests.what, "sbmf_foldin_timing", true);
    list_registered(ctx->guests, "sbmf_foldin_timing");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    if (ms_draw) *ms_draw = 0.0;
    if (ms_score) *ms_score = 0.0;
    if (ctx->fdrawn) {
        list_sync(ctx);
        if (ms_draw) *ms_draw = sbmf::ev_ms(ctx->fev[0], ctx->fev[1]);
        // (collected sweeps follow the burn-in: once a scoring launch was timed, the last
        // sweep's draw end is its begin)
        if (ms_score && ctx->guests.count) *ms_score = sbmf::ev_ms(ctx->fev[1], ctx->fev[2]);
    }
    if (ms_select) *ms_select = ctx->guests.sel.ms();
    API_END(ctx)
}

// --- query list of libFM's MCMC / ALS learner ---------------------------------------------------
static void fmq_drop(sbmf_ctx* c) {
    if (c->fm) c->fm->query = nullptr;
    c->fmq.drop();
    c->fmqd.drop();
}
// The contexts the query list covers: the general libFM learner with relations, on one rank.
static void fmq_scope(const sbmf_ctx* c, const char* fn) {
    sbmf::one_real_rank(c, "query list", fn);
    if (c->cfg.method != SBMF_METHOD_LIBFM_MCMC && c->cfg.method != SBMF_METHOD_ALS)
        sbmf::fail(SBMF_E_STATE, "%s: the query list is offered by libFM's MCMC / ALS learner (SBMF_METHOD_LIBFM_MCMC, "
                                 "SBMF_METHOD_ALS) only; this context runs the %s (its lists: sbmf_watch_users, "
                                 "sbmf_foldin_users)", fn, c->cfg.method == SBMF_METHOD_VB ? "online VB learner" : "SBPMF sampler");
    sbmf::is_prepared(c, fn);
    if (!c->fm || c->fm->rel_info.empty())
        sbmf::fail(SBMF_E_STATE, "%s: this context has no relations (sbmf_add_relation): the candidates of a query "
                                 "list are the block rows of one", fn);
}

int sbmf_fm_query_cases(sbmf_ctx* ctx, uint32_t relation, const sbmf_cases* queries, const uint32_t* const* rows,
                        const uint32_t* excl_ptr, const uint32_t* excl_rows, uint32_t flags) {
    API_BEGIN
    const char* fn = "sbmf_fm_query_cases";
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (!queries) sbmf::fail(SBMF_E_ARG, "%s: null queries", fn);
    fmq_scope(ctx, fn);
    sbmf::FMChain& fm = *ctx->fm;
    const uint32_t nrel = (uint32_t)fm.rel_info.size();
    if (flags & ~1u) sbmf::fail(SBMF_E_ARG, "%s: unknown flags 0x%x (bit 0 = clamp)", fn, flags & ~1u);
    if (relation >= nrel)
        sbmf::fail(SBMF_E_ARG, "%s: relation %u is not below the context's %u relations", fn, relation, nrel);
    if (queries->n == 0) {
        list_sync(ctx);
        fmq_drop(ctx);
        return SBMF_OK;
    }
    if (queries->n >= 0xfffffffeull || queries->nnz >= 0xffffffffull)
        sbmf::fail(SBMF_E_ARG, "%s: %llu queries with %llu features are too many", fn, (unsigned long long)queries->n,
                   (unsigned long long)queries->nnz);
    const uint32_t n = (uint32_t)queries->n, nnz = (uint32_t)queries->nnz;
    if (!queries->ptr || (nnz && (!queries->attr || !queries->x))) sbmf::fail(SBMF_E_ARG, "%s: null array in queries", fn);
    if (queries->ptr[0] != 0 || queries->ptr[n] != nnz) sbmf::fail(SBMF_E_ARG, "%s: queries ptr must run from 0 to nnz", fn);
    for (uint32_t q = 0; q < n; ++q)
        if (queries->ptr[q + 1] < queries->ptr[q] || queries->ptr[q + 1] > nnz)
            sbmf::fail(SBMF_E_ARG, "%s: queries ptr decreases at query %u", fn, q);
    const uint32_t p_main = fm.rel_info[0].attr_offset;
    for (uint32_t k = 0; k < nnz; ++k)
        if (queries->attr[k] >= p_main)
            sbmf::fail(SBMF_E_ARG, "%s: attr[%u] = %u is not a main attribute id (below attr_offset_0 = %u); the "
                                   "relations' features come from the block rows", fn, k, queries->attr[k], p_main);
    for (uint32_t r = 0; r < nrel; ++r) {
        if (r == relation) continue;
        if (!rows || !rows[r])
            sbmf::fail(SBMF_E_ARG, "%s: rows[%u] is missing: every query joins one block row of each relation but "
                                   "the candidates' (%u)", fn, r, relation);
        for (uint32_t q = 0; q < n; ++q)
            if (rows[r][q] >= fm.rel_info[r].block_rows)
                sbmf::fail(SBMF_E_ARG, "%s: rows[%u][%u] = %u is not below relation %u's %u block rows", fn, r, q,
                           rows[r][q], r, fm.rel_info[r].block_rows);
    }
    const uint32_t nb = fm.rel_info[relation].block_rows;
    if (nb == 0) sbmf::fail(SBMF_E_ARG, "%s: relation %u has no block rows", fn, relation);
    if ((excl_rows && !excl_ptr) || (excl_ptr && !excl_rows && excl_ptr[n] != excl_ptr[0]))
        sbmf::fail(SBMF_E_ARG, "%s: excl_ptr and excl_rows go together (both NULL: no exclusions)", fn);
    uint32_t nex = 0;
    if (excl_ptr) {
        for (uint32_t q = 0; q < n; ++q)
            if (excl_ptr[q + 1] < excl_ptr[q])
                sbmf::fail(SBMF_E_ARG, "%s: excl_ptr decreases at query %u (%u then %u)", fn, q, excl_ptr[q], excl_ptr[q + 1]);
        nex = excl_ptr[n] - excl_ptr[0];
        for (uint32_t k = 0; k < nex; ++k)
            if (excl_rows[excl_ptr[0] + k] >= nb)
                sbmf::fail(SBMF_E_ARG, "%s: excl_rows[%u] = %u is not below relation %u's %u block rows", fn,
                           excl_ptr[0] + k, excl_rows[excl_ptr[0] + k], relation, nb);
    }
    list_sync(ctx);
    fmq_drop(ctx);
    const uint32_t Kp = fm.Kp, nbp = sbmf::watch_jp(nb);
    const size_t b_sum = (size_t)n * nbp * sizeof(double);
    const size_t b_tot = 2 * b_sum + ((size_t)n * (Kp + 1) + nb) * sizeof(double) + sbmf::fmq_operand_bytes(nb, Kp) +
                         ((size_t)2 * n + 2 + (size_t)nrel * n + nex) * sizeof(uint32_t) + (size_t)nnz * 8 + n * sizeof(uint32_t);
    try {
        hipStream_t st = ctx->st;
        // the sums first: a list the device cannot hold fails here, before any host copy is made
        ctx->fmq.alloc(n, nb, (int)(flags & 1u), st);
        ctx->fmq.latest = ctx->cfg.method == SBMF_METHOD_ALS;
        // the queries as the learner keeps its cases: entries in ascending attribute (stable)
        std::vector<uint32_t> ptr(n + 1), attr(nnz), ident(n), hrows((size_t)nrel * n, 0), ord;
        std::vector<float> x(nnz);
        for (uint32_t q = 0; q <= n; ++q) ptr[q] = (uint32_t)queries->ptr[q];
        for (uint32_t q = 0; q < n; ++q) {
            ident[q] = q;
            const uint32_t b = ptr[q], m = ptr[q + 1] - b;
            ord.resize(m);
            std::iota(ord.begin(), ord.end(), 0u);
            std::stable_sort(ord.begin(), ord.end(),
                             [&](uint32_t i, uint32_t j) { return queries->attr[b + i] < queries->attr[b + j]; });
            for (uint32_t k = 0; k < m; ++k) {
                attr[b + k] = queries->attr[b + ord[k]];
                x[b + k] = queries->x[b + ord[k]];
            }
        }
        for (uint32_t r = 0; r < nrel; ++r)
            if (r != relation) std::copy(rows[r], rows[r] + n, hrows.begin() + (size_t)r * n);
        sbmf::FMQueryList& ql = ctx->fmqd;
        sbmf::upload(ctx->fmq.d_ids, ident, st);
        sbmf::upload(ql.d_ptr, ptr, st);
        sbmf::upload(ql.d_attr, attr, st);
        sbmf::upload(ql.d_x, x, st);
        sbmf::upload(ql.d_rows, hrows, st);
        ql.d_s.alloc((size_t)n * Kp * sizeof(double));
        ql.d_a.alloc((size_t)n * sizeof(double));
        ql.d_B.alloc(sbmf::fmq_operand_bytes(nb, Kp));
        ql.d_y.alloc((size_t)nb * sizeof(double));
        if (nex) {
            std::vector<uint32_t> ep(n + 1);
            for (uint32_t q = 0; q <= n; ++q) ep[q] = excl_ptr[q] - excl_ptr[0];  // the device CSR starts at 0
            sbmf::upload(ql.d_eptr, ep, st);
            ql.d_erows.alloc((size_t)nex * sizeof(uint32_t));
            HIPCHK(hipMemcpyAsync(ql.d_erows.p, excl_rows + excl_ptr[0], (size_t)nex * sizeof(uint32_t),
                                  hipMemcpyHostToDevice, st));
            HIPCHK(hipStreamSynchronize(st));  // ep is a local
        }
        for (hipEvent_t& e : ql.ev) sbmf::event_create(&e);
        HIPCHK(hipStreamSynchronize(st));  // the vectors are locals
        ql.rel = relation;
        ql.nq = n;
        ql.nb = nb;
        ql.clamp = (int)(flags & 1u);
        ql.ids = ctx->fmq.d_ids.as<uint32_t>();
        ql.S1 = ctx->fmq.d_S1.as<double>();
        ql.S2 = ctx->fmq.d_S2.as<double>();
        ql.count = &ctx->fmq.count;
        fm.query = &ql;
    } catch (const sbmf::Error& e) {
        fmq_drop(ctx);
        if (e.code == SBMF_E_NOMEM)
            sbmf::fail(SBMF_E_NOMEM, "%s: %u queries against %u block rows need %zu bytes of device memory: %s", fn, n,
                       nb, b_tot, e.msg.c_str());
        throw;
    } catch (...) {
        fmq_drop(ctx);
        throw;
    }
    API_END(ctx)
}

int sbmf_fm_query_scores(sbmf_ctx* ctx, uint32_t q, double* mean, double* stdev) {
    API_BEGIN
    if (!ctx || !mean) sbmf::fail(SBMF_E_ARG, "null argument");
    fmq_scope(ctx, "sbmf_fm_query_scores");
    list_ready(ctx, ctx->fmq, "sbmf_fm_query_scores", true, " (every iteration of sbmf_run accumulates one)");
    ctx->fmq.scores(ctx, "sbmf_fm_query_scores", q, mean, stdev);
    API_END(ctx)
}

int sbmf_fm_query_recommend(sbmf_ctx* ctx, uint32_t topn, uint32_t flags, double risk, uint32_t* rows, double* mean,
                            double* stdev) {
    API_BEGIN
    if (!ctx || !rows || !mean) sbmf::fail(SBMF_E_ARG, "null argument");
    fmq_scope(ctx, "sbmf_fm_query_recommend");
    recommend_args("sbmf_fm_query_recommend", topn, flags, risk);
    list_ready(ctx, ctx->fmq, "sbmf_fm_query_recommend", true, " (every iteration of sbmf_run accumulates one)");
    // "rated": the query's exclusion list (none registered: nothing is left out)
    if (!ctx->fmqd.d_eptr.p) flags |= 1u;
    ctx->fmq.recommend(ctx, ctx->fmqd.d_eptr.as<uint32_t>(), ctx->fmqd.d_erows.as<uint32_t>(), topn, flags, risk, rows,
                       mean, stdev);
    API_END(ctx)
}

int sbmf_fm_query_timing(sbmf_ctx* ctx, double* ms_terms, double* ms_score, double* ms_select) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    fmq_scope(ctx, "sbmf_fm_query_timing");
    list_registered(ctx->fmq, "sbmf_fm_query_timing");
    if (ms_terms) *ms_terms = 0.0;
    if (ms_score) *ms_score = 0.0;
    if (ctx->fmq.count) {
        list_sync(ctx);
        if (ms_terms) *ms_terms = sbmf::ev_ms(ctx->fmqd.ev[0], ctx->fmqd.ev[1]);
        if (ms_score) *ms_score = sbmf::ev_ms(ctx->fmqd.ev[1], ctx->fmqd.ev[2]);
    }
    if (ms_select) *ms_select = ctx->fmq.sel.ms();
    API_END(ctx)
}

int sbmf_test_watch_lds(uint32_t Kp, uint32_t* rows, uint64_t* bytes) {
    sbmf_ctx* ctx = nullptr;
    API_BEGIN
    if (!rows || !bytes) sbmf::fail(SBMF_E_ARG, "null argument");
    const int mu = sbmf::watch_mu(Kp);
    *rows = 16u * (uint32_t)mu;
    *bytes = sbmf::watch_lds_bytes(mu, Kp);
    API_END(ctx)
}

}  // extern "C"
