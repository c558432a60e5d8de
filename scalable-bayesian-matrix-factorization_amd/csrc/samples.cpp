// samples.cpp -- the posterior sample store (SampleStore, ctx.h) and its entry points: keeping
// thinned samples of the SBPMF chain on the device (sbmf_keep_samples; the copy runs in the sweep's
// evaluation, sweep.cpp), scoring users and pairs from them after the run (samples.hip); the
// samples' hyperparameters, and guests drawn from the stored samples after the run
// (sbmf_samples_foldin_*; samples_foldin.hip).  The store's files: samples_file.cpp.
#include "ctx.h"

namespace sbmf {

void samples_ready(sbmf_ctx* c, const char* fn) {
    list_scope(c, "sample store", fn, false);
    if (!c->samples.cap || !c->samples.count)
        fail(SBMF_E_STATE, "%s: no sample kept yet (sbmf_keep_samples, then a collected sweep; or sbmf_load_samples)", fn);
    list_sync(c);
}
size_t slot_bytes(const sbmf_ctx* c) {
    return ((size_t)c->I + c->J) * c->Kp * tsize(c) + (c->bias ? ((size_t)c->I + c->J) * sizeof(double) : 0);
}

}  // namespace sbmf

namespace {

// The store as the kernels read it; d_b0: the samples' b0 in order of age (biased sampler)
sbmf::SampleView view_of(sbmf_ctx* c, sbmf::DBuf& d_b0, hipStream_t st) {
    const SampleStore& ss = c->samples;
    sbmf::SampleView v;
    v.U = ss.d_U.p;
    v.V = ss.d_V.p;
    v.su = (size_t)c->I * c->Kp;
    v.sv = (size_t)c->J * c->Kp;
    v.head = ss.head;
    v.cap = ss.cap;
    v.count = ss.count;
    if (c->bias) {
        std::vector<double> b(ss.count);
        for (uint32_t s = 0; s < ss.count; ++s) b[s] = ss.b0[ss.slot(s)];
        sbmf::upload(d_b0, b, st);
        HIPCHK(hipStreamSynchronize(st));  // b is a local
        v.bu = ss.d_bu.as<double>();
        v.bv = ss.d_bv.as<double>();
        v.b0 = d_b0.as<double>();
        v.sbu = c->I;
        v.sbv = c->J;
    }
    return v;
}

// S1 / S2 [n][Jp] of the users d_ids[0..n) over every stored sample: the fused kernel, or (test
// hook) one launch_watch_accum per sample into zeroed sums -- the same values, the sums passing
// through memory once per sample
template <typename T>
void score_rows(sbmf_ctx* c, const sbmf::SampleView& v, const uint32_t* d_ids, uint32_t n, int clamp, double* S1,
                double* S2, hipStream_t st) {
    if (!c->samples.unfused) {
        HIPCHK(sbmf::launch_samples_score<T>(v, d_ids, n, c->J, c->Kp, clamp, c->lo, c->hi, S1, S2, st));
        return;
    }
    const size_t bytes = (size_t)n * sbmf::watch_jp(c->J) * sizeof(double);
    HIPCHK(hipMemsetAsync(S1, 0, bytes, st));
    HIPCHK(hipMemsetAsync(S2, 0, bytes, st));
    for (uint32_t s = 0; s < v.count; ++s) {
        const size_t p = c->samples.slot(s);
        HIPCHK(sbmf::launch_watch_accum<T>(d_ids, n, static_cast<const T*>(v.U) + p * v.su, static_cast<const T*>(v.V) + p * v.sv,
                                           c->J, c->Kp, v.bu ? v.bu + p * v.sbu : nullptr, v.bv ? v.bv + p * v.sbv : nullptr,
                                           c->bias ? c->samples.b0[p] : 0.0, clamp, c->lo, c->hi, S1, S2, st));
    }
}
void score_rows(sbmf_ctx* c, const sbmf::SampleView& v, const uint32_t* d_ids, uint32_t n, int clamp, double* S1, double* S2,
                hipStream_t st) {
    c->cfg.precision == SBMF_F32 ? score_rows<float>(c, v, d_ids, n, clamp, S1, S2, st)
                                 : score_rows<double>(c, v, d_ids, n, clamp, S1, S2, st);
}

void check_users(const sbmf_ctx* c, const char* fn, uint64_t n, const uint32_t* users) {
    for (uint64_t w = 0; w < n; ++w)
        if (users[w] >= c->I)
            sbmf::fail(SBMF_E_ARG, "%s: users[%llu] = %u is not below the %u users", fn, (unsigned long long)w, users[w], c->I);
}

// the temporaries' budget of sbmf_samples_recommend: S1 and S2 of one slice of users
constexpr uint64_t kBudget = 1ull << 30;

// ------------------------------------------------------------------ guests from the stored samples
// What the three guest calls check before anything is allocated.
void guests_ready(sbmf_ctx* c, const char* fn, uint32_t n, const uint32_t* ptr, const uint32_t* items, const double* ratings,
                  uint32_t scans) {
    list_scope(c, "sample store", fn, false);
    if (c->bias)
        sbmf::fail(SBMF_E_STATE, "%s: guests are folded into a store of the unbiased quirk sets (final, sbpmf2, none); a "
                                 "guest bias would need a draw of its own", fn);
    if (scans < 1 || scans > sbmf::SAMPLES_FOLDIN_SCANS_MAX)
        sbmf::fail(SBMF_E_ARG, "%s: scans %u is not in 1..%u", fn, scans, sbmf::SAMPLES_FOLDIN_SCANS_MAX);
    sbmf::GuestCSR::check(fn, n, ptr, items, ratings, c->J);
    samples_ready(c, fn);
    if (!c->samples.has_hyper)
        sbmf::fail(SBMF_E_STATE, "%s: the stored samples have no hyperparameters (a sample file holds none: "
                                 "sbmf_load_samples_hyper loads its companion file)", fn);
}

// One guest call: the guests' CSR and what the draw reads of the samples on the device, the
// slices' temporaries, and the draw / scoring of one slice.  Everything is freed with the object.
struct GuestCall {
    sbmf_ctx* c;
    const char* fn;
    uint32_t n, nnz, scans, rows = 0;  // rows: guests per slice
    size_t gs = 0;                     // elements of one sample's GS table: (rows + 2) Kp
    sbmf::GuestCSR csr;  // (its order: by falling length within each slice)
    sbmf::DBuf d_hyp, d_tau, d_sw, d_GS, d_S1, d_S2, d_b0;
    sbmf::SamplesFoldinArgs a;

    // sums: the slice also holds S1 / S2 [rows][Jp] (else only the rows are wanted)
    GuestCall(sbmf_ctx* c_, const char* fn_, uint32_t n_, const uint32_t* ptr, const uint32_t* items, const double* ratings,
              uint32_t scans_, bool sums)
        : c(c_), fn(fn_), n(n_), nnz(n_ ? ptr[n_] - ptr[0] : 0), scans(scans_) {
        const SampleStore& ss = c->samples;
        const uint32_t K = c->K, Kp = c->Kp, Jp = sbmf::watch_jp(c->J), count = ss.count;
        const size_t ts = sbmf::tsize(c);
        // guests per slice: as many as the budget holds of two sums' rows and `count` factor rows,
        // in whole workgroups of 64, one at least
        const uint64_t budget = ss.budget ? ss.budget : kBudget;
        const uint64_t per = (sums ? (uint64_t)2 * Jp * sizeof(double) : 0) + (uint64_t)count * Kp * ts;
        rows = (uint32_t)std::min<uint64_t>(n, std::max<uint64_t>(budget / per / 64 * 64, 64));
        gs = ((size_t)rows + 2) * Kp;
        const size_t b_GS = (size_t)count * gs * ts, b_sum = sums ? (size_t)rows * Jp * sizeof(double) : 0;
        const size_t b_tot = b_GS + 2 * b_sum + ((size_t)n + 1 + 3 * (size_t)n + nnz + count) * sizeof(uint32_t) +
                             ((size_t)2 * nnz + (size_t)count * (2 * Kp + 1)) * sizeof(double) +
                             (ss.fused_draw ? 0 : (size_t)rows * Kp * sizeof(double));
        try {
            hipStream_t st = c->st;
            // the samples' [sig_u | mu_u], tau and sweep index, oldest first
            std::vector<double> hyp((size_t)count * 2 * Kp, 0.0), tau(count);
            std::vector<uint32_t> sw(count);
            for (uint32_t s = 0; s < count; ++s) {
                const uint32_t p = ss.slot(s);
                const double* h = ss.hyper.data() + (size_t)p * (4 * K + 1);
                std::copy(h, h + K, hyp.begin() + (size_t)s * 2 * Kp);
                std::copy(h + K, h + 2 * K, hyp.begin() + (size_t)s * 2 * Kp + Kp);
                tau[s] = h[4 * K];
                sw[s] = ss.sweep[p];
            }
            // (the per-launch form's carry [rows][Kp] doubles sits behind GS in the same allocation)
            d_GS.alloc(b_GS + (ss.fused_draw ? 0 : (size_t)rows * Kp * sizeof(double)));
            if (sums) {
                d_S1.alloc(b_sum);
                d_S2.alloc(b_sum);
            }
            sbmf::upload(d_hyp, hyp, st);
            sbmf::upload(d_tau, tau, st);
            sbmf::upload(d_sw, sw, st);
            a.sv = view_of(c, d_b0, st);
            csr.upload(n, ptr, items, ratings, rows, st);  // (its synchronisation covers the vectors above: locals)
        } catch (const sbmf::Error& e) {
            if (e.code == SBMF_E_NOMEM)
                sbmf::fail(SBMF_E_NOMEM, "%s: %u guests with %u ratings at %u samples need %zu bytes of device memory: %s", fn,
                           n, nnz, count, b_tot, e.msg.c_str());
            throw;
        }
        // A sample's GS table sits at its ring slot, so the scoring kernel reads GS through the
        // store's own view (one head and cap for both sides): a store that has not wrapped has
        // head 0, a wrapped one is full -- the `count` slots in use are 0..count-1 either way.
        a.GS = d_GS.p;
        a.gs = gs;
        a.ptr = csr.d_ptr.as<uint32_t>();
        a.items = csr.d_items.as<uint32_t>();
        a.ratings = csr.d_ratings.as<double>();
        a.K = K;
        a.Kp = Kp;
        a.hyper = d_hyp.as<double>();
        a.tau = d_tau.as<double>();
        a.sweeps = d_sw.as<uint32_t>();
        a.scans = scans;
        a.sd_is_var = c->sd_is_var;
        a.seed = c->cfg.seed;
        a.E = csr.d_E.as<double>();
    }

    // the rows of the guests off .. off + m - 1 at every sample into GS (events: ss.gdr)
    template <typename T>
    void draw_T(uint32_t off, uint32_t m) {
        SampleStore& ss = c->samples;
        hipStream_t st = c->st;
        a.n = m;
        a.g0 = off;
        a.order = csr.d_order.as<uint32_t>() + off;
        HIPCHK(hipMemsetAsync(d_GS.p, 0, d_GS.bytes, st));
        ss.gdr.begin(st);
        if (ss.fused_draw) {
            HIPCHK(sbmf::launch_samples_foldin<T>(a, st));
        } else {  // the memset above zeroed the carry too
            double* carry = reinterpret_cast<double*>(static_cast<char*>(d_GS.p) + (size_t)ss.count * gs * sizeof(T));
            for (uint32_t s = 0; s < ss.count; ++s)
                for (uint32_t r = 0; r < scans; ++r) HIPCHK(sbmf::launch_samples_foldin_step<T>(a, s, r, carry, st));
        }
        ss.gdr.end(st);
    }
    void draw(uint32_t off, uint32_t m) {
        c->cfg.precision == SBMF_F32 ? draw_T<float>(off, m) : draw_T<double>(off, m);
    }
    // S1 / S2 of the slice just drawn: the store's scoring kernel, GS in U's place, rows 0..m-1
    void score(uint32_t m, int clamp) {
        SampleStore& ss = c->samples;
        sbmf::SampleView v = a.sv;
        v.U = d_GS.p;
        v.su = gs;
        ss.gsc.begin(c->st);
        score_rows(c, v, csr.d_ids.as<uint32_t>(), m, clamp, d_S1.as<double>(), d_S2.as<double>(), c->st);
        ss.gsc.end(c->st);
    }
};

}  // namespace

void SampleStore::alloc(sbmf_ctx* c, uint32_t cap_, uint32_t every_) {
    const size_t ts = sbmf::tsize(c), I = c->I, J = c->J, Kp = c->Kp;
    d_U.alloc((size_t)cap_ * I * Kp * ts);
    d_V.alloc((size_t)cap_ * J * Kp * ts);
    if (c->bias) {
        d_bu.alloc((size_t)cap_ * I * sizeof(double));
        d_bv.alloc((size_t)cap_ * J * sizeof(double));
    }
    for (sbmf::Span* s : {&cev, &scv, &sel, &gdr, &gsc, &gse}) s->create();
    b0.assign(cap_, 0.0);
    sweep.assign(cap_, 0);
    hyper.assign((size_t)cap_ * (4 * c->K + 1), 0.0);
    has_hyper = true;  // of every sample kept from here on; a loaded file's have none
    cap = cap_;
    every = every_;
    bytes = (size_t)cap_ * slot_bytes(c);
}
void SampleStore::drop() {
    for (sbmf::DBuf* d : {&d_U, &d_V, &d_bu, &d_bv}) d->release();
    for (sbmf::Span* s : {&cev, &scv, &sel, &gdr, &gsc, &gse}) s->destroy();
    b0.clear();
    sweep.clear();
    hyper.clear();
    has_hyper = false;
    cap = head = count = seen = 0;
    every = 1;
    bytes = 0;
}
// (the caller has checked that the sweep is a collected one)
template <typename T>
void SampleStore::keep(sbmf_ctx* c, const Hyper& hy, hipStream_t se) {
    if (seen++ % every) return;
    const uint32_t p = count < cap ? slot(count) : head;  // the next free slot, or the oldest sample's
    const size_t I = c->I, J = c->J, Kp = c->Kp;
    cev.begin(se);
    HIPCHK(hipMemcpyAsync(d_U.as<T>() + p * I * Kp, c->d_U.p, I * Kp * sizeof(T), hipMemcpyDeviceToDevice, se));
    HIPCHK(hipMemcpyAsync(d_V.as<T>() + p * J * Kp, c->d_V.p, J * Kp * sizeof(T), hipMemcpyDeviceToDevice, se));
    if (c->bias) {
        HIPCHK(hipMemcpyAsync(d_bu.as<double>() + p * I, c->d_bu.p, I * sizeof(double), hipMemcpyDeviceToDevice, se));
        HIPCHK(hipMemcpyAsync(d_bv.as<double>() + p * J, c->d_bv.p, J * sizeof(double), hipMemcpyDeviceToDevice, se));
    }
    cev.end(se);
    b0[p] = hy.b0;
    sweep[p] = c->sweep;
    const size_t K = c->K;
    double* h = hyper.data() + (size_t)p * (4 * K + 1);
    std::copy(hy.sig_u.begin(), hy.sig_u.begin() + K, h);
    std::copy(hy.mu_u.begin(), hy.mu_u.begin() + K, h + K);
    std::copy(hy.sig_v.begin(), hy.sig_v.begin() + K, h + 2 * K);
    std::copy(hy.mu_v.begin(), hy.mu_v.begin() + K, h + 3 * K);
    h[4 * K] = hy.tau;
    if (count < cap) count++;
    else head = (head + 1) % cap;
    c->launches += c->bias ? 4 : 2;
}
template void SampleStore::keep<float>(sbmf_ctx*, const Hyper&, hipStream_t);
template void SampleStore::keep<double>(sbmf_ctx*, const Hyper&, hipStream_t);

extern "C" {

int sbmf_keep_samples(sbmf_ctx* ctx, uint32_t every, uint32_t cap) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    list_scope(ctx, "sample store", "sbmf_keep_samples", false);
    if (every == 0) sbmf::fail(SBMF_E_ARG, "sbmf_keep_samples: every = 0 (1 keeps every collected sweep)");
    if (cap > 65535) sbmf::fail(SBMF_E_ARG, "sbmf_keep_samples: cap %u is above 65535", cap);
    list_sync(ctx);
    ctx->samples.drop();  // (the test hook's settings stay)
    if (cap == 0) return SBMF_OK;
    try {
        ctx->samples.alloc(ctx, cap, every);
    } catch (const sbmf::Error& e) {
        ctx->samples.drop();
        if (e.code == SBMF_E_NOMEM)
            sbmf::fail(SBMF_E_NOMEM, "sbmf_keep_samples: %u samples of %zu bytes need %zu bytes of device memory: %s", cap,
                       slot_bytes(ctx), (size_t)cap * slot_bytes(ctx), e.msg.c_str());
        throw;
    } catch (...) {
        ctx->samples.drop();
        throw;
    }
    API_END(ctx)
}

int sbmf_samples_info(sbmf_ctx* ctx, uint32_t* count, uint32_t* cap, uint32_t* every, uint64_t* bytes) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    list_scope(ctx, "sample store", "sbmf_samples_info", false);
    const SampleStore& ss = ctx->samples;
    if (count) *count = ss.count;
    if (cap) *cap = ss.cap;
    if (every) *every = ss.every;
    if (bytes) *bytes = ss.bytes;
    API_END(ctx)
}

int sbmf_get_sample(sbmf_ctx* ctx, uint32_t s, uint32_t* sweep, double* U, double* V, double* bu, double* bv, double* b0) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    samples_ready(ctx, "sbmf_get_sample");
    const SampleStore& ss = ctx->samples;
    if (s >= ss.count) sbmf::fail(SBMF_E_ARG, "sbmf_get_sample: sample %u of %u kept", s, ss.count);
    const uint32_t p = ss.slot(s);
    const size_t I = ctx->I, J = ctx->J;
    if (sweep) *sweep = ss.sweep[p];
    if (b0) *b0 = ctx->bias ? ss.b0[p] : 0.0;
    // only what was asked for is downloaded (a sample is 148 MB at ML-20M K = 100)
    const size_t K = ctx->K, Kp = ctx->Kp;
    auto table = [&](auto type, const sbmf::DBuf& d, size_t R, double* out) {
        using T = decltype(type);
        std::vector<T> h(R * Kp);
        HIPCHK(hipMemcpy(h.data(), d.as<T>() + (size_t)p * R * Kp, R * Kp * sizeof(T), hipMemcpyDeviceToHost));
        for (size_t r = 0; r < R; ++r)
            for (size_t k = 0; k < K; ++k) out[r * K + k] = (double)h[r * Kp + k];  // an f32 value widens exactly
    };
    const bool f32 = ctx->cfg.precision == SBMF_F32;
    if (U) f32 ? table(float{}, ss.d_U, I, U) : table(double{}, ss.d_U, I, U);
    if (V) f32 ? table(float{}, ss.d_V, J, V) : table(double{}, ss.d_V, J, V);
    auto biases = [&](const sbmf::DBuf& d, size_t R, double* out) {
        if (ctx->bias)
            HIPCHK(hipMemcpy(out, d.as<double>() + (size_t)p * R, R * sizeof(double), hipMemcpyDeviceToHost));
        else
            std::fill(out, out + R, 0.0);
    };
    if (bu) biases(ss.d_bu, I, bu);
    if (bv) biases(ss.d_bv, J, bv);
    API_END(ctx)
}

int sbmf_samples_recommend(sbmf_ctx* ctx, uint32_t n, const uint32_t* users, uint32_t topn, uint32_t flags, double risk,
                           uint32_t* items, double* mean, double* stdev) {
    API_BEGIN
    const char* fn = "sbmf_samples_recommend";
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    list_scope(ctx, "sample store", fn, false);
    if (n && (!users || !items || !mean)) sbmf::fail(SBMF_E_ARG, "%s: null argument", fn);
    if (topn < 1 || topn > 1024) sbmf::fail(SBMF_E_ARG, "%s: topn %u is not in 1..1024", fn, topn);
    if (flags & ~3u)
        sbmf::fail(SBMF_E_ARG, "%s: unknown flags 0x%x (bit 0 = keep rated items, bit 1 = clamp)", fn, flags & ~3u);
    if (!(risk == risk)) sbmf::fail(SBMF_E_ARG, "%s: risk is NaN", fn);
    check_users(ctx, fn, n, users);
    samples_ready(ctx, fn);
    if (n == 0) return SBMF_OK;
    SampleStore& ss = ctx->samples;
    hipStream_t st = ctx->st;
    const uint32_t J = ctx->J, Jp = sbmf::watch_jp(J);
    const bool exclude = !(flags & 1u);
    const int clamp = (flags & 2u) ? 1 : 0;
    // users per slice: as many as the budget's two sums hold, in whole workgroups of 64, one at least
    const uint64_t budget = ss.budget ? ss.budget : kBudget;
    const uint64_t fit = budget / ((uint64_t)2 * Jp * sizeof(double)) / 64 * 64;
    const uint32_t rows = (uint32_t)std::min<uint64_t>(n, std::max<uint64_t>(fit, 64));
    sbmf::DBuf d_b0, d_ids, d_S1, d_S2;
    sbmf::TopnScratch t;
    const sbmf::SampleView v = view_of(ctx, d_b0, st);
    d_ids.alloc((size_t)rows * sizeof(uint32_t));
    d_S1.alloc((size_t)rows * Jp * sizeof(double));
    d_S2.alloc((size_t)rows * Jp * sizeof(double));
    t.alloc(rows, topn, J, exclude);
    for (uint32_t off = 0; off < n; off += rows) {
        const uint32_t m = std::min(rows, n - off);
        const size_t o = (size_t)off * topn;
        HIPCHK(hipMemcpyAsync(d_ids.p, users + off, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        ss.scv.begin(st);
        score_rows(ctx, v, d_ids.as<uint32_t>(), m, clamp, d_S1.as<double>(), d_S2.as<double>(), st);
        ss.scv.end(st);
        sbmf::select_topn(t, d_ids.as<uint32_t>(), m, d_S1.as<double>(), d_S2.as<double>(), J, ss.count,
                          exclude ? ctx->d_uptr.as<uint32_t>() : nullptr, ctx->d_upart.as<uint32_t>(), topn, risk, ss.sel, st,
                          items + o, mean + o, stdev ? stdev + o : nullptr);
    }
    API_END(ctx)
}

int sbmf_samples_scores(sbmf_ctx* ctx, uint32_t user, uint32_t flags, double* mean, double* stdev) {
    API_BEGIN
    const char* fn = "sbmf_samples_scores";
    if (!ctx || !mean) sbmf::fail(SBMF_E_ARG, "null argument");
    list_scope(ctx, "sample store", fn, false);
    if (flags & ~2u) sbmf::fail(SBMF_E_ARG, "%s: unknown flags 0x%x (bit 1 = clamp)", fn, flags & ~2u);
    check_users(ctx, fn, 1, &user);
    samples_ready(ctx, fn);
    SampleStore& ss = ctx->samples;
    hipStream_t st = ctx->st;
    const uint32_t J = ctx->J, Jp = sbmf::watch_jp(J);
    sbmf::DBuf d_b0, d_id, d_S;
    const sbmf::SampleView v = view_of(ctx, d_b0, st);
    d_id.alloc(sizeof(uint32_t));
    d_S.alloc((size_t)2 * Jp * sizeof(double));
    double* S = d_S.as<double>();
    HIPCHK(hipMemcpyAsync(d_id.p, &user, sizeof(uint32_t), hipMemcpyHostToDevice, st));
    ss.scv.begin(st);
    score_rows(ctx, v, d_id.as<uint32_t>(), 1, (flags & 2u) ? 1 : 0, S, S + Jp, st);
    ss.scv.end(st);
    sbmf::row_moments(S, S + Jp, J, ss.count, st, mean, stdev);
    API_END(ctx)
}

int sbmf_samples_predict(sbmf_ctx* ctx, uint64_t n, const uint32_t* users, const uint32_t* items, uint32_t flags,
                         double* mean, double* stdev) {
    API_BEGIN
    const char* fn = "sbmf_samples_predict";
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    list_scope(ctx, "sample store", fn, false);
    if (n && (!users || !items || !mean)) sbmf::fail(SBMF_E_ARG, "%s: null argument", fn);
    if (flags & ~2u) sbmf::fail(SBMF_E_ARG, "%s: unknown flags 0x%x (bit 1 = clamp)", fn, flags & ~2u);
    check_users(ctx, fn, n, users);
    for (uint64_t q = 0; q < n; ++q)
        if (items[q] >= ctx->J)
            sbmf::fail(SBMF_E_ARG, "%s: items[%llu] = %u is not below the %u items", fn, (unsigned long long)q, items[q], ctx->J);
    samples_ready(ctx, fn);
    if (n == 0) return SBMF_OK;
    hipStream_t st = ctx->st;
    const uint64_t chunk = std::min<uint64_t>(n, 1u << 22);  // pairs per launch
    sbmf::DBuf d_b0, d_u, d_i, d_out;
    const sbmf::SampleView v = view_of(ctx, d_b0, st);
    d_u.alloc(chunk * sizeof(uint32_t));
    d_i.alloc(chunk * sizeof(uint32_t));
    d_out.alloc(2 * chunk * sizeof(double));
    const int clamp = (flags & 2u) ? 1 : 0;
    for (uint64_t off = 0; off < n; off += chunk) {
        const uint32_t m = (uint32_t)std::min(chunk, n - off);
        double* d = d_out.as<double>();
        HIPCHK(hipMemcpyAsync(d_u.p, users + off, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_i.p, items + off, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIPCHK(ctx->cfg.precision == SBMF_F32
                   ? sbmf::launch_samples_pairs<float>(v, d_u.as<uint32_t>(), d_i.as<uint32_t>(), m, ctx->Kp, clamp, ctx->lo,
                                                       ctx->hi, d, d + m, st)
                   : sbmf::launch_samples_pairs<double>(v, d_u.as<uint32_t>(), d_i.as<uint32_t>(), m, ctx->Kp, clamp, ctx->lo,
                                                        ctx->hi, d, d + m, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(mean + off, d, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
        if (stdev) HIPCHK(hipMemcpy(stdev + off, d + m, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    }
    API_END(ctx)
}

int sbmf_samples_timing(sbmf_ctx* ctx, double* ms_copy, double* ms_score, double* ms_select) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    list_scope(ctx, "sample store", "sbmf_samples_timing", false);
    SampleStore& ss = ctx->samples;
    if (!ss.cap) sbmf::fail(SBMF_E_STATE, "sbmf_samples_timing: no sample store registered (sbmf_keep_samples)");
    list_sync(ctx);
    if (ms_copy) *ms_copy = ss.cev.ms();
    if (ms_score) *ms_score = ss.scv.ms();
    if (ms_select) *ms_select = ss.sel.ms();
    API_END(ctx)
}

// --- the samples' hyperparameters ---------------------------------------------------------------
int sbmf_get_sample_hyper(sbmf_ctx* ctx, uint32_t s, double* hyper4k, double* tau) {
    API_BEGIN
    const char* fn = "sbmf_get_sample_hyper";
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    samples_ready(ctx, fn);
    const SampleStore& ss = ctx->samples;
    if (s >= ss.count) sbmf::fail(SBMF_E_ARG, "%s: sample %u of %u kept", fn, s, ss.count);
    if (!ss.has_hyper)
        sbmf::fail(SBMF_E_STATE, "%s: the stored samples have no hyperparameters (a sample file holds none: "
                                 "sbmf_load_samples_hyper loads its companion file)", fn);
    const size_t K = ctx->K;
    const double* h = ss.hyper.data() + (size_t)ss.slot(s) * (4 * K + 1);
    if (hyper4k) std::copy(h, h + 4 * K, hyper4k);
    if (tau) *tau = h[4 * K];
    API_END(ctx)
}

// --- guests from the stored samples -----------------------------------------------------------
int sbmf_samples_foldin_recommend(sbmf_ctx* ctx, uint32_t n, const uint32_t* ptr, const uint32_t* items,
                                  const double* ratings, uint32_t scans, uint32_t topn, uint32_t flags, double risk,
                                  uint32_t* out_items, double* mean, double* stdev) {
    API_BEGIN
    const char* fn = "sbmf_samples_foldin_recommend";
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    list_scope(ctx, "sample store", fn, false);
    if (n && (!out_items || !mean)) sbmf::fail(SBMF_E_ARG, "%s: null argument", fn);
    if (topn < 1 || topn > 1024) sbmf::fail(SBMF_E_ARG, "%s: topn %u is not in 1..1024", fn, topn);
    if (flags & ~3u)
        sbmf::fail(SBMF_E_ARG, "%s: unknown flags 0x%x (bit 0 = keep the guest's own items, bit 1 = clamp)", fn, flags & ~3u);
    if (!(risk == risk)) sbmf::fail(SBMF_E_ARG, "%s: risk is NaN", fn);
    guests_ready(ctx, fn, n, ptr, items, ratings, scans);
    if (n == 0) return SBMF_OK;
    SampleStore& ss = ctx->samples;
    hipStream_t st = ctx->st;
    const uint32_t J = ctx->J;
    const bool exclude = !(flags & 1u);
    GuestCall gc(ctx, fn, n, ptr, items, ratings, scans, true);
    const uint32_t rows = gc.rows;
    sbmf::TopnScratch t;
    try {
        t.alloc(rows, topn, J, exclude);
    } catch (const sbmf::Error& e) {
        if (e.code == SBMF_E_NOMEM)
            sbmf::fail(SBMF_E_NOMEM, "%s: the selection of %u guests needs %zu bytes of device memory: %s", fn, rows,
                       (size_t)rows * topn * (sizeof(uint32_t) + 2 * sizeof(double)) +
                           (exclude ? (size_t)rows * sbmf::watch_jw(J) * sizeof(uint32_t) : 0),
                       e.msg.c_str());
        throw;
    }
    for (uint32_t off = 0; off < n; off += rows) {
        const uint32_t m = std::min(rows, n - off);
        const size_t o = (size_t)off * topn;
        gc.draw(off, m);
        gc.score(m, (flags & 2u) ? 1 : 0);
        // "rated": the guest's own items (the guest CSR in the user-side CSR's place)
        sbmf::select_topn(t, gc.csr.d_ids.as<uint32_t>() + off, m, gc.d_S1.as<double>(), gc.d_S2.as<double>(), J, ss.count,
                          exclude ? gc.csr.d_ptr.as<uint32_t>() : nullptr, gc.csr.d_items.as<uint32_t>(), topn, risk, ss.gse, st,
                          out_items + o, mean + o, stdev ? stdev + o : nullptr);
    }
    API_END(ctx)
}

int sbmf_samples_foldin_rows(sbmf_ctx* ctx, uint32_t n, const uint32_t* ptr, const uint32_t* items, const double* ratings,
                             uint32_t scans, double* rows) {
    API_BEGIN
    const char* fn = "sbmf_samples_foldin_rows";
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    list_scope(ctx, "sample store", fn, false);
    if (n && !rows) sbmf::fail(SBMF_E_ARG, "%s: null argument", fn);
    guests_ready(ctx, fn, n, ptr, items, ratings, scans);
    if (n == 0) return SBMF_OK;
    const SampleStore& ss = ctx->samples;
    const size_t K = ctx->K, Kp = ctx->Kp;
    GuestCall gc(ctx, fn, n, ptr, items, ratings, scans, false);
    auto fetch = [&](auto type, uint32_t off, uint32_t m) {
        using T = decltype(type);
        std::vector<T> h((size_t)m * Kp);
        for (uint32_t s = 0; s < ss.count; ++s) {
            HIPCHK(hipMemcpy(h.data(), gc.d_GS.as<T>() + (size_t)ss.slot(s) * gc.gs, h.size() * sizeof(T), hipMemcpyDeviceToHost));
            double* out = rows + ((size_t)s * n + off) * K;
            for (size_t g = 0; g < m; ++g)
                for (size_t k = 0; k < K; ++k) out[g * K + k] = (double)h[g * Kp + k];  // an f32 value widens exactly
        }
    };
    for (uint32_t off = 0; off < n; off += gc.rows) {
        const uint32_t m = std::min(gc.rows, n - off);
        gc.draw(off, m);
        HIPCHK(hipStreamSynchronize(ctx->st));
        ctx->cfg.precision == SBMF_F32 ? fetch(float{}, off, m) : fetch(double{}, off, m);
    }
    API_END(ctx)
}

int sbmf_samples_foldin_scores(sbmf_ctx* ctx, uint32_t len, const uint32_t* items, const double* ratings, uint32_t scans,
                               uint32_t flags, double* mean, double* stdev) {
    API_BEGIN
    const char* fn = "sbmf_samples_foldin_scores";
    if (!ctx || !mean) sbmf::fail(SBMF_E_ARG, "null argument");
    list_scope(ctx, "sample store", fn, false);
    if (flags & ~2u) sbmf::fail(SBMF_E_ARG, "%s: unknown flags 0x%x (bit 1 = clamp)", fn, flags & ~2u);
    const uint32_t ptr[2] = {0, len};
    guests_ready(ctx, fn, 1, ptr, items, ratings, scans);
    const SampleStore& ss = ctx->samples;
    GuestCall gc(ctx, fn, 1, ptr, items, ratings, scans, true);
    gc.draw(0, 1);
    gc.score(1, (flags & 2u) ? 1 : 0);
    sbmf::row_moments(gc.d_S1.as<double>(), gc.d_S2.as<double>(), ctx->J, ss.count, ctx->st, mean, stdev);
    API_END(ctx)
}

int sbmf_samples_foldin_timing(sbmf_ctx* ctx, double* ms_draw, double* ms_score, double* ms_select) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    list_scope(ctx, "sample store", "sbmf_samples_foldin_timing", false);
    SampleStore& ss = ctx->samples;
    if (!ss.cap) sbmf::fail(SBMF_E_STATE, "sbmf_samples_foldin_timing: no sample store registered (sbmf_keep_samples)");
    list_sync(ctx);
    if (ms_draw) *ms_draw = ss.gdr.ms();
    if (ms_score) *ms_score = ss.gsc.ms();
    if (ms_select) *ms_select = ss.gse.ms();
    API_END(ctx)
}

int sbmf_test_samples_tune(sbmf_ctx* ctx, uint64_t budget_bytes, int unfused) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    ctx->samples.budget = budget_bytes;
    ctx->samples.unfused = (unfused & 1) != 0;
    ctx->samples.fused_draw = (unfused & 2) != 0;
    API_END(ctx)
}

int sbmf_test_samples_lds(uint32_t Kp, uint32_t* rows, uint64_t* bytes) {
    sbmf_ctx* ctx = nullptr;
    API_BEGIN
    if (!rows || !bytes) sbmf::fail(SBMF_E_ARG, "null argument");
    const int mu = sbmf::watch_mu(Kp);
    *rows = 16u * (uint32_t)mu;
    *bytes = sbmf::samples_lds_bytes(mu, Kp);
    API_END(ctx)
}

}  // extern "C"
