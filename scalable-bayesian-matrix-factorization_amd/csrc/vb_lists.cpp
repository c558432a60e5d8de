// vb_lists.cpp -- the online VB learner's lists (include/sbmf.h, sbmf_vb_*): the posterior read
// back, closed-form score moments and top-N for training users and for guests, pair predictions
// and the posterior file.  Stateless: every call answers from the learner's current tables
// (vbo_view) and frees its temporaries; the context keeps the user-side CSR of the train set (the
// rated-item masks) and the last launches' event pairs (VBLists, ctx.h).
#include "ctx.h"

namespace {

using namespace sbmf;

constexpr uint64_t kVbBudget = 1ull << 30;
constexpr char kMagic[8] = {'S', 'B', 'M', 'F', 'V', 'B', 'P', '1'};
constexpr uint32_t kVersion = 1;

void vb_scope(const sbmf_ctx* c, const char* fn) {
    if (c->cfg.method != SBMF_METHOD_VB)
        fail(SBMF_E_STATE, "%s: the closed-form posterior lists are offered by the online VB learner (SBMF_METHOD_VB) "
                           "only; this context runs the %s", fn,
             c->cfg.method == SBMF_METHOD_MCMC ? "SBPMF sampler" : c->cfg.method == SBMF_METHOD_ALS ? "ALS learner"
                                                                                                     : "libFM MCMC learner");
    if (c->virt) fail(SBMF_E_STATE, "%s: a virtual rank's numbers are not a model; no online VB list there", fn);
    if (c->nranks > 1 || c->comm->active() || c->comm != &c->own_comm)
        fail(SBMF_E_STATE, "%s: the online VB lists run on one rank; this context joined a communicator", fn);
    if (!c->prepared || !c->vb) fail(SBMF_E_STATE, "%s: not prepared (sbmf_prepare)", fn);
}
void check_users(const sbmf_ctx* c, const char* fn, uint64_t n, const uint32_t* users) {
    for (uint64_t w = 0; w < n; ++w)
        if (users[w] >= c->I)
            fail(SBMF_E_ARG, "%s: users[%llu] = %u is not below the %u users", fn, (unsigned long long)w, users[w], c->I);
}
void check_topn(const char* fn, uint32_t topn, uint32_t flags, double risk) {
    if (topn < 1 || topn > 1024) fail(SBMF_E_ARG, "%s: topn %u is not in 1..1024", fn, topn);
    if (flags & ~1u)
        fail(SBMF_E_ARG, "%s: unknown flags 0x%x (bit 0 = keep rated items; the closed-form moments have no clamp)", fn,
             flags & ~1u);
    if (!(risk == risk)) fail(SBMF_E_ARG, "%s: risk is NaN", fn);
}
void check_scans(const char* fn, uint32_t scans) {
    if (scans < 1 || scans > 64) fail(SBMF_E_ARG, "%s: scans %u is not in 1..64", fn, scans);
}

// One call's view of the learner: in scope, the transposes current, the operands of the kernels.
struct Call {
    sbmf_ctx* c;
    VBLists& l;
    VBView v;
    VBItems it;
    hipStream_t st;
    uint32_t J, Jp, K, Kp;
    Call(sbmf_ctx* ctx, const char* fn) : c(ctx), l(ctx->vbl) {
        vb_scope(c, fn);
        HIPCHK(hipSetDevice(c->cfg.device));
        v = vbo_view(c->vb);
        st = v.st;
        J = v.J, Jp = watch_jp(J), K = v.K, Kp = v.Kp;
        if (!l.spans) {
            for (Span* s : {&l.tr, &l.sc, &l.sel, &l.gu}) s->create();
            l.spans = true;
        }
        if (!vbo_transposes_fresh(c->vb)) {
            l.tr.begin(st);
            vbo_fresh_transposes(c->vb);
            l.tr.end(st);
        }
        it = VBItems{v.muT + (size_t)v.I * Kp, v.sgT + (size_t)v.I * Kp, v.tb.mu_w + v.I, v.tb.sg_w + v.I, v.tb.scal, J, Kp};
    }
    VBRows users(const uint32_t* d_ids) const { return VBRows{d_ids, v.muT, v.sgT, v.tb.mu_w, v.tb.sg_w}; }
    // rows per slice: as many as the budget's two moment rows hold, in whole workgroups of 64, one at least
    uint32_t slice(uint32_t n) const {
        const uint64_t budget = l.budget ? l.budget : kVbBudget;
        const uint64_t fit = budget / ((uint64_t)2 * Jp * sizeof(double)) / 64 * 64;
        return (uint32_t)std::min<uint64_t>(n, std::max<uint64_t>(fit, 64));
    }
    void score(const VBRows& rows, uint32_t m, double* M, double* Vr) {
        l.sc.begin(st);
        HIPCHK(launch_vb_score(rows, m, it, M, Vr, st));
        l.sc.end(st);
    }
    // the user-side CSR of the train set, from the context's triples (items in file order)
    void user_csr() {
        if (l.csr) return;
        std::vector<uint32_t> ptr(c->I + 1, 0), part(c->tu.size());
        for (uint32_t u : c->tu) ptr[u + 1]++;
        for (uint32_t u = 0; u < c->I; ++u) ptr[u + 1] += ptr[u];
        std::vector<uint32_t> at(ptr.begin(), ptr.end() - 1);
        for (size_t x = 0; x < c->tu.size(); ++x) part[at[c->tu[x]]++] = c->ti[x];
        try {
            upload(l.d_uptr, ptr, st);
            upload(l.d_upart, part, st);
            HIPCHK(hipStreamSynchronize(st));  // the vectors are locals
        } catch (...) {
            l.d_uptr.release();
            l.d_upart.release();
            throw;
        }
        l.csr = true;
    }
    // one row's mean and (sd: its square root; else itself) variance to the host
    void row_out(const VBRows& rows, double* mean, double* second, bool sd) {
        DBuf d_S;
        d_S.alloc((size_t)3 * Jp * sizeof(double));
        double* S = d_S.as<double>();
        score(rows, 1, S, S + Jp);
        if (sd && second) HIPCHK(launch_vb_sd(S + Jp, J, S + 2 * Jp, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(mean, S, (size_t)J * sizeof(double), hipMemcpyDeviceToHost));
        if (second) HIPCHK(hipMemcpy(second, S + (sd ? 2 : 1) * Jp, (size_t)J * sizeof(double), hipMemcpyDeviceToHost));
    }
};

// The guests of one call: their CSR on the device and their posterior rows GM, GS [n][Kp], gb, gs [n].
struct Guests {
    GuestCSR csr;
    DBuf d_GM, d_GS, d_gb, d_gs;
    void run(Call& k, const char* fn, uint32_t n, const uint32_t* ptr, const uint32_t* items, const double* ratings,
             uint32_t scans) {
        if (k.Kp > VB_GUEST_KP_MAX) fail(SBMF_E_ARG, "%s: K = %u is above the guests' limit of %u factors", fn, k.K, VB_GUEST_KP_MAX);
        csr.upload(n, ptr, items, ratings, n, k.st);  // one slice: every guest in one launch, the longest first
        d_GM.alloc((size_t)n * k.Kp * sizeof(double));
        d_GS.alloc((size_t)n * k.Kp * sizeof(double));
        d_gb.alloc((size_t)n * sizeof(double));
        d_gs.alloc((size_t)n * sizeof(double));
        k.l.gu.begin(k.st);
        HIPCHK(launch_vb_guest(csr.d_ptr.as<uint32_t>(), csr.d_items.as<uint32_t>(), csr.d_ratings.as<double>(),
                               csr.d_order.as<uint32_t>(), csr.d_E.as<double>(), n, scans, k.it, k.v.tb.sigma_v, k.K,
                               d_GM.as<double>(), d_GS.as<double>(), d_gb.as<double>(), d_gs.as<double>(), k.st));
        k.l.gu.end(k.st);
    }
    VBRows rows(const Call& k, uint32_t off) const {
        return VBRows{nullptr, d_GM.as<double>() + (size_t)off * k.Kp, d_GS.as<double>() + (size_t)off * k.Kp,
                      d_gb.as<double>() + off, d_gs.as<double>() + off};
    }
};

// the tables on the host, attribute-major and without padding
struct HostPosterior {
    uint32_t I = 0, J = 0, K = 0;
    std::vector<double> Um, Us, Vm, Vs, bum, bus, bvm, bvs, sigma_v;
    double mu0 = 0, sg0 = 0, alpha = 0, sigma_0 = 0, sigma_w = 0;
    uint64_t bytes() const { return 24 + 8ull * (5 + K) + 16ull * (K + 1) * ((uint64_t)I + J); }
};
void split_fmajor(const std::vector<double>& h, uint32_t K, uint32_t I, uint32_t J, std::vector<double>& U, std::vector<double>& V) {
    const size_t p = (size_t)I + J;
    U.resize((size_t)I * K);
    V.resize((size_t)J * K);
    for (uint32_t f = 0; f < K; ++f) {
        for (uint32_t a = 0; a < I; ++a) U[(size_t)a * K + f] = h[f * p + a];
        for (uint32_t a = 0; a < J; ++a) V[(size_t)a * K + f] = h[f * p + I + a];
    }
}
void download(sbmf_ctx* c, HostPosterior& P) {
    const VBView v = vbo_view(c->vb);
    HIPCHK(hipStreamSynchronize(v.st));
    P.I = v.I, P.J = v.J, P.K = v.K;
    const size_t p = (size_t)v.I + v.J;
    std::vector<double> h((size_t)v.K * p), w(p);
    HIPCHK(hipMemcpy(h.data(), v.tb.mu_v, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    split_fmajor(h, v.K, v.I, v.J, P.Um, P.Vm);
    HIPCHK(hipMemcpy(h.data(), v.tb.sg_v, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    split_fmajor(h, v.K, v.I, v.J, P.Us, P.Vs);
    HIPCHK(hipMemcpy(w.data(), v.tb.mu_w, p * sizeof(double), hipMemcpyDeviceToHost));
    P.bum.assign(w.begin(), w.begin() + v.I);
    P.bvm.assign(w.begin() + v.I, w.end());
    HIPCHK(hipMemcpy(w.data(), v.tb.sg_w, p * sizeof(double), hipMemcpyDeviceToHost));
    P.bus.assign(w.begin(), w.begin() + v.I);
    P.bvs.assign(w.begin() + v.I, w.end());
    P.sigma_v.resize(v.K);
    HIPCHK(hipMemcpy(P.sigma_v.data(), v.tb.sigma_v, v.K * sizeof(double), hipMemcpyDeviceToHost));
    VBScal sc;
    HIPCHK(hipMemcpy(&sc, v.tb.scal, sizeof sc, hipMemcpyDeviceToHost));
    P.mu0 = sc.mu0, P.sg0 = sc.sg0, P.alpha = sc.alpha, P.sigma_0 = sc.sigma_0, P.sigma_w = sc.sigma_w;
}
void join_fmajor(const std::vector<double>& U, const std::vector<double>& V, uint32_t K, uint32_t I, uint32_t J, std::vector<double>& h) {
    const size_t p = (size_t)I + J;
    h.resize((size_t)K * p);
    for (uint32_t f = 0; f < K; ++f) {
        for (uint32_t a = 0; a < I; ++a) h[f * p + a] = U[(size_t)a * K + f];
        for (uint32_t a = 0; a < J; ++a) h[f * p + I + a] = V[(size_t)a * K + f];
    }
}

struct File {
    FILE* f = nullptr;
    ~File() {
        if (f) std::fclose(f);
    }
};
// the header of `path`, validated against the file's length
void read_header(const char* fn, const char* path, File& F, HostPosterior& P, uint32_t& version) {
    if (!path) fail(SBMF_E_ARG, "%s: null path", fn);
    F.f = std::fopen(path, "rb");
    if (!F.f) fail(SBMF_E_IO, "%s: cannot open %s", fn, path);
    char magic[8];
    uint32_t h[4];
    if (std::fread(magic, 1, 8, F.f) != 8 || std::fread(h, 4, 4, F.f) != 4)
        fail(SBMF_E_IO, "%s: %s is truncated in its header", fn, path);
    if (std::memcmp(magic, kMagic, 8) != 0) fail(SBMF_E_IO, "%s: %s is not a VB posterior file (bad magic)", fn, path);
    version = h[0];
    if (version != kVersion) fail(SBMF_E_IO, "%s: %s has version %u (this library reads %u)", fn, path, version, kVersion);
    P.I = h[1], P.J = h[2], P.K = h[3];
    if (P.K == 0 || P.K > 256) fail(SBMF_E_IO, "%s: %s has a bad field (num_factor %u)", fn, path, P.K);
    if (std::fseek(F.f, 0, SEEK_END) != 0) fail(SBMF_E_IO, "%s: cannot seek in %s", fn, path);
    const long long len = std::ftell(F.f);
    if (len < 0 || (uint64_t)len < P.bytes())
        fail(SBMF_E_IO, "%s: %s is truncated in its body (%lld bytes; its header implies %llu)", fn, path, len,
             (unsigned long long)P.bytes());
    if ((uint64_t)len > P.bytes())
        fail(SBMF_E_IO, "%s: %s has trailing bytes (%lld bytes; its header implies %llu)", fn, path, len,
             (unsigned long long)P.bytes());
    std::fseek(F.f, 24, SEEK_SET);
}

}  // namespace

extern "C" {

int sbmf_vb_get_posterior(sbmf_ctx* ctx, double* U_mean, double* U_var, double* V_mean, double* V_var, double* bu_mean,
                          double* bu_var, double* bv_mean, double* bv_var, double* b0, double* hyper) {
    API_BEGIN
    const char* fn = "sbmf_vb_get_posterior";
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    vb_scope(ctx, fn);
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HostPosterior P;
    download(ctx, P);
    auto out = [](double* dst, const std::vector<double>& v) {
        if (dst) std::copy(v.begin(), v.end(), dst);
    };
    out(U_mean, P.Um), out(U_var, P.Us), out(V_mean, P.Vm), out(V_var, P.Vs);
    out(bu_mean, P.bum), out(bu_var, P.bus), out(bv_mean, P.bvm), out(bv_var, P.bvs);
    if (b0) b0[0] = P.mu0, b0[1] = P.sg0;
    if (hyper) {
        hyper[0] = P.alpha, hyper[1] = P.sigma_0, hyper[2] = P.sigma_w;
        std::copy(P.sigma_v.begin(), P.sigma_v.end(), hyper + 3);
    }
    API_END(ctx)
}

static int vb_user_row(sbmf_ctx* ctx, const char* fn, uint32_t user, double* mean, double* second, bool sd) {
    API_BEGIN
    if (!ctx || !mean) sbmf::fail(SBMF_E_ARG, "null argument");
    Call k(ctx, fn);
    check_users(ctx, fn, 1, &user);
    sbmf::DBuf d_id;
    d_id.alloc(sizeof(uint32_t));
    HIPCHK(hipMemcpyAsync(d_id.p, &user, sizeof(uint32_t), hipMemcpyHostToDevice, k.st));
    k.row_out(k.users(d_id.as<uint32_t>()), mean, second, sd);
    API_END(ctx)
}
int sbmf_vb_scores(sbmf_ctx* ctx, uint32_t user, double* mean, double* stdev) {
    return vb_user_row(ctx, "sbmf_vb_scores", user, mean, stdev, true);
}
int sbmf_test_vb_moments(sbmf_ctx* ctx, uint32_t user, double* mean, double* var) {
    return vb_user_row(ctx, "sbmf_test_vb_moments", user, mean, var, false);
}

int sbmf_vb_recommend(sbmf_ctx* ctx, uint32_t n, const uint32_t* users, uint32_t topn, uint32_t flags, double risk,
                      uint32_t* items, double* mean, double* stdev) {
    API_BEGIN
    const char* fn = "sbmf_vb_recommend";
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    Call k(ctx, fn);
    if (n && (!users || !items || !mean)) sbmf::fail(SBMF_E_ARG, "%s: null argument", fn);
    check_topn(fn, topn, flags, risk);
    check_users(ctx, fn, n, users);
    if (n == 0) return SBMF_OK;
    const bool exclude = !(flags & 1u);
    if (exclude) k.user_csr();
    const uint32_t rows = k.slice(n);
    sbmf::DBuf d_ids, d_M, d_V;
    sbmf::TopnScratch t;
    d_ids.alloc((size_t)rows * sizeof(uint32_t));
    d_M.alloc((size_t)rows * k.Jp * sizeof(double));
    d_V.alloc((size_t)rows * k.Jp * sizeof(double));
    t.alloc(rows, topn, k.J, exclude);
    for (uint32_t off = 0; off < n; off += rows) {
        const uint32_t m = std::min(rows, n - off);
        const size_t o = (size_t)off * topn;
        HIPCHK(hipMemcpyAsync(d_ids.p, users + off, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, k.st));
        k.score(k.users(d_ids.as<uint32_t>()), m, d_M.as<double>(), d_V.as<double>());
        sbmf::select_topn(t, d_ids.as<uint32_t>(), m, d_M.as<double>(), d_V.as<double>(), k.J, 1,
                          exclude ? k.l.d_uptr.as<uint32_t>() : nullptr, k.l.d_upart.as<uint32_t>(), topn, risk, k.l.sel, k.st,
                          items + o, mean + o, stdev ? stdev + o : nullptr, true);
    }
    API_END(ctx)
}

int sbmf_vb_predict(sbmf_ctx* ctx, uint64_t n, const uint32_t* users, const uint32_t* items, double* mean, double* stdev) {
    API_BEGIN
    const char* fn = "sbmf_vb_predict";
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    Call k(ctx, fn);
    if (n && (!users || !items || !mean)) sbmf::fail(SBMF_E_ARG, "%s: null argument", fn);
    check_users(ctx, fn, n, users);
    for (uint64_t q = 0; q < n; ++q)
        if (items[q] >= ctx->J)
            sbmf::fail(SBMF_E_ARG, "%s: items[%llu] = %u is not below the %u items", fn, (unsigned long long)q, items[q], ctx->J);
    if (n == 0) return SBMF_OK;
    sbmf::DBuf d_u, d_i, d_o;
    d_u.alloc(n * sizeof(uint32_t));
    d_i.alloc(n * sizeof(uint32_t));
    d_o.alloc(2 * n * sizeof(double));
    double* o = d_o.as<double>();
    HIPCHK(hipMemcpyAsync(d_u.p, users, n * sizeof(uint32_t), hipMemcpyHostToDevice, k.st));
    HIPCHK(hipMemcpyAsync(d_i.p, items, n * sizeof(uint32_t), hipMemcpyHostToDevice, k.st));
    HIPCHK(launch_vb_pairs(d_u.as<uint32_t>(), d_i.as<uint32_t>(), n, k.v.muT, k.v.sgT, k.v.tb, k.Kp, o, o + n, nullptr, k.st));
    HIPCHK(hipStreamSynchronize(k.st));
    HIPCHK(hipMemcpy(mean, o, n * sizeof(double), hipMemcpyDeviceToHost));
    if (stdev) HIPCHK(hipMemcpy(stdev, o + n, n * sizeof(double), hipMemcpyDeviceToHost));
    API_END(ctx)
}

int sbmf_vb_foldin_rows(sbmf_ctx* ctx, uint32_t n, const uint32_t* ptr, const uint32_t* items, const double* ratings,
                        uint32_t scans, double* row_mean, double* row_var, double* b_mean, double* b_var) {
    API_BEGIN
    const char* fn = "sbmf_vb_foldin_rows";
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    Call k(ctx, fn);
    check_scans(fn, scans);
    sbmf::GuestCSR::check(fn, n, ptr, items, ratings, ctx->J);
    if (n == 0) return SBMF_OK;
    Guests g;
    g.run(k, fn, n, ptr, items, ratings, scans);
    HIPCHK(hipStreamSynchronize(k.st));
    std::vector<double> h((size_t)n * k.Kp);
    for (int which = 0; which < 2; ++which) {
        double* dst = which ? row_var : row_mean;
        if (!dst) continue;
        HIPCHK(hipMemcpy(h.data(), (which ? g.d_GS : g.d_GM).p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (uint32_t r = 0; r < n; ++r) std::copy_n(h.begin() + (size_t)r * k.Kp, k.K, dst + (size_t)r * k.K);
    }
    if (b_mean) HIPCHK(hipMemcpy(b_mean, g.d_gb.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    if (b_var) HIPCHK(hipMemcpy(b_var, g.d_gs.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    API_END(ctx)
}

int sbmf_vb_foldin_scores(sbmf_ctx* ctx, uint32_t len, const uint32_t* items, const double* ratings, uint32_t scans,
                          double* mean, double* stdev) {
    API_BEGIN
    const char* fn = "sbmf_vb_foldin_scores";
    if (!ctx || !mean) sbmf::fail(SBMF_E_ARG, "null argument");
    Call k(ctx, fn);
    check_scans(fn, scans);
    const uint32_t ptr[2] = {0, len};
    sbmf::GuestCSR::check(fn, 1, ptr, items, ratings, ctx->J);
    Guests g;
    g.run(k, fn, 1, ptr, items, ratings, scans);
    k.row_out(g.rows(k, 0), mean, stdev, true);
    API_END(ctx)
}

int sbmf_vb_foldin_recommend(sbmf_ctx* ctx, uint32_t n, const uint32_t* ptr, const uint32_t* items, const double* ratings,
                             uint32_t scans, uint32_t topn, uint32_t flags, double risk, uint32_t* out_items, double* mean,
                             double* stdev) {
    API_BEGIN
    const char* fn = "sbmf_vb_foldin_recommend";
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    Call k(ctx, fn);
    if (n && (!out_items || !mean)) sbmf::fail(SBMF_E_ARG, "%s: null argument", fn);
    check_scans(fn, scans);
    check_topn(fn, topn, flags, risk);
    sbmf::GuestCSR::check(fn, n, ptr, items, ratings, ctx->J);
    if (n == 0) return SBMF_OK;
    const bool exclude = !(flags & 1u);
    Guests g;
    g.run(k, fn, n, ptr, items, ratings, scans);
    const uint32_t rows = k.slice(n);
    sbmf::DBuf d_M, d_V;
    sbmf::TopnScratch t;
    d_M.alloc((size_t)rows * k.Jp * sizeof(double));
    d_V.alloc((size_t)rows * k.Jp * sizeof(double));
    t.alloc(rows, topn, k.J, exclude);
    for (uint32_t off = 0; off < n; off += rows) {
        const uint32_t m = std::min(rows, n - off);
        const size_t o = (size_t)off * topn;
        k.score(g.rows(k, off), m, d_M.as<double>(), d_V.as<double>());
        // "rated": the guest's own items (the guest CSR in the user-side CSR's place; the rows' ids off ..)
        sbmf::select_topn(t, g.csr.d_ids.as<uint32_t>() + off, m, d_M.as<double>(), d_V.as<double>(), k.J, 1,
                          exclude ? g.csr.d_ptr.as<uint32_t>() : nullptr, g.csr.d_items.as<uint32_t>(), topn, risk, k.l.sel,
                          k.st, out_items + o, mean + o, stdev ? stdev + o : nullptr, true);
    }
    API_END(ctx)
}

int sbmf_vb_save_posterior(sbmf_ctx* ctx, const char* path) {
    API_BEGIN
    const char* fn = "sbmf_vb_save_posterior";
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (!path) sbmf::fail(SBMF_E_ARG, "%s: null path", fn);
    vb_scope(ctx, fn);
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HostPosterior P;
    download(ctx, P);
    File F;
    F.f = std::fopen(path, "wb");
    if (!F.f) sbmf::fail(SBMF_E_IO, "%s: cannot open %s for writing", fn, path);
    const uint32_t h[4] = {kVersion, P.I, P.J, P.K};
    const double sc[5] = {P.mu0, P.sg0, P.alpha, P.sigma_0, P.sigma_w};
    bool ok = std::fwrite(kMagic, 1, 8, F.f) == 8 && std::fwrite(h, 4, 4, F.f) == 4 && std::fwrite(sc, 8, 5, F.f) == 5;
    for (const std::vector<double>* v : {&P.sigma_v, &P.Um, &P.Us, &P.Vm, &P.Vs, &P.bum, &P.bus, &P.bvm, &P.bvs})
        ok = ok && std::fwrite(v->data(), 8, v->size(), F.f) == v->size();
    ok = ok && std::fflush(F.f) == 0;
    if (!ok) sbmf::fail(SBMF_E_IO, "%s: writing %s failed", fn, path);
    API_END(ctx)
}

int sbmf_vb_load_posterior(sbmf_ctx* ctx, const char* path) {
    API_BEGIN
    const char* fn = "sbmf_vb_load_posterior";
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    vb_scope(ctx, fn);
    HIPCHK(hipSetDevice(ctx->cfg.device));
    File F;
    HostPosterior P;
    uint32_t version = 0;
    read_header(fn, path, F, P, version);
    const VBView v = vbo_view(ctx->vb);
    if (P.I != v.I || P.J != v.J || P.K != v.K)
        sbmf::fail(SBMF_E_ARG, "%s: %s holds %u users, %u items and %u factors; this context has %u, %u and %u", fn, path, P.I,
                   P.J, P.K, v.I, v.J, v.K);
    double sc[5];
    P.sigma_v.resize(P.K);
    P.Um.resize((size_t)P.I * P.K), P.Us.resize((size_t)P.I * P.K), P.Vm.resize((size_t)P.J * P.K), P.Vs.resize((size_t)P.J * P.K);
    P.bum.resize(P.I), P.bus.resize(P.I), P.bvm.resize(P.J), P.bvs.resize(P.J);
    bool ok = std::fread(sc, 8, 5, F.f) == 5;
    for (std::vector<double>* a : {&P.sigma_v, &P.Um, &P.Us, &P.Vm, &P.Vs, &P.bum, &P.bus, &P.bvm, &P.bvs})
        ok = ok && std::fread(a->data(), 8, a->size(), F.f) == a->size();
    if (!ok) sbmf::fail(SBMF_E_IO, "%s: %s is truncated in its body", fn, path);
    // everything is read: only now does the context change
    HIPCHK(hipStreamSynchronize(v.st));
    std::vector<double> h, w((size_t)P.I + P.J);
    join_fmajor(P.Um, P.Vm, P.K, P.I, P.J, h);
    HIPCHK(hipMemcpy(v.tb.mu_v, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    join_fmajor(P.Us, P.Vs, P.K, P.I, P.J, h);
    HIPCHK(hipMemcpy(v.tb.sg_v, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    std::copy(P.bum.begin(), P.bum.end(), w.begin());
    std::copy(P.bvm.begin(), P.bvm.end(), w.begin() + P.I);
    HIPCHK(hipMemcpy(v.tb.mu_w, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
    std::copy(P.bus.begin(), P.bus.end(), w.begin());
    std::copy(P.bvs.begin(), P.bvs.end(), w.begin() + P.I);
    HIPCHK(hipMemcpy(v.tb.sg_w, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(v.tb.sigma_v, P.sigma_v.data(), P.K * sizeof(double), hipMemcpyHostToDevice));
    VBScal s;
    HIPCHK(hipMemcpy(&s, v.tb.scal, sizeof s, hipMemcpyDeviceToHost));
    s.mu0 = sc[0], s.sg0 = sc[1], s.alpha = sc[2], s.sigma_0 = sc[3], s.sigma_w = sc[4];
    HIPCHK(hipMemcpy(v.tb.scal, &s, sizeof s, hipMemcpyHostToDevice));
    vbo_set_loaded(ctx->vb);
    API_END(ctx)
}

int sbmf_vb_posterior_file_info(const char* path, uint32_t* version, uint32_t* num_users, uint32_t* num_items,
                                uint32_t* num_factor, uint64_t* bytes) {
    sbmf_ctx* ctx = nullptr;
    API_BEGIN
    File F;
    HostPosterior P;
    uint32_t ver = 0;
    read_header("sbmf_vb_posterior_file_info", path, F, P, ver);
    if (version) *version = ver;
    if (num_users) *num_users = P.I;
    if (num_items) *num_items = P.J;
    if (num_factor) *num_factor = P.K;
    if (bytes) *bytes = P.bytes();
    API_END(ctx)
}

int sbmf_vb_timing(sbmf_ctx* ctx, double* ms_transpose, double* ms_score, double* ms_select, double* ms_guest) {
    API_BEGIN
    const char* fn = "sbmf_vb_timing";
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    vb_scope(ctx, fn);
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(vbo_view(ctx->vb).st));
    const VBLists& l = ctx->vbl;
    if (ms_transpose) *ms_transpose = l.tr.ms();
    if (ms_score) *ms_score = l.sc.ms();
    if (ms_select) *ms_select = l.sel.ms();
    if (ms_guest) *ms_guest = l.gu.ms();
    API_END(ctx)
}

int sbmf_test_vb_tune(sbmf_ctx* ctx, uint64_t budget_bytes) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    ctx->vbl.budget = budget_bytes;
    API_END(ctx)
}

int sbmf_test_vb_score_lds(uint32_t Kp, uint32_t* rows, uint64_t* bytes) {
    sbmf_ctx* ctx = nullptr;
    API_BEGIN
    if (!rows || !bytes) sbmf::fail(SBMF_E_ARG, "null argument");
    const int mu = sbmf::vb_score_mu(Kp);
    *rows = 16u * (uint32_t)mu;
    *bytes = sbmf::vb_score_lds_bytes(mu, Kp);
    API_END(ctx)
}

}  // extern "C"
