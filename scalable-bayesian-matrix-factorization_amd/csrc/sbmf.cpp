// sbmf.cpp -- host side of the MI355X SBPMF sampler: the C ABI of include/sbmf.h.
//
// Per sweep (reference loop body gibbs_sbpmf_final.cpp:309-564):
//   1. residual sum of squares + column statistics of U and V (device,
//      fixed-order reductions)            -> one small D2H
//   2. tau, sigma_u/mu_u, sigma_v/mu_v drawn on the host in fp64 with the
//      reference's expressions (:339-342, :375-414)  -> H2D hyper buffer
//   3. user half-sweep (kernels.hip), [RCCL: broadcast U row blocks]
//   4. item half-sweep,               [RCCL: broadcast V row blocks]
//   5. test prediction + running mean RMSE (:539-563)
// Reference RNG mode pre-generates the sweep's whole variate stream on the
// host (it is data independent, see rng.h) and uploads it; Philox mode draws
// in-kernel.  No CPU compute fallback exists: without a GPU, sbmf_create fails.
#include "ctx.h"

namespace {
thread_local std::string g_err;
}

namespace sbmf {

[[noreturn]] void comm_fail(const char* what, ncclResult_t r) {
    fail(SBMF_E_COMM, "%s failed: %s", what, rccl_error_string((int)r));
}

Audit& audit() {
    static Audit a;
    return a;
}

}  // namespace sbmf

// ===================================================================== C ABI
sbmf_ctx::~sbmf_ctx() {
    vbo_destroy(vb);
    delete fm;
    using namespace sbmf;
    pinned_free(h_pinned, h_pinned_bytes);
    pinned_free(h_pre, h_pre_bytes);
    pinned_free(h_io, h_io_bytes);
    for (hipEvent_t& e : ev) event_destroy(e);
    for (hipEvent_t& e : kevs) event_destroy(e);
    for (hipEvent_t& e : sev) event_destroy(e);
    for (hipEvent_t& e : tsev) event_destroy(e);
    for (hipEvent_t& e : cev) event_destroy(e);
    for (hipEvent_t& e : oev) event_destroy(e);
    for (hipEvent_t& e : wev) event_destroy(e);
    for (hipEvent_t& e : fev) event_destroy(e);
    for (ScoreList* l : {&watch, &guests, &fmq}) l->drop();
    fmqd.drop();
    samples.drop();
    vbl.drop();
    pinned_free(h_fhyp, h_fhyp_bytes);
    event_destroy(hev);
    stream_destroy(sto);
    stream_destroy(sto2);
    stream_destroy(stc);
    stream_destroy(st);
    audit().contexts--;
}

namespace sbmf {
// sbmf_test_rccl_selftest: the exchange's RCCL calls through Comm's dlsym table on
// a one-rank communicator, issued on the comm stream while the item half's
// persistent k_gres grids (and its Gram-block launches) run on the compute
// streams -- the situation of the pipelined multi-GPU half (stage p's exchange
// beside stage p+1's compute), minus the peers.  Per repetition, one RCCL group of
// three in-place ncclBroadcast calls over adjacent blocks of a patterned buffer
// (as bcast_stage issues for U, the biases and the row sums), then the grouped
// ncclSend / ncclRecv of alltoallv (here to the rank itself), then an
// ncclAllGather.  Every byte is checked afterwards; the comm stream must finish
// within the deadline.
template <typename T>
void rccl_selftest(sbmf_ctx* c, uint64_t nbytes, uint32_t reps, double deadline_s, sbmf_rccl_selftest* out) {
    *out = sbmf_rccl_selftest{};
    Comm loop;
    loop.init_loopback();
    const size_t n = (size_t)nbytes, nag = n / 4;
    std::vector<uint8_t> pa(n), pb(n), pc(nag);
    for (size_t x = 0; x < n; ++x) {
        pa[x] = (uint8_t)(x * 2654435761u >> 13);
        pb[x] = (uint8_t)(x * 40503u + 17u);
    }
    for (size_t x = 0; x < nag; ++x) pc[x] = (uint8_t)(x * 97u + 5u);
    DBuf blk, snd, rcv, ags, agr;
    blk.alloc(n);
    snd.alloc(n);
    rcv.alloc(n);
    ags.alloc(nag);
    agr.alloc(nag);
    HIPCHK(hipMemcpy(blk.p, pa.data(), n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(snd.p, pb.data(), n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ags.p, pc.data(), nag, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    struct Events {  // destroyed on every path but a timeout (below)
        hipEvent_t e[4] = {};
        bool keep = false;
        ~Events() {
            if (!keep)
                for (hipEvent_t& x : e) event_destroy(x);
        }
    } evs;
    hipEvent_t* e = evs.e;
    for (int x = 0; x < 4; ++x) event_create(&e[x]);
    // three adjacent blocks of blk; the p2p segments [0, n/2) -> [n/2, n) and [n/2, n) -> [0, n/2)
    const std::vector<uint64_t> b0{0}, b1{n / 3}, b2{2 * (n / 3)}, b3{n};
    const std::vector<size_t> soff{0}, scnt{n / 2}, roff{n / 2}, rcnt{n / 2};
    const std::vector<size_t> soff2{n / 2}, scnt2{n / 2}, roff2{0}, rcnt2{n / 2};
    HIPCHK(hipEventRecord(e[0], c->st));
    for (uint32_t r = 0; r < reps; ++r) {
        run_half<T>(c, c->hyp[c->reported], false, 0);  // the item half: persistent k_gres grids on st (+ sto)
        if (r == 0) HIPCHK(hipEventRecord(e[2], c->stc));
        loop.group_begin();
        loop.bcast_blocks(blk.p, 1, b0, b1, c->stc);
        loop.bcast_blocks(blk.p, 1, b1, b2, c->stc);
        loop.bcast_blocks(blk.p, 1, b2, b3, c->stc);
        loop.group_end();
        loop.alltoallv(snd.p, r & 1 ? soff2 : soff, r & 1 ? scnt2 : scnt, rcv.p, r & 1 ? roff2 : roff,
                       r & 1 ? rcnt2 : rcnt, c->stc);
        loop.allgather(ags.p, nag, agr.p, c->stc);
        out->n_calls += 3 + 2 + 1;
    }
    HIPCHK(hipEventRecord(e[1], c->st));
    HIPCHK(hipEventRecord(e[3], c->stc));
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipEventQuery(e[3]);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) fail(SBMF_E_COMM, "RCCL self-test: %s", hipGetErrorString(q));
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > deadline_s) {
            // RCCL work is still queued on stc: abort the communicator instead of
            // destroying it, and leave the buffers and events in place (freeing them
            // would wait on the stuck stream); the context is dead from here on
            loop.abort();
            evs.keep = true;
            for (DBuf* b : {&blk, &snd, &rcv, &ags, &agr}) b->leak();
            c->dead = true;
            fail(SBMF_E_COMM, "RCCL self-test: the comm stream did not finish within %.1f s (communicator aborted, "
                              "context unusable)", deadline_s);
        }
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    HIPCHK(hipEventSynchronize(e[1]));
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, e[0], e[1]));
    out->ms_half = f;
    HIPCHK(hipEventElapsedTime(&f, e[2], e[3]));
    out->ms_rccl = f;
    HIPCHK(hipEventElapsedTime(&f, e[0], e[3]));
    out->ms_rccl_end = f;
    std::vector<uint8_t> h(n);
    HIPCHK(hipMemcpy(h.data(), blk.p, n, hipMemcpyDeviceToHost));
    for (size_t x = 0; x < n; ++x) out->bad_bcast += h[x] != pa[x];
    HIPCHK(hipMemcpy(h.data(), rcv.p, n, hipMemcpyDeviceToHost));
    // even repetitions send snd[0, n/2) to rcv[n/2, n), odd ones snd[n/2, n) to rcv[0, n/2)
    for (size_t x = 0; x < n; ++x) {
        if (x < n / 2 && reps == 1) continue;  // never written
        out->bad_p2p += h[x] != pb[x < n / 2 ? x + n / 2 : x - n / 2];
    }
    h.resize(nag);
    HIPCHK(hipMemcpy(h.data(), agr.p, nag, hipMemcpyDeviceToHost));
    for (size_t x = 0; x < nag; ++x) out->bad_allgather += h[x] != pc[x];
    out->overlapped = out->ms_rccl_end < out->ms_half ? 1u : 0u;
}
}  // namespace sbmf

// In a catch (...) of an entry point: the exception in flight as the thread's and the context's
// last error and its return code (anything but these three passes through)
int sbmf::api_error(sbmf_ctx* ctx) {
    int code = SBMF_E_ARG;
    try {
        throw;
    } catch (const sbmf::Error& e) {
        g_err = e.msg;
        code = e.code;
    } catch (const std::bad_alloc&) {
        g_err = "host allocation failed";
        code = SBMF_E_NOMEM;
    } catch (const std::exception& e) {
        g_err = e.what();
    }
    if (ctx) ctx->err = g_err;
    return code;
}

extern "C" {

int sbmf_abi_version(void) { return SBMF_ABI_VERSION; }

namespace {
int g_exit_rc = 1;
bool g_exit_guarded = false;
void exit_guard_handler() {
    std::fflush(nullptr);
    std::_Exit(g_exit_rc);
}
}  // namespace
int sbmf_exit_guard(int rc) {
    g_exit_rc = rc;
    if (g_exit_guarded) return SBMF_OK;
    if (std::atexit(exit_guard_handler) != 0) {
        g_err = "sbmf_exit_guard: atexit failed";
        return SBMF_E_STATE;
    }
    g_exit_guarded = true;
    return SBMF_OK;
}

int sbmf_config_default(sbmf_config* c) {
    if (!c) return SBMF_E_ARG;
    std::memset(c, 0, sizeof *c);
    c->num_factor = 20;  // gibbs_sbpmf_final.cpp:218
    c->num_iter = 100;   // :299
    c->burnin = 0;       // :300
    c->seed = 1;         // glibc default seed (the sampler never calls srand)
    c->rng_mode = SBMF_RNG_REFERENCE;
    c->quirks = SBMF_QUIRKS_FINAL;
    c->precision = SBMF_F64;
    c->device = 0;
    c->init_stdev = -1.0;
    c->clamp_lo = -1.0;
    c->clamp_hi = 5.0;
    c->a0 = 1;
    c->b0 = 1;
    c->alpha0 = 1;
    c->beta0 = 1;
    c->nu0 = 1;
    c->mu0 = 0.0;
    c->recompute_every = 1;
    c->eval_train = 0;
    c->eval_test = 1;
    c->libfm_dim = 3;  // libfm.cpp:130 default -dim 1,1,8
    return SBMF_OK;
}

const char* sbmf_last_error(const sbmf_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }
const char* sbmf_last_global_error(void) { return g_err.c_str(); }

int sbmf_create(const sbmf_config* cfg, sbmf_ctx** out) {
    sbmf_ctx* ctx = nullptr;
    API_BEGIN
    if (!cfg || !out) sbmf::fail(SBMF_E_ARG, "null argument");
    *out = nullptr;
    if (cfg->num_factor == 0 || cfg->num_factor > 256) sbmf::fail(SBMF_E_ARG, "num_factor must be in [1,256]");
    if (cfg->rng_mode != SBMF_RNG_REFERENCE && cfg->rng_mode != SBMF_RNG_PHILOX) sbmf::fail(SBMF_E_ARG, "bad rng_mode");
    if (cfg->quirks < 0 || cfg->quirks > 4) sbmf::fail(SBMF_E_ARG, "bad quirks");
    if (cfg->average > 2) sbmf::fail(SBMF_E_ARG, "bad average (0 default, 1 collected sweeps, 2 sweep + 1)");
    if (cfg->precision != SBMF_F64 && cfg->precision != SBMF_F32) sbmf::fail(SBMF_E_ARG, "bad precision");
    if (cfg->method > SBMF_METHOD_ALS) sbmf::fail(SBMF_E_ARG, "bad method");
    if (cfg->method == SBMF_METHOD_VB && cfg->precision != SBMF_F64)
        sbmf::fail(SBMF_E_ARG, "the online VB learner computes in f64 (the reference's double) only");
    if ((cfg->method == SBMF_METHOD_LIBFM_MCMC || cfg->method == SBMF_METHOD_ALS) && cfg->precision != SBMF_F64)
        sbmf::fail(SBMF_E_ARG, "the libFM MCMC / ALS learner computes in f64 (the reference's double) only");
    if (cfg->libfm_dim > 3) sbmf::fail(SBMF_E_ARG, "bad libfm_dim (bit 0 = w0, bit 1 = w)");
    if (cfg->task > SBMF_TASK_CLASSIFICATION) sbmf::fail(SBMF_E_ARG, "bad task (0 regression, 1 classification)");
    if (cfg->task == SBMF_TASK_CLASSIFICATION && cfg->method != SBMF_METHOD_LIBFM_MCMC && cfg->method != SBMF_METHOD_ALS) {
        static const char* const names[] = {"mcmc (the SBPMF sampler)", "vb (online VB)"};
        sbmf::fail(SBMF_E_ARG, "classification (task = SBMF_TASK_CLASSIFICATION) is libFM's MCMC / ALS learner's "
                               "(SBMF_METHOD_LIBFM_MCMC, SBMF_METHOD_ALS); method %s fits real-valued targets only",
                   names[cfg->method]);
    }
    {
        // the tune bits with a meaning in this build (include/sbmf.h); a bit of a removed variant
        // is refused, so a value saved for an older build does not silently pick something else
        // (INTEGRATION.md lists what changed between rounds)
        constexpr uint32_t known = (1u << 1) | (1u << 2) | (1u << 3) | (1u << 7) | (1u << 8) | (1u << 9) | (1u << 10) |
                                   (1u << 11) | (1u << 12) | (1u << 13) | (1u << 14) | (1u << 17) |
                                   (1u << 23) | (1u << 24) | (1u << 25) | (1u << 26) | (1u << 27) | (1u << 28) |
                                   (1u << 29) | (1u << 30);
        if (cfg->tune & ~known)
            sbmf::fail(SBMF_E_ARG, "tune bits 0x%x have no meaning in this build (variants removed earlier; see "
                                   "include/sbmf.h and INTEGRATION.md)", cfg->tune & ~known);
    }
    if (cfg->gram_threshold || cfg->row_kernel)
        sbmf::fail(SBMF_E_ARG, "gram_threshold / row_kernel are reserved (must be 0): the per-coordinate and "
                               "full-Gram row kernels were removed (measured slower than the Gram-block kernels)");
    int ndev = 0;
    const hipError_t derr = hipGetDeviceCount(&ndev);
    if (derr != hipSuccess || ndev <= 0)
        sbmf::fail(SBMF_E_DEVICE, "no HIP device available (%s; this library has no CPU fallback)",
                   derr != hipSuccess ? hipGetErrorString(derr) : "0 devices");
    if (cfg->device < 0 || cfg->device >= ndev) sbmf::fail(SBMF_E_DEVICE, "device %d out of range (%d)", cfg->device, ndev);
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        sbmf::fail(SBMF_E_DEVICE, "device %d is %s; this build targets gfx950 (MI355X)", cfg->device, prop.gcnArchName);
    HIPCHK(hipSetDevice(cfg->device));
    std::unique_ptr<sbmf_ctx> c(new sbmf_ctx());
    c->cfg = *cfg;
    // init 0.1 / clamp 0.5: src/libfm/gibbs_sbpmf2.cpp:240,557 and the top-level gibbs_sbpmf2.cpp:242,628
    const bool q2 = cfg->quirks == SBMF_QUIRKS_SBPMF2 || cfg->quirks == SBMF_QUIRKS_BIAS2;
    c->bias = cfg->quirks == SBMF_QUIRKS_BIAS2 || cfg->quirks == SBMF_QUIRKS_BIAS22;
    if (c->bias && (cfg->tune & 2u))
        sbmf::fail(SBMF_E_ARG, "tune bit 1 (residuals from r - own.partner) does not carry biases");
    c->init_sd = cfg->init_stdev >= 0 ? cfg->init_stdev : (q2 ? 0.1 : 1.0);
    c->lo = cfg->clamp_lo >= 0 ? cfg->clamp_lo : (q2 ? 0.5 : 1.0);
    c->hi = cfg->clamp_hi;
    c->sd_is_var = cfg->quirks == SBMF_QUIRKS_NONE ? 0 : 1;
    sbmf::stream_create(&c->st);
    sbmf::stream_create(&c->stc);
    for (auto& e : c->ev) sbmf::event_create(&e);
    for (auto& e : c->cev) sbmf::event_create(&e, hipEventDisableTiming);
    sbmf::stream_create(&c->sto);
    sbmf::stream_create(&c->sto2);
    for (auto& e : c->oev) sbmf::event_create(&e, hipEventDisableTiming);
    sbmf::event_create(&c->hev, hipEventDisableTiming);
    *out = c.release();
    API_END(ctx)
}

void sbmf_destroy(sbmf_ctx* ctx) {
    if (!ctx || ctx->dead) return;  // dead: work may still be queued (see sbmf_ctx::dead); leaked
    (void)hipSetDevice(ctx->cfg.device);
    (void)hipStreamSynchronize(ctx->st);
    delete ctx;
}

// The learner's set-up for the data given so far.  Every learner's dims: max id + 1 over train
// and test (gibbs_sbpmf_final.cpp:146-148), or sbmf_set_dims; for -method mcmc --order libfm / als
// I is the item attribute offset of the users-first layout
static bool libfm_method(const sbmf_ctx* c) {
    return c->cfg.method == SBMF_METHOD_LIBFM_MCMC || c->cfg.method == SBMF_METHOD_ALS;
}

// The general learner (fmg.cpp) on the cases given so far: one rank only
static void prepare_cases(sbmf_ctx* c, bool triples) {
    if (c->nranks > 1 || c->virt || c->comm != &c->own_comm || c->own_comm.active())
        sbmf::fail(SBMF_E_STATE, "the general libFM learner (cases with any number of features) runs on one rank: "
                                 "this context joined a communicator or is a virtual rank");
    c->K = c->cfg.num_factor;
    c->fm = fmg_create(c->cfg, c->ctr.view(), c->cte.view(), c->st, &c->fmgroups, &c->fmrels);
    if (triples) {  // the users-first layout: the model reads back by user / item
        c->fm->I = c->I;
        c->fm->J = c->J;
    }
    c->prepared = true;
}

// SBMF_FMM_GENERAL=1: the triples as cases {user u -> attribute u, item i -> I + i, x = 1}
static void triples_to_cases(const std::vector<uint32_t>& u, const std::vector<uint32_t>& i, const std::vector<double>& r,
                             uint32_t I, sbmf_ctx::HostCases& out) {
    const size_t n = u.size();
    out.ptr.resize(n + 1);
    out.attr.resize(2 * n);
    out.x.assign(2 * n, 1.0f);
    out.y.resize(n);
    uint32_t mx = 0;
    for (size_t q = 0; q < n; ++q) {
        if ((uint64_t)I + i[q] > 0xfffffffdull) sbmf::fail(SBMF_E_ARG, "attribute id too large");
        out.ptr[q] = 2 * q;
        out.attr[2 * q] = u[q];
        out.attr[2 * q + 1] = I + i[q];
        mx = std::max(mx, I + i[q]);
        out.y[q] = (float)r[q];
    }
    out.ptr[n] = 2 * n;
    out.num_attr = n ? mx + 1 : 0;
    out.set = true;
}

static void prepare_ctx(sbmf_ctx* c) {
    if (c->ctr.set) {
        prepare_cases(c, false);
        return;
    }
    if (c->cte.set) sbmf::fail(SBMF_E_STATE, "sbmf_set_test_cases without sbmf_set_train_cases");
    if (c->tu.empty()) sbmf::fail(SBMF_E_STATE, "no training data (sbmf_set_train)");
    uint32_t umax = 0, imax = 0;
    for (size_t x = 0; x < c->tu.size(); ++x) {
        umax = std::max(umax, c->tu[x]);
        imax = std::max(imax, c->ti[x]);
    }
    for (size_t x = 0; x < c->su.size(); ++x) {
        umax = std::max(umax, c->su[x]);
        imax = std::max(imax, c->si[x]);
    }
    c->I = std::max(c->I_req, umax + 1);
    c->J = std::max(c->J_req, imax + 1);
    c->K = c->cfg.num_factor;
    if (c->cfg.method == SBMF_METHOD_MCMC) {
        c->cfg.precision == SBMF_F32 ? prepare_T<float>(c) : prepare_T<double>(c);
        return;
    }
    sbmf::Comm* comm = c->nranks > 1 ? c->comm : nullptr;
    // a triples context given attribute groups takes the general learner: the two-attribute
    // kernels (fmm.hip) keep one group
    const char* gen = std::getenv("SBMF_FMM_GENERAL");
    const bool grouped = !c->fmgroups.group.empty() || !c->fmgroups.regw.empty() || !c->fmrels.empty();
    if (libfm_method(c) && ((gen && std::atoi(gen) != 0) || grouped)) {
        triples_to_cases(c->tu, c->ti, c->tr, c->I, c->ctr);
        triples_to_cases(c->su, c->si, c->sr, c->I, c->cte);
        prepare_cases(c, true);
        return;
    }
    if (c->cfg.method == SBMF_METHOD_VB)
        c->vb = vbo_create(c->cfg, c->tu.size(), c->tu.data(), c->ti.data(), c->tr.data(), c->su.size(), c->su.data(),
                           c->si.data(), c->sr.data(), c->I, c->J, c->st, comm);
    else
        c->fm = fmm_create(c->cfg, c->tu.size(), c->tu.data(), c->ti.data(), c->tr.data(), c->su.size(), c->su.data(),
                           c->si.data(), c->sr.data(), c->I, c->J, c->st, comm);
    c->prepared = true;
}

static void set_triples(uint64_t n, const uint32_t* u, const uint32_t* i, const double* r, std::vector<uint32_t>& U,
                        std::vector<uint32_t>& I, std::vector<double>& R) {
    if (n && (!u || !i || !r)) sbmf::fail(SBMF_E_ARG, "null array with n > 0");
    U.assign(u, u + n);
    I.assign(i, i + n);
    R.assign(r, r + n);
}

int sbmf_set_train(sbmf_ctx* ctx, uint64_t n, const uint32_t* user, const uint32_t* item, const double* rating) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (ctx->prepared) sbmf::fail(SBMF_E_STATE, "data already prepared");
    if (ctx->ctr.set || ctx->cte.set) sbmf::fail(SBMF_E_STATE, "the context already holds cases (sbmf_set_train_cases)");
    set_triples(n, user, item, rating, ctx->tu, ctx->ti, ctx->tr);
    API_END(ctx)
}

int sbmf_set_test(sbmf_ctx* ctx, uint64_t n, const uint32_t* user, const uint32_t* item, const double* rating) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (ctx->prepared) sbmf::fail(SBMF_E_STATE, "data already prepared");
    if (ctx->ctr.set || ctx->cte.set) sbmf::fail(SBMF_E_STATE, "the context already holds cases (sbmf_set_test_cases)");
    set_triples(n, user, item, rating, ctx->su, ctx->si, ctx->sr);
    API_END(ctx)
}

// the caller's cases, copied: entries sorted by attribute within a case (stable), a repeat refused
static void set_cases(const sbmf_cases* in, sbmf_ctx::HostCases& out, const char* fn) {
    if (!in) sbmf::fail(SBMF_E_ARG, "%s: null cases", fn);
    if ((in->n && (!in->ptr || !in->target)) || (in->nnz && (!in->attr || !in->x)))
        sbmf::fail(SBMF_E_ARG, "%s: null array", fn);
    if (in->n && (in->ptr[0] != 0 || in->ptr[in->n] != in->nnz))
        sbmf::fail(SBMF_E_ARG, "%s: ptr must run from 0 to nnz", fn);
    sbmf_ctx::HostCases h;
    h.ptr.assign(in->n + 1, 0);
    if (in->n) h.ptr.assign(in->ptr, in->ptr + in->n + 1);
    h.attr.assign(in->attr, in->attr + in->nnz);
    h.x.assign(in->x, in->x + in->nnz);
    h.y.assign(in->target, in->target + in->n);
    h.num_attr = in->num_attr;
    std::vector<std::pair<uint32_t, float>> tmp;
    for (uint64_t c = 0; c < in->n; ++c) {
        const uint64_t b = h.ptr[c], e = h.ptr[c + 1];
        if (e < b || e > in->nnz) sbmf::fail(SBMF_E_ARG, "%s: ptr decreases at case %llu", fn, (unsigned long long)c);
        bool sorted = true;
        for (uint64_t k = b; k < e; ++k) {
            if (h.attr[k] >= in->num_attr)
                sbmf::fail(SBMF_E_ARG, "%s: case %llu holds attribute %u >= num_attr %u", fn, (unsigned long long)c,
                           h.attr[k], in->num_attr);
            if (k > b && h.attr[k - 1] >= h.attr[k]) sorted = false;
        }
        if (sorted) continue;
        tmp.clear();
        for (uint64_t k = b; k < e; ++k) tmp.emplace_back(h.attr[k], h.x[k]);
        std::stable_sort(tmp.begin(), tmp.end(), [](const auto& a, const auto& b2) { return a.first < b2.first; });
        for (uint64_t k = b; k < e; ++k) {
            h.attr[k] = tmp[k - b].first;
            h.x[k] = tmp[k - b].second;
            if (k > b && h.attr[k - 1] == h.attr[k])
                sbmf::fail(SBMF_E_ARG, "%s: case %llu repeats attribute %u (the learner writes one record per case of "
                                       "a row)", fn, (unsigned long long)c, h.attr[k]);
        }
    }
    h.set = true;
    out = std::move(h);
}

static void check_cases_ctx(sbmf_ctx* ctx, const char* fn) {
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (ctx->prepared) sbmf::fail(SBMF_E_STATE, "data already prepared");
    static const char* const names[] = {"mcmc (the SBPMF sampler)", "vb (online VB)", "mcmc, libFM order", "als"};
    if (!libfm_method(ctx))
        sbmf::fail(SBMF_E_STATE, "%s: cases with any number of features are read by libFM's MCMC / ALS learner "
                                 "(SBMF_METHOD_LIBFM_MCMC, SBMF_METHOD_ALS) only; this context runs method %s",
                   fn, names[ctx->cfg.method]);
    if (!ctx->tu.empty() || !ctx->su.empty())
        sbmf::fail(SBMF_E_STATE, "%s: the context already holds triples (sbmf_set_train / sbmf_set_test)", fn);
}

int sbmf_set_train_cases(sbmf_ctx* ctx, const sbmf_cases* cases) {
    API_BEGIN
    check_cases_ctx(ctx, "sbmf_set_train_cases");
    set_cases(cases, ctx->ctr, "sbmf_set_train_cases");
    API_END(ctx)
}

int sbmf_set_test_cases(sbmf_ctx* ctx, const sbmf_cases* cases) {
    API_BEGIN
    check_cases_ctx(ctx, "sbmf_set_test_cases");
    set_cases(cases, ctx->cte, "sbmf_set_test_cases");
    API_END(ctx)
}

int sbmf_get_fm(sbmf_ctx* ctx, double* w0, double* w, double* v) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (!ctx->prepared) sbmf::fail(SBMF_E_STATE, "not prepared");
    if (!ctx->fm || !ctx->fm->nranges)
        sbmf::fail(SBMF_E_STATE, "sbmf_get_fm: this context does not run the general libFM learner");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    ctx->fm->model(w0, w, v);
    API_END(ctx)
}

int sbmf_fm_info(sbmf_ctx* ctx, uint32_t* num_attr, uint32_t* nranges, uint32_t* launches_per_iter) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (!ctx->prepared) sbmf::fail(SBMF_E_STATE, "not prepared");
    if (!ctx->fm || !ctx->fm->nranges)
        sbmf::fail(SBMF_E_STATE, "sbmf_fm_info: this context does not run the general libFM learner");
    if (num_attr) *num_attr = ctx->fm->p;
    if (nranges) *nranges = ctx->fm->nranges;
    if (launches_per_iter) *launches_per_iter = ctx->fm->n_launch;
    API_END(ctx)
}

// ---- libFM's attribute groups (-meta)
static void check_groups_ctx(sbmf_ctx* ctx, const char* fn) {
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (ctx->prepared) sbmf::fail(SBMF_E_STATE, "%s: data already prepared", fn);
    static const char* const names[] = {"mcmc (the SBPMF sampler)", "vb (online VB)", "mcmc, libFM order", "als"};
    if (ctx->virt) sbmf::fail(SBMF_E_STATE, "%s: this context is a virtual rank; attribute groups run on one rank", fn);
    if (ctx->nranks > 1 || ctx->comm != &ctx->own_comm || ctx->own_comm.active())
        sbmf::fail(SBMF_E_STATE, "%s: this context joined a communicator; attribute groups run on one rank", fn);
    if (!libfm_method(ctx))
        sbmf::fail(SBMF_E_STATE, "%s: attribute groups belong to libFM's MCMC / ALS learner (SBMF_METHOD_LIBFM_MCMC, "
                                 "SBMF_METHOD_ALS); this context runs method %s", fn, names[ctx->cfg.method]);
}

int sbmf_set_attr_groups(sbmf_ctx* ctx, uint32_t n, const uint32_t* group) {
    API_BEGIN
    check_groups_ctx(ctx, "sbmf_set_attr_groups");
    if (n && !group) sbmf::fail(SBMF_E_ARG, "sbmf_set_attr_groups: null array with n > 0");
    // with the data already given the count is checked here, else at sbmf_prepare
    uint64_t p = 0;
    if (ctx->ctr.set) {
        p = (uint64_t)std::max(ctx->ctr.num_attr, ctx->cte.set ? ctx->cte.num_attr : 0u) + 1;
    } else if (!ctx->tu.empty()) {
        uint32_t umax = 0, imax = 0;
        for (size_t x = 0; x < ctx->tu.size(); ++x) umax = std::max(umax, ctx->tu[x]), imax = std::max(imax, ctx->ti[x]);
        for (size_t x = 0; x < ctx->su.size(); ++x) umax = std::max(umax, ctx->su[x]), imax = std::max(imax, ctx->si[x]);
        p = (uint64_t)std::max(ctx->I_req, umax + 1) + imax + 2;
    }
    if (n && p && n != p)
        sbmf::fail(SBMF_E_ARG, "sbmf_set_attr_groups: %u group ids given, the context's num_attribute is %llu (largest "
                               "attribute id over train and test + 2)", n, (unsigned long long)p);
    ctx->fmgroups.group.assign(group, group + n);
    API_END(ctx)
}

int sbmf_set_group_regular(sbmf_ctx* ctx, uint32_t G, const double* regw, const double* regv) {
    API_BEGIN
    check_groups_ctx(ctx, "sbmf_set_group_regular");
    if (G && (!regw || !regv)) sbmf::fail(SBMF_E_ARG, "sbmf_set_group_regular: null array with G > 0");
    if (!ctx->fmgroups.group.empty() || !ctx->fmrels.empty()) {
        // the joined groups: the main table's, then every relation's own
        uint32_t have = ctx->fmgroups.group.empty()
                            ? 1 : *std::max_element(ctx->fmgroups.group.begin(), ctx->fmgroups.group.end()) + 1;
        for (const sbmf::FMRelation& r : ctx->fmrels) have += r.G;
        if (G && G != have && ctx->fmrels.empty())
            sbmf::fail(SBMF_E_ARG, "sbmf_set_group_regular: %u groups given, sbmf_set_attr_groups set %u", G, have);
        else if (G && G != have)
            sbmf::fail(SBMF_E_ARG, "sbmf_set_group_regular: %u groups given, sbmf_set_attr_groups and the %zu "
                                   "relations set %u", G, ctx->fmrels.size(), have);
    }
    ctx->fmgroups.regw.assign(regw, regw + G);
    ctx->fmgroups.regv.assign(regv, regv + G);
    API_END(ctx)
}

// ---- libFM's block-structure relations (-relation)
int sbmf_add_relation(sbmf_ctx* ctx, const sbmf_cases* block, const uint32_t* train_row, uint64_t n_train,
                      const uint32_t* test_row, uint64_t n_test, const uint32_t* group, uint32_t G) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (ctx->prepared) sbmf::fail(SBMF_E_STATE, "sbmf_add_relation: data already prepared");
    static const char* const names[] = {"mcmc (the SBPMF sampler)", "vb (online VB)", "mcmc, libFM order", "als"};
    if (ctx->virt)
        sbmf::fail(SBMF_E_STATE, "sbmf_add_relation: this context is a virtual rank; relations run on one rank");
    if (ctx->nranks > 1 || ctx->comm != &ctx->own_comm || ctx->own_comm.active())
        sbmf::fail(SBMF_E_STATE, "sbmf_add_relation: this context joined a communicator; relations run on one rank");
    if (!libfm_method(ctx))
        sbmf::fail(SBMF_E_STATE, "sbmf_add_relation: relations belong to libFM's MCMC / ALS learner "
                                 "(SBMF_METHOD_LIBFM_MCMC, SBMF_METHOD_ALS); this context runs method %s",
                   names[ctx->cfg.method]);
    if (!ctx->ctr.set && ctx->tu.empty())
        sbmf::fail(SBMF_E_STATE, "sbmf_add_relation: give the train / test cases first (the maps are checked against them)");
    if (ctx->fmrels.size() >= sbmf::FG_MAX_REL)
        sbmf::fail(SBMF_E_ARG, "sbmf_add_relation: a context takes at most %u relations", sbmf::FG_MAX_REL);
    if (!block) sbmf::fail(SBMF_E_ARG, "sbmf_add_relation: null block table");
    if ((block->n && !block->ptr) || (block->nnz && (!block->attr || !block->x)) || (n_train && !train_row) ||
        (n_test && !test_row))
        sbmf::fail(SBMF_E_ARG, "sbmf_add_relation: null array");
    if (block->n && (block->ptr[0] != 0 || block->ptr[block->n] != block->nnz))
        sbmf::fail(SBMF_E_ARG, "sbmf_add_relation: ptr must run from 0 to nnz");
    const uint64_t have_tr = ctx->ctr.set ? ctx->ctr.y.size() : ctx->tu.size();
    const uint64_t have_te = ctx->ctr.set ? ctx->cte.y.size() : ctx->su.size();
    if (n_train != have_tr)
        sbmf::fail(SBMF_E_ARG, "sbmf_add_relation: the train map holds %llu block-row indices, the train set %llu cases",
                   (unsigned long long)n_train, (unsigned long long)have_tr);
    if (n_test != have_te)
        sbmf::fail(SBMF_E_ARG, "sbmf_add_relation: the test map holds %llu block-row indices, the test set %llu cases",
                   (unsigned long long)n_test, (unsigned long long)have_te);
    for (uint64_t q = 0; q < n_train; ++q)
        if (train_row[q] >= block->n)
            sbmf::fail(SBMF_E_ARG, "sbmf_add_relation: train case %llu joins block row %u; the block table has %llu rows",
                       (unsigned long long)q, train_row[q], (unsigned long long)block->n);
    for (uint64_t q = 0; q < n_test; ++q)
        if (test_row[q] >= block->n)
            sbmf::fail(SBMF_E_ARG, "sbmf_add_relation: test case %llu joins block row %u; the block table has %llu rows",
                       (unsigned long long)q, test_row[q], (unsigned long long)block->n);
    sbmf::FMRelation r;
    r.ptr.assign(block->n + 1, 0);
    if (block->n) r.ptr.assign(block->ptr, block->ptr + block->n + 1);
    r.attr.assign(block->attr, block->attr + block->nnz);
    r.x.assign(block->x, block->x + block->nnz);
    r.num_attr = block->num_attr;
    std::vector<std::pair<uint32_t, float>> tmp;
    for (uint64_t j = 0; j < block->n; ++j) {  // entries by attribute within a block row, as set_cases
        const uint64_t b = r.ptr[j], e = r.ptr[j + 1];
        if (e < b || e > block->nnz)
            sbmf::fail(SBMF_E_ARG, "sbmf_add_relation: ptr decreases at block row %llu", (unsigned long long)j);
        tmp.clear();
        for (uint64_t k = b; k < e; ++k) {
            if (r.attr[k] >= block->num_attr)
                sbmf::fail(SBMF_E_ARG, "sbmf_add_relation: block row %llu holds attribute %u >= num_attr %u",
                           (unsigned long long)j, r.attr[k], block->num_attr);
            tmp.emplace_back(r.attr[k], r.x[k]);
        }
        std::stable_sort(tmp.begin(), tmp.end(), [](const auto& a, const auto& b2) { return a.first < b2.first; });
        for (uint64_t k = b; k < e; ++k) {
            r.attr[k] = tmp[k - b].first;
            r.x[k] = tmp[k - b].second;
            if (k > b && r.attr[k - 1] == r.attr[k])
                sbmf::fail(SBMF_E_ARG, "sbmf_add_relation: block row %llu repeats attribute %u (the passes write one "
                                       "record per block row of an attribute)", (unsigned long long)j, r.attr[k]);
        }
    }
    r.train_row.assign(train_row, train_row + n_train);
    r.test_row.assign(test_row, test_row + n_test);
    if (group && G) {
        r.group.assign(group, group + block->num_attr);
        for (uint32_t a = 0; a < block->num_attr; ++a)
            if (group[a] >= G)
                sbmf::fail(SBMF_E_ARG, "sbmf_add_relation: attribute %u has group %u; G = %u", a, group[a], G);
        r.G = G;
    }
    ctx->fmrels.push_back(std::move(r));
    API_END(ctx)
}

int sbmf_fm_relation_info(sbmf_ctx* ctx, uint32_t* nrel, uint32_t cap, uint32_t* attr_offset, uint32_t* num_attr,
                          uint32_t* block_rows, uint32_t* nranges, uint32_t* group_offset, uint32_t* num_groups) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (!ctx->prepared) sbmf::fail(SBMF_E_STATE, "not prepared");
    if (!ctx->fm || !ctx->fm->nranges)
        sbmf::fail(SBMF_E_STATE, "sbmf_fm_relation_info: this context does not run the general libFM learner");
    const auto& ri = ctx->fm->rel_info;
    if (nrel) *nrel = (uint32_t)ri.size();
    for (uint32_t r = 0; r < ri.size() && r < cap; ++r) {
        if (attr_offset) attr_offset[r] = ri[r].attr_offset;
        if (num_attr) num_attr[r] = ri[r].num_attr;
        if (block_rows) block_rows[r] = ri[r].block_rows;
        if (nranges) nranges[r] = ri[r].nranges;
        if (group_offset) group_offset[r] = ri[r].group_offset;
        if (num_groups) num_groups[r] = ri[r].G;
    }
    API_END(ctx)
}

int sbmf_get_fm_groups(sbmf_ctx* ctx, uint32_t* G, uint32_t* cnt, double* w_lambda, double* w_mu, double* v_lambda,
                       double* v_mu) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (!ctx->prepared) sbmf::fail(SBMF_E_STATE, "not prepared");
    if (!ctx->fm) sbmf::fail(SBMF_E_STATE, "sbmf_get_fm_groups: this context does not run libFM's MCMC / ALS learner");
    const sbmf::FMChain& f = *ctx->fm;
    if (G) *G = f.G;
    if (cnt) std::copy(f.cnt.begin(), f.cnt.end(), cnt);
    if (w_lambda) std::copy(f.w_lambda.begin(), f.w_lambda.end(), w_lambda);
    if (w_mu) std::copy(f.w_mu.begin(), f.w_mu.end(), w_mu);
    if (v_lambda) std::copy(f.v_lambda.begin(), f.v_lambda.end(), v_lambda);
    if (v_mu) std::copy(f.v_mu.begin(), f.v_mu.end(), v_mu);
    API_END(ctx)
}

int sbmf_test_fm_group_sums(sbmf_ctx* ctx, double* out) {
    API_BEGIN
    if (!ctx || !out) sbmf::fail(SBMF_E_ARG, "null argument");
    if (!ctx->prepared) sbmf::fail(SBMF_E_STATE, "not prepared");
    if (!ctx->fm || !ctx->fm->nranges)
        sbmf::fail(SBMF_E_STATE, "sbmf_test_fm_group_sums: this context does not run the general libFM learner");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    ctx->fm->group_sums(out);
    API_END(ctx)
}

int sbmf_test_tgauss(int mode, int device, uint64_t seed, uint32_t it, uint64_t n, const double* mean, const int32_t* sign,
                     const uint32_t* index, double* out) {
    sbmf_ctx* ctx = nullptr;
    API_BEGIN
    if (n && (!mean || !sign || !out)) sbmf::fail(SBMF_E_ARG, "null argument");
    if (mode == 1) {  // the host restatement over the reference's stream, consumed in index order
        sbmf::GlibcRand g((unsigned)seed);
        for (uint64_t i = 0; i < n; ++i)
            out[i] = sign[i] >= 0 ? sbmf::ran_left_tgaussian(g, 0.0, mean[i], 1.0)
                                  : sbmf::ran_right_tgaussian(g, 0.0, mean[i], 1.0);
    } else if (mode == 0) {
        if (n >= 0xffffffffull) sbmf::fail(SBMF_E_ARG, "more than 2^32-1 draws");
        int ndev = 0;
        const hipError_t derr = hipGetDeviceCount(&ndev);
        if (derr != hipSuccess || ndev <= 0)
            sbmf::fail(SBMF_E_DEVICE, "no HIP device available (%s; this library has no CPU fallback)",
                       derr != hipSuccess ? hipGetErrorString(derr) : "0 devices");
        if (device < 0 || device >= ndev) sbmf::fail(SBMF_E_DEVICE, "device %d out of range (%d)", device, ndev);
        HIPCHK(hipSetDevice(device));
        std::vector<float> y(n);
        for (uint64_t i = 0; i < n; ++i) y[i] = sign[i] >= 0 ? 1.0f : -1.0f;
        sbmf::DBuf d_mean, d_y, d_out, d_idx;
        if (index && n) {
            d_idx.alloc(n * sizeof(uint32_t));
            HIPCHK(hipMemcpy(d_idx.p, index, n * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
        d_mean.alloc(std::max<uint64_t>(n, 1) * sizeof(double));
        d_y.alloc(std::max<uint64_t>(n, 1) * sizeof(float));
        d_out.alloc(std::max<uint64_t>(n, 1) * sizeof(double));
        if (n) {
            HIPCHK(hipMemcpy(d_mean.p, mean, n * sizeof(double), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(d_y.p, y.data(), n * sizeof(float), hipMemcpyHostToDevice));
            HIPCHK(sbmf::fm_tgauss(seed, it, n, d_mean.as<double>(), d_y.as<float>(), d_idx.as<uint32_t>(), d_out.as<double>(),
                                   nullptr));
            HIPCHK(hipDeviceSynchronize());
            HIPCHK(hipMemcpy(out, d_out.p, n * sizeof(double), hipMemcpyDeviceToHost));
        }
    } else {
        sbmf::fail(SBMF_E_ARG, "sbmf_test_tgauss: mode %d (0 device, 1 host)", mode);
    }
    API_END(ctx)
}

int sbmf_fm_ranges(const sbmf_cases* train, uint32_t num_attr, uint32_t* bounds, uint32_t cap, uint32_t* nranges) {
    sbmf_ctx* ctx = nullptr;
    API_BEGIN
    if (!train || !nranges) sbmf::fail(SBMF_E_ARG, "null argument");
    if ((train->n && !train->ptr) || (train->nnz && !train->attr)) sbmf::fail(SBMF_E_ARG, "null array");
    if (train->n && train->ptr[train->n] != train->nnz) sbmf::fail(SBMF_E_ARG, "ptr[n] != nnz");
    for (uint64_t k = 0; k < train->nnz; ++k)
        if (train->attr[k] >= num_attr) sbmf::fail(SBMF_E_ARG, "attribute %u >= num_attr %u", train->attr[k], num_attr);
    std::vector<uint32_t> b;
    sbmf::fm_ranges(*train, num_attr, b);
    *nranges = (uint32_t)b.size() - 1;
    if (bounds) {
        if (cap < b.size()) sbmf::fail(SBMF_E_ARG, "bounds holds %u values, %zu needed", cap, b.size());
        std::copy(b.begin(), b.end(), bounds);
    }
    API_END(ctx)
}

int sbmf_set_dims(sbmf_ctx* ctx, uint32_t num_users, uint32_t num_items) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (ctx->prepared) sbmf::fail(SBMF_E_STATE, "data already prepared");
    ctx->I_req = num_users;
    ctx->J_req = num_items;
    API_END(ctx)
}

int sbmf_prepare(sbmf_ctx* ctx) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    if (ctx->prepared) return SBMF_OK;
    for (size_t x = 0; x < ctx->tu.size(); ++x)
        if ((ctx->I_req && ctx->tu[x] >= ctx->I_req) || (ctx->J_req && ctx->ti[x] >= ctx->J_req))
            sbmf::fail(SBMF_E_ARG, "rating %zu has an id beyond sbmf_set_dims", x);
    prepare_ctx(ctx);
    API_END(ctx)
}

int sbmf_run(sbmf_ctx* ctx, uint32_t sweeps, sbmf_sweep_cb cb, void* user) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (ctx->spent || ctx->dead)
        sbmf::fail(SBMF_E_STATE, "sbmf_test_rccl_selftest ran extra item halves on this context: its chain is no "
                                 "longer the sampler's; create a new context");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    if (!ctx->prepared) prepare_ctx(ctx);
    if (ctx->vb) {
        if (vbo_loaded(ctx->vb))
            sbmf::fail(SBMF_E_STATE, "sbmf_run: this context's posterior came from a file (sbmf_vb_load_posterior), which "
                                     "holds no natural parameters or step counts: training cannot resume from it");
        vbo_run(ctx->vb, sweeps, cb, user);
        ctx->timing = sbmf_timing{};
        ctx->timing.n_launch = vbo_launches(ctx->vb);
        ctx->timing.ms_vb_factor = vbo_factor_ms(ctx->vb);
        return SBMF_OK;
    }
    if (ctx->fm) {
        ctx->fm->run(sweeps, cb, user);
        ctx->timing = sbmf_timing{};
        ctx->timing.n_launch = ctx->fm->n_launch;
        return SBMF_OK;
    }
    ctx->cfg.precision == SBMF_F32 ? run_sweeps_T<float>(ctx, sweeps, cb, user) : run_sweeps_T<double>(ctx, sweeps, cb, user);
    API_END(ctx)
}

int sbmf_predict(sbmf_ctx* ctx, double* out) {
    API_BEGIN
    if (!ctx || !out) sbmf::fail(SBMF_E_ARG, "null argument");
    if (!ctx->prepared) sbmf::fail(SBMF_E_STATE, "not prepared");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    if (ctx->vb) {
        vbo_predict_out(ctx->vb, out);
        return SBMF_OK;
    }
    if (ctx->fm) {
        ctx->fm->predict_out(out);
        return SBMF_OK;
    }
    const uint64_t T_ = ctx->su.size();
    if (ctx->nranks > 1) ctx->comm->bcast_ranges(ctx->d_tsum.p, sizeof(double), ctx->tbounds, ctx->st);
    HIPCHK(hipStreamSynchronize(ctx->st));
    std::vector<double> h(T_);
    HIPCHK(hipMemcpy(h.data(), ctx->d_tsum.p, T_ * sizeof(double), hipMemcpyDeviceToHost));
    const double div = sbmf::avg_collected(ctx->cfg) ? (double)std::max(1u, ctx->collected) : (double)std::max(1u, ctx->sweep);
    for (uint64_t j = 0; j < T_; ++j) out[ctx->tperm[j]] = h[j] / div;  // device (user) order -> file order
    API_END(ctx)
}

int sbmf_get_factors(sbmf_ctx* ctx, double* U, double* V) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (!ctx->prepared) sbmf::fail(SBMF_E_STATE, "not prepared");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->st));
    if (ctx->vb) {
        vbo_factors(ctx->vb, U, V);
        return SBMF_OK;
    }
    if (ctx->fm) {  // libFM's v of the users [I][K] and items [J][K]
        ctx->fm->factors(U, V);
        return SBMF_OK;
    }
    if (U) sbmf::download_table(ctx, ctx->d_U, U, ctx->I);
    if (V) sbmf::download_table(ctx, ctx->d_V, V, ctx->J);
    API_END(ctx)
}

int sbmf_set_factors(sbmf_ctx* ctx, const double* U, const double* V) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (!ctx->prepared) sbmf::fail(SBMF_E_STATE, "not prepared");
    if (ctx->vb || ctx->fm)
        sbmf::fail(SBMF_E_STATE, "sbmf_set_factors is not supported by the VB / libFM learners");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->st));
    ctx->pre.valid = false;  // hyperparameters drawn ahead from the old tables
    if (U) sbmf::upload_table(ctx, ctx->d_U, U, ctx->I);
    if (V) sbmf::upload_table(ctx, ctx->d_V, V, ctx->J);
    API_END(ctx)
}

int sbmf_get_hyper(sbmf_ctx* ctx, double* h, double* tau) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (!ctx->prepared) sbmf::fail(SBMF_E_STATE, "not prepared");
    if (ctx->vb) {
        HIPCHK(hipSetDevice(ctx->cfg.device));
        vbo_hyper_out(ctx->vb, h, tau);
        return SBMF_OK;
    }
    if (ctx->fm) {
        ctx->fm->hyper_out(h, tau);
        return SBMF_OK;
    }
    const uint32_t K = ctx->K;
    const Hyper& hy = ctx->hyp[ctx->reported];
    if (h) {
        std::copy(hy.sig_u.begin(), hy.sig_u.end(), h);
        std::copy(hy.mu_u.begin(), hy.mu_u.end(), h + K);
        std::copy(hy.sig_v.begin(), hy.sig_v.end(), h + 2 * K);
        std::copy(hy.mu_v.begin(), hy.mu_v.end(), h + 3 * K);
    }
    if (tau) *tau = hy.tau;
    API_END(ctx)
}

int sbmf_get_biases(sbmf_ctx* ctx, double* bu, double* bv, double* b0) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (!ctx->prepared) sbmf::fail(SBMF_E_STATE, "not prepared");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    if (ctx->vb) {  // posterior means of w (users, items) and w0
        vbo_biases(ctx->vb, bu, bv, b0);
        return SBMF_OK;
    }
    if (ctx->fm) {  // libFM's w (users, items) and w0
        ctx->fm->biases(bu, bv, b0);
        return SBMF_OK;
    }
    if (!ctx->bias) sbmf::fail(SBMF_E_STATE, "not a biased sampler (quirks bias2 / bias22) or the VB learner");
    HIPCHK(hipStreamSynchronize(ctx->st));
    if (bu) HIPCHK(hipMemcpy(bu, ctx->d_bu.p, (size_t)ctx->I * sizeof(double), hipMemcpyDeviceToHost));
    if (bv) HIPCHK(hipMemcpy(bv, ctx->d_bv.p, (size_t)ctx->J * sizeof(double), hipMemcpyDeviceToHost));
    if (b0) *b0 = ctx->hyp[ctx->reported].b0;
    API_END(ctx)
}

int sbmf_get_dims(sbmf_ctx* ctx, uint32_t* nu, uint32_t* ni, uint64_t* ntr, uint64_t* nte) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (nu) *nu = ctx->I;
    if (ni) *ni = ctx->J;
    const bool cases = ctx->ctr.set && ctx->tu.empty();  // given as cases (never beside triples): no user / item dims
    if (ntr) *ntr = cases ? ctx->ctr.y.size() : ctx->tu.size();
    if (nte) *nte = cases ? ctx->cte.y.size() : ctx->su.size();
    API_END(ctx)
}

int sbmf_get_timing(sbmf_ctx* ctx, sbmf_timing* t) {
    API_BEGIN
    if (!ctx || !t) sbmf::fail(SBMF_E_ARG, "null argument");
    *t = ctx->timing;
    // per sweep, both halves: N*(sK + 4 + 4) + rows*2*sK
    const uint64_t s = sbmf::tsize(ctx);
    const uint64_t N = ctx->tu.size();
    t->bytes_algorithmic = 2 * N * (s * ctx->K + 4 + s) + ((uint64_t)ctx->I + ctx->J) * 2 * s * ctx->K;
    API_END(ctx)
}

int sbmf_comm_unique_id(uint8_t id[128]) {
    sbmf_ctx* ctx = nullptr;
    API_BEGIN
    if (!id) sbmf::fail(SBMF_E_ARG, "null id");
    sbmf::Comm::unique_id(id);
    API_END(ctx)
}

int sbmf_comm_init(sbmf_ctx* ctx, int nranks, int rank, const uint8_t id[128]) {
    API_BEGIN
    if (!ctx || !id) sbmf::fail(SBMF_E_ARG, "null argument");
    if (ctx->prepared) sbmf::fail(SBMF_E_STATE, "sbmf_comm_init must precede sbmf_prepare");
    if (nranks < 1 || rank < 0 || rank >= nranks) sbmf::fail(SBMF_E_ARG, "bad rank %d / %d", rank, nranks);
    HIPCHK(hipSetDevice(ctx->cfg.device));
    ctx->nranks = nranks;
    ctx->rank = rank;
    if (ctx->comm != &ctx->own_comm) sbmf::fail(SBMF_E_STATE, "context already attached to a communicator");
    if (nranks > 1) ctx->comm->init(nranks, rank, id);
    API_END(ctx)
}

// one communicator per process, shared by every context of the process (bench.py's
// legs): RCCL's set-up runs once, not once per learner
struct sbmf_comm {
    sbmf::Comm c;
    int device = 0, nranks = 1, rank = 0;
};

int sbmf_comm_create(int device, int nranks, int rank, const uint8_t id[128], sbmf_comm** out) {
    sbmf_ctx* ctx = nullptr;
    API_BEGIN
    if (!id || !out) sbmf::fail(SBMF_E_ARG, "null argument");
    *out = nullptr;
    if (nranks < 1 || rank < 0 || rank >= nranks) sbmf::fail(SBMF_E_ARG, "bad rank %d / %d", rank, nranks);
    if (device < 0) sbmf::fail(SBMF_E_ARG, "bad device %d", device);
    std::unique_ptr<sbmf_comm> cm(new sbmf_comm());
    cm->device = device;
    cm->nranks = nranks;
    cm->rank = rank;
    if (nranks > 1) {
        // RCCL binds the communicator to the current device: this rank's, set first
        HIPCHK(hipSetDevice(device));
        cm->c.init(nranks, rank, id);
    }
    *out = cm.release();
    API_END(ctx)
}

int sbmf_comm_attach(sbmf_ctx* ctx, sbmf_comm* comm) {
    API_BEGIN
    if (!ctx || !comm) sbmf::fail(SBMF_E_ARG, "null argument");
    if (ctx->prepared) sbmf::fail(SBMF_E_STATE, "sbmf_comm_attach must precede sbmf_prepare");
    if (ctx->own_comm.active() || ctx->virt) sbmf::fail(SBMF_E_STATE, "context already joined a communicator");
    if (comm->nranks > 1 && comm->device != ctx->cfg.device)
        sbmf::fail(SBMF_E_ARG, "communicator on device %d, context on device %d", comm->device, ctx->cfg.device);
    ctx->nranks = comm->nranks;
    ctx->rank = comm->rank;
    ctx->comm = &comm->c;
    API_END(ctx)
}

void sbmf_comm_destroy(sbmf_comm* comm) { delete comm; }

int sbmf_test_virtual_rank(sbmf_ctx* ctx, int nranks, int rank) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    if (ctx->prepared) sbmf::fail(SBMF_E_STATE, "sbmf_test_virtual_rank must precede sbmf_prepare");
    if (nranks < 2 || rank < 0 || rank >= nranks) sbmf::fail(SBMF_E_ARG, "bad rank %d / %d", rank, nranks);
    if (ctx->cfg.method != SBMF_METHOD_MCMC) sbmf::fail(SBMF_E_ARG, "virtual ranks: the SBPMF sampler only");
    if (ctx->comm->active() || ctx->comm != &ctx->own_comm)
        sbmf::fail(SBMF_E_STATE, "context already joined a communicator");
    ctx->nranks = nranks;
    ctx->rank = rank;
    ctx->virt = true;
    API_END(ctx)
}

int sbmf_test_stage_ms(sbmf_ctx* ctx, double* ms, uint32_t cap, uint32_t* nstages) {
    API_BEGIN
    if (!ctx || !nstages) sbmf::fail(SBMF_E_ARG, "null argument");
    if (!ctx->virt || !ctx->prepared) sbmf::fail(SBMF_E_STATE, "stage times need a prepared virtual rank");
    *nstages = ctx->nstages;
    if (ms && cap < 2 * ctx->nstages) sbmf::fail(SBMF_E_ARG, "need %u slots", 2 * ctx->nstages);
    HIPCHK(hipStreamSynchronize(ctx->st));
    for (uint32_t sd = 0; ms && sd < 2; ++sd)
        for (uint32_t p = 0; p < ctx->nstages; ++p) {
            float f = 0.f;
            const size_t tb = (size_t)sd * (ctx->nstages + 1);
            HIPCHK(hipEventElapsedTime(&f, ctx->tsev[tb + p], ctx->tsev[tb + p + 1]));
            ms[sd * ctx->nstages + p] = f;
        }
    API_END(ctx)
}

int sbmf_test_rccl_selftest(sbmf_ctx* ctx, uint64_t nbytes, uint32_t reps, double deadline_s,
                            sbmf_rccl_selftest* out) {
    API_BEGIN
    if (!ctx || !out) sbmf::fail(SBMF_E_ARG, "null argument");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    if (!ctx->prepared || ctx->nranks != 1 || ctx->cfg.method != SBMF_METHOD_MCMC)
        sbmf::fail(SBMF_E_STATE, "the RCCL self-test needs a prepared one-rank sampler context");
    if (nbytes < 64 || nbytes % 64 || reps == 0) sbmf::fail(SBMF_E_ARG, "nbytes a positive multiple of 64, reps >= 1");
    if (ctx->spent || ctx->dead) sbmf::fail(SBMF_E_STATE, "the RCCL self-test already ran on this context");
    ctx->spent = true;  // from the first extra half on, the chain is not the sampler's
    ctx->cfg.precision == SBMF_F32 ? sbmf::rccl_selftest<float>(ctx, nbytes, reps, deadline_s, out)
                                   : sbmf::rccl_selftest<double>(ctx, nbytes, reps, deadline_s, out);
    API_END(ctx)
}

int sbmf_test_device_usage(int device, sbmf_device_usage* out) {
    sbmf_ctx* ctx = nullptr;
    API_BEGIN
    if (!out) sbmf::fail(SBMF_E_ARG, "null argument");
    *out = sbmf_device_usage{};
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        sbmf::fail(SBMF_E_DEVICE, "no HIP device %d", device);
    HIPCHK(hipSetDevice(device));
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    out->device_free = fr;
    out->device_total = tot;
    const sbmf::Audit& a = sbmf::audit();
    out->dev_bytes = a.dev_bytes.load();
    out->dev_allocs = a.dev_allocs.load();
    out->pinned_bytes = a.pinned_bytes.load();
    out->pinned_allocs = a.pinned_allocs.load();
    out->streams = a.streams.load();
    out->events = a.events.load();
    out->contexts = a.contexts.load();
    out->comms = a.comms.load();
    API_END(ctx)
}

int sbmf_partition_rows(const uint32_t* ptr, uint32_t R, int nranks, uint64_t* bounds) {
    sbmf_ctx* ctx = nullptr;
    API_BEGIN
    if (!ptr || !bounds || nranks < 1) sbmf::fail(SBMF_E_ARG, "bad arguments");
    sbmf::partition_bounds(ptr, R, nranks, bounds);
    API_END(ctx)
}

int sbmf_ref_stream(uint32_t seed, int kind, double shape, uint64_t n, double* out) {
    sbmf_ctx* ctx = nullptr;
    API_BEGIN
    if (!out && n) sbmf::fail(SBMF_E_ARG, "null out");
    sbmf::GlibcRand g(seed);
    for (uint64_t x = 0; x < n; ++x) {
        if (kind == 0)
            out[x] = g.next();
        else if (kind == 1)
            out[x] = sbmf::leva_normal(g);
        else
            out[x] = sbmf::mt_gamma(g, shape);
    }
    API_END(ctx)
}

int sbmf_philox_normals(uint64_t seed, uint32_t sweep, uint32_t tag, uint32_t row, uint32_t K, double* out) {
    sbmf_ctx* ctx = nullptr;
    API_BEGIN
    if (!out && K) sbmf::fail(SBMF_E_ARG, "null out");
    for (uint32_t k = 0; k < K; k += 2) {
        double z0, z1;
        sbmf::philox_normal_pair(seed, row, sweep, tag, k / 2, z0, z1);
        out[k] = z0;
        if (k + 1 < K) out[k + 1] = z1;
    }
    API_END(ctx)
}

}  // extern "C"
