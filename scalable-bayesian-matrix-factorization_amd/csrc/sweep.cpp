// sweep.cpp -- the sampler's sweeps: the host's variates and hyperparameter draws, the launch
// schedule of a half-sweep, the multi-rank exchange and the loop of sbmf_run.
#include "ctx.h"

namespace sbmf {

// ------------------------------------------------------------------ one sweep
struct HostStream {  // variates of one sweep, in the reference's consumption order
    double g_tau;
    double g_sb0 = 0, z_mb0 = 0, z_b0 = 0;  // biased sampler: sigma_b0, mu_b0, b0
    std::vector<double> g_su, z_mu, g_sv, z_mv;
};

// Unbiased samplers: tau (:339-342), then per k {sigma_u, mu_u, sigma_v, mu_v}
// (:375-414).  Biased sampler (top-level gibbs_sbpmf2.cpp:366-467): alpha with
// shape a0 + N, sigma_b0 / mu_b0 / b0, then per k with shapes alpha0 + I / + J.
template <class G>
static void draw_hyper_variates(G& g, sbmf_ctx* c, HostStream& hs) {
    const sbmf_config& cf = c->cfg;
    const uint64_t N = c->tu.size();
    if (c->bias) {
        hs.g_tau = mt_gamma(g, cf.a0 + (double)N);
        hs.g_sb0 = mt_gamma(g, cf.alpha0 + 1);
        hs.z_mb0 = leva_normal(g);
        hs.z_b0 = leva_normal(g);
    } else {
        hs.g_tau = mt_gamma(g, cf.a0 + 0.5 * (double)N);
    }
    hs.g_su.resize(c->K);
    hs.z_mu.resize(c->K);
    hs.g_sv.resize(c->K);
    hs.z_mv.resize(c->K);
    const double shu = c->bias ? cf.alpha0 + c->I : cf.alpha0 + 0.5 * (c->I + 1);
    const double shv = c->bias ? cf.alpha0 + c->J : cf.alpha0 + 0.5 * (c->J + 1);
    for (uint32_t k = 0; k < c->K; ++k) {
        hs.g_su[k] = mt_gamma(g, shu);
        hs.z_mu[k] = leva_normal(g);
        hs.g_sv[k] = mt_gamma(g, shv);
        hs.z_mv[k] = leva_normal(g);
    }
}

// Reference mode, biased sampler: the per-row bias hyperparameter variates of
// every user then every item (:470-489, :492-511), then per user {b_i, K
// factor normals} (:515-558) and per item {b_j, K normals} (:563-606).
//
// ran_gaussian(mean, stdev) consumes no variate when stdev is 0 or NaN
// (random.h:166-172).  That happens for rows without train ratings: their
// bias draw has variance 1/sigma_b (no data term), so under the reference's
// variance-as-stdev quirk the walk b -> N(mu, 1/sigma_b), sigma_b ~ 1/b^2
// grows like b^2 per sweep, overflows, and turns NaN within a few dozen
// sweeps.  From then on the reference skips those draws.  The walk of such a
// row depends only on its own variates, so the host replays it here in the
// reference's exact expressions to know which draws the stream skips (a
// skipped slot carries 0: the device then yields the mean, as the reference
// does); k_bias_rows evaluates the same expressions without contraction and
// reaches the same values.
template <typename T>
static void fill_bias_variates(sbmf_ctx* c, const Hyper& hy) {
    const uint32_t K = c->K;
    const sbmf_config& cf = c->cfg;
    auto sdv = [&](double var) { return c->sd_is_var ? var : std::sqrt(var); };
    auto consumes = [](double sd) { return !(sd == 0.0 || std::isnan(sd)); };
    auto hyper_rows = [&](uint32_t R, const std::vector<uint32_t>& empty, std::vector<std::array<double, 3>>& sh,
                          std::vector<double>& v) {
        size_t e = 0;
        for (uint32_t r = 0; r < R; ++r) {
            const double g = mt_gamma(c->grand, cf.alpha0 + 1);
            v[3 * (size_t)r] = g;
            if (e < empty.size() && empty[e] == r) {  // shadow: (b, mu, sigma)
                std::array<double, 3>& x = sh[e++];
                x[2] = g / (cf.beta0 + (0.5 * (x[0] - x[1]) * (x[0] - x[1])));
                const double s4 = 1.0 / (cf.nu0 + x[2]);
                const double mean = s4 * ((cf.nu0 * cf.mu0) + x[0] * x[2]);
                const double z = consumes(sdv(s4)) ? leva_normal(c->grand) : 0.0;
                v[3 * (size_t)r + 1] = z;
                x[1] = consumes(sdv(s4)) ? mean + sdv(s4) * z : mean;
            } else {
                v[3 * (size_t)r + 1] = leva_normal(c->grand);
            }
        }
    };
    auto bias_draw = [&](const std::vector<uint32_t>& empty, std::vector<std::array<double, 3>>& sh, uint32_t r,
                         size_t& e) -> double {
        if (e < empty.size() && empty[e] == r) {
            std::array<double, 3>& x = sh[e++];
            const double sb = 1 / (x[2] + (hy.tau * 0.0));
            const double mb = sb * ((x[2] * x[1]) + hy.tau * 0.0);
            if (!consumes(sdv(sb))) {
                x[0] = mb;
                return 0.0;
            }
            const double z = leva_normal(c->grand);
            x[0] = mb + sdv(sb) * z;
            return z;
        }
        return leva_normal(c->grand);
    };
    std::vector<double> vu((size_t)3 * c->I), vv((size_t)3 * c->J);
    hyper_rows(c->I, c->empty_u, c->shadow_u, vu);
    hyper_rows(c->J, c->empty_v, c->shadow_v, vv);
    const size_t nz = ((size_t)c->I + c->J) * K;
    ensure_pinned(c, nz * sizeof(T));
    T* h = reinterpret_cast<T*>(c->h_pinned);
    size_t e = 0;
    for (uint32_t i = 0; i < c->I; ++i) {
        vu[3 * (size_t)i + 2] = bias_draw(c->empty_u, c->shadow_u, i, e);
        for (uint32_t k = 0; k < K; ++k) h[(size_t)i * K + k] = (T)leva_normal(c->grand);
    }
    T* hv = h + (size_t)c->I * K;
    e = 0;
    for (uint32_t j = 0; j < c->J; ++j) {
        vv[3 * (size_t)j + 2] = bias_draw(c->empty_v, c->shadow_v, j, e);
        for (uint32_t k = 0; k < K; ++k) hv[(size_t)j * K + k] = (T)leva_normal(c->grand);
    }
    HIPCHK(hipMemcpy(c->d_zU.p, h, (size_t)c->I * K * sizeof(T), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->d_zV.p, hv, (size_t)c->J * K * sizeof(T), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->d_var3u.p, vu.data(), vu.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->d_var3v.p, vv.data(), vv.size() * sizeof(double), hipMemcpyHostToDevice));
}

static BiasArgs bias_args(const sbmf_ctx* c, const Hyper& hy, bool users, double d0) {
    BiasArgs p{};
    p.alpha = hy.tau;
    p.d0 = d0;
    p.ag = c->cfg.alpha0;
    p.bg = c->cfg.beta0;
    p.sg = c->cfg.nu0;
    p.mg = c->cfg.mu0;
    p.seed = c->cfg.seed;
    p.sweep = c->sweep;
    p.tag = users ? TAG_BIAS_U : TAG_BIAS_V;
    p.sd_is_var = c->sd_is_var;
    return p;
}

template <typename T>
static void fill_z(sbmf_ctx* c, uint32_t R, DBuf& d) {
    const size_t n = (size_t)R * c->K;
    ensure_pinned(c, n * sizeof(T));
    T* h = reinterpret_cast<T*>(c->h_pinned);
    for (size_t x = 0; x < n; ++x) h[x] = (T)leva_normal(c->grand);
    HIPCHK(hipMemcpy(d.p, h, n * sizeof(T), hipMemcpyHostToDevice));
}

template <typename T>
static HalfArgs<T> half_args(sbmf_ctx* c, const Hyper& hy, bool users) {
    HalfArgs<T> a{};
    const bool md = c->nranks > 1;
    if (users) {
        a.ptr = c->d_uptr.as<uint32_t>();
        a.part = c->d_upart.as<uint32_t>();
        a.perm = (md ? c->d_uperm2 : c->d_uperm).as<uint32_t>();
        a.E_this = c->d_Eu.as<T>();   // user order
        a.E_other = c->d_Ev.as<T>();  // item order
        a.r_this = c->d_ur.as<T>();
        a.own = c->d_U.as<T>();
        a.partner = c->d_V.as<T>();
        a.sig = c->d_hyper.as<T>();
        a.mu = c->d_hyper.as<T>() + c->Kp;
        a.zrow = c->J;
        a.zbuf = c->d_zU.as<T>();
        a.tag = TAG_USERS;
        a.row_sq = nullptr;
        a.row_tr = nullptr;
    } else {
        a.ptr = c->d_vptr.as<uint32_t>();
        a.part = c->d_vpart.as<uint32_t>();
        a.perm = (md ? c->d_vperm2 : c->d_vperm).as<uint32_t>();
        a.E_this = c->d_Ev.as<T>();   // item order
        a.E_other = c->d_Eu.as<T>();  // user order
        a.r_this = c->d_vr.as<T>();
        a.own = c->d_V.as<T>();
        a.partner = c->d_U.as<T>();
        a.sig = c->d_hyper.as<T>() + 2 * c->Kp;
        a.mu = c->d_hyper.as<T>() + 3 * c->Kp;
        a.zrow = c->I;
        a.zbuf = c->d_zV.as<T>();
        a.tag = TAG_ITEMS;
        a.row_sq = c->d_rowsq_v.as<double>();
        a.row_tr = c->cfg.eval_train ? c->d_rowtr_v.as<double>() : nullptr;
    }
    a.tune = c->cfg.tune;
    a.prof = c->kprof ? c->d_kprof.as<unsigned long long>() + 16 + 8 * (users ? 0 : 1) : nullptr;
    a.tau = (T)hy.tau;
    a.K = c->K;
    a.Kp = c->Kp;
    a.sd_is_var = c->sd_is_var;
    a.seed = c->cfg.seed;
    a.sweep = c->sweep;
    a.lo = (T)c->lo;
    a.hi = (T)c->hi;
    a.lim_partner = (uint64_t)((users ? c->J : c->I) + 2) * c->Kp;
    a.lim_other = (uint64_t)c->tu.size() + (users ? c->users.nsend : c->items.nsend);
    a.lim_this = c->tu.size();
    a.lim_rows = users ? c->I : c->J;
    // tune bit 1: residuals from r - own.partner (the former multi-GPU form, kept for validation);
    // otherwise every rank reads the residuals the exchange delivered
    a.e_from_dot = (c->cfg.tune & 2u) ? 1 : 0;
    return a;
}

// The device copy of a streaming launch's cold block, in slot `slot` ((stage * 2 + side) * 3 +
// shape) of d_gcold: uploaded here if it differs from what the device holds.  The block's fields
// are the context's buffers and configuration, fixed from set_data on, and every stage has slots
// of its own, so in a chain of sweeps each slot is uploaded the first time its launch runs and
// never again, with one stage per half or several; a change (new buffers, another tune) drains
// the streams that may still read the old block first.  SBMF_COLD_LOG=1 reports each upload.
template <typename T>
static const GresCold<T>* cold_block(sbmf_ctx* c, int slot, const GresCold<T>& cold) {
    static_assert(sizeof(GresCold<T>) <= sbmf_ctx::kColdSlot, "cold block slot");
    unsigned char* h = c->h_gcold.data() + (size_t)slot * sbmf_ctx::kColdSlot;
    unsigned char* d = c->d_gcold.as<unsigned char>() + (size_t)slot * sbmf_ctx::kColdSlot;
    if (std::memcmp(h, &cold, sizeof(cold)) != 0) {
        for (hipStream_t s : {c->st, c->sto, c->sto2}) HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipMemcpy(d, &cold, sizeof(cold), hipMemcpyHostToDevice));
        std::memcpy(h, &cold, sizeof(cold));
        static const bool log = std::getenv("SBMF_COLD_LOG") != nullptr;
        if (log) std::fprintf(stderr, "[sbmf] cold block upload: slot %d, sweep %u\n", slot, c->sweep);
    }
    return reinterpret_cast<const GresCold<T>*>(d);
}

// `start` (optional): a timing event the caller has just recorded on the compute stream with
// nothing queued there since.  The half then forks its side streams from it and, when nothing
// precedes its first kind on the compute stream, times that kind from it: two event records
// back to back on a stream leave the device idle ~6 us each (r04f trace; ML-1M K=50 r05s42:
// 37 us between the user half's end and the item half's streaming launch).
template <typename T>
void run_half(sbmf_ctx* c, const Hyper& hy, bool users, uint32_t stage, hipEvent_t start) {
    Side& s = users ? c->users : c->items;
    Side::Stage& g = *s.stg[stage];
    HalfArgs<T> a = half_args<T>(c, hy, users);
    hipStream_t st = c->st;
    const int sd = users ? 0 : 1;
    // Overlap (default; tune bit 29 off): the streaming launch (persistent, queue
    // order) on `st`, every other bin on `sto` beside it, so the short Gram-block
    // launches fill the CU time the streaming launch's serial phases (solve,
    // split-row hand-offs) and its tail leave idle.  Rows of different bins are
    // disjoint and no launch reads another's outputs, so the results do not
    // depend on the interleaving.  The streaming launch is an ordinary one in every
    // schedule (its claiming workgroups are resident by construction; tune bit 24's
    // cooperative launch, experiments only, would wait for the whole device).
    int others = 0;
    for (int k = 0; k < NBIN; ++k) others += k != KIND_STREAM && !g.bin_rows[k].empty();
    const bool serial = (c->cfg.tune & 0x20000000u) != 0;
    const bool ovl = !serial && others && !g.bin_rows[KIND_STREAM].empty();
    // The Gram-block kinds alternate between two side streams (sto, sto2), so they also run
    // beside each other: a small stage's kinds are each bound by one row's latency through
    // its k-blocks, which a chain of launches adds up (r05s2 per-rank trace).  Per-rank
    // compute of the 8-way split, 4 stages: K=100 2.06 -> 1.96 ms, K=200 3.09 -> 2.76 ms;
    // the single-GPU sweep is unchanged (7.33 both ways, r05s5).  Tune bit 25: one side stream.
    // With two stream sets (items: rows > 1024 on 16-wave workgroups, set 1, and the
    // rest on 8-wave ones, set 0), set 1 runs on `st` and set 0 on `sto` beside it
    // (tune bit 30: one after the other), each with split-row areas of its own.
    // Side by side pays nothing at ML-20M (r05s32, neutral) and costs on small stages (ML-1M K=50:
    // 0.424-0.453 ms side by side, 0.416-0.423 in turn, r05s43): below kSetsSideMin ratings in the
    // stage (ML-1M, a rank's stage of an 8-way ML-20M split) the sets run one after the other
    // (SBMF_SETS_SIDE_MIN overrides the threshold: measurements only)
    static const uint64_t kSetsSideMin = [] {
        const char* e = std::getenv("SBMF_SETS_SIDE_MIN");
        return e ? (uint64_t)std::strtoull(e, nullptr, 10) : (uint64_t)4000000;
    }();
    const bool big = (uint64_t)(s.ptr[g.r1] - s.ptr[g.r0]) >= kSetsSideMin;
    const bool sov = ovl && big && !(c->cfg.tune & 0x40000000u) && !g.ss[0].stasks.empty() && !g.ss[1].stasks.empty();
    // Beside two streaming sets every Gram-block kind goes to sto2: on sto it would queue behind
    // set 0 (r05s14 trace: two item kinds, 0.18 ms, ran after the stage; measured neutral, 6.91
    // ms both ways, r05s15: the persistent sets hold every CU, so the kinds' work only moves)
    const bool two = !serial && (others >= 2 || sov) && !(c->cfg.tune & 0x2000000u);
    const bool side = ovl || two;
    // (the long-row set alone first, every other launch of the half after it, so its split rows'
    // chunks share no CU with other launches' workgroups: user half 2.77-2.81 -> 2.86-3.04 ms,
    // item half neutral, r06s6; not kept)
    // (the split-row counters and queue heads of both stream sets are zero: each streaming
    // launch's k_split_finish clears its own)
    bool st_busy = false;  // something queued on the compute stream since `start`
    auto fork = [&] {
        hipEvent_t f = start && !st_busy ? start : c->oev[0];
        if (f == c->oev[0]) HIPCHK(hipEventRecord(c->oev[0], c->st));
        HIPCHK(hipStreamWaitEvent(c->sto, f, 0));
        if (two) HIPCHK(hipStreamWaitEvent(c->sto2, f, 0));
    };
    if (side) fork();
    // (the Gram-block launches on `sto` ahead of set 0 instead of behind it: neutral, r04s22)
    int last[3] = {-1, -1, -1};  // the last kind launched on st / sto / sto2 (its end event recorded there)
    int nside = 0;  // Gram-block kinds launched so far (two: even ones on sto, odd ones on sto2)
    for (int k = NBIN - 1; k >= 0; --k) {
        if (g.bin_rows[k].empty()) continue;
        st = side && k != KIND_STREAM ? (two && (sov || (nside++ & 1)) ? c->sto2 : c->sto) : c->st;
        // launch-kind events: the streaming kind's every sweep (the bench's roofline), the
        // others' on the first sweep of a run only (each event between two launches on a
        // stream leaves the device idle ~6 us)
        const bool timed = c->time_kinds || k == KIND_STREAM;
        int& lk = last[st == c->st ? 0 : st == c->sto ? 1 : 2];
        if (timed) {
            c->kpv(stage, sd, k) = (int8_t)lk;
            if (lk < 0) {
                if (st == c->st && start && !st_busy) {
                    c->kbg(stage, sd, k) = start;  // the caller's event is this kind's start
                } else {
                    HIPCHK(hipEventRecord(c->kev(stage, sd, k, 0), st));
                    c->kbg(stage, sd, k) = c->kev(stage, sd, k, 0);
                }
            }
            lk = k;
        } else {
            lk = -1;  // no end event behind this launch
        }
        // f64 rows of 65..128 ratings on one-wave k_grow workgroups, 129..256 on two-wave ones
        // (the streaming kernel's code on whole rows: 32 vectors per wave, one wave with no
        // cross-wave sum or D hand-off) instead of 3-4-wave Gram-block rows: user half
        // 3.20-3.24 -> 2.93-3.04 ms, sweep 7.22-7.25 -> 7.02-7.06 (r05s11, 2 interleaved
        // rounds); the 9..64-rating bin too, on one-wave k_grow workgroups (sweep 6.99-7.03 ->
        // 6.90-6.95, r05s12).  Tune bits 8 / 9 / 10 keep the Gram-block kinds of these bins.
        const uint32_t tn = c->cfg.tune;
        // f32 rows of 17..256 ratings on one-wave k_grow workgroups, 257..512 on two-wave ones (64
        // vectors per f32 wave): f32 sweep 5.46 -> 4.63 ms (r05s18); tune bit 11 keeps the
        // Gram-block kinds
        const bool g32 = sizeof(T) == 4 && !(tn & 0x800u);
        const int gw = g32 ? (k == GK_W16 || k == GK_B2 || k == GK_B4 ? 1 : k == GK_B8 ? 2 : 0)
                       : sizeof(T) != 8                               ? 0
                       : k == GK_B4 && !(tn & 0x100u)                 ? 1
                       : k == GK_B8 && !(tn & 0x200u)                 ? 2
                       : k == GK_W16 && !(tn & 0x400u) && !(tn & 8u)  ? 1
                                                                      : 0;
        if (gw) {
            HIPCHK(launch_grow<T>(gw, g.d_bins[k].as<uint32_t>(), (uint32_t)g.bin_rows[k].size(), a,
                                  cold_block<T>(c, (2 * (int)stage + sd) * 3 + 2, gres_cold<T>(a, nullptr)), st));
        } else if (k < GK_NUM && k >= GK_B2 && !(c->cfg.tune & 4u)) {
            for (const auto& gs : g.gsub[k])
                HIPCHK(launch_gblock_nw<T>((int)gs[0], g.d_bins[k].as<uint32_t>() + gs[1], gs[2], a, st));
        } else if (k < GK_NUM)
            HIPCHK(launch_gblock<T>(k, g.d_bins[k].as<uint32_t>(), (uint32_t)g.bin_rows[k].size(), a, st));
        else {
            for (int q = 0; q < 2; ++q) {
                const int set = sov ? 1 - q : q;  // set 1 (the long rows) first
                const Side::StreamSet& S = g.ss[set];
                if (S.stasks.empty()) continue;
                const hipStream_t ss = sov && set == 0 ? c->sto : st;
                const size_t ox = set ? c->xset_nx : 0;
                SplitSync sy{};
                sy.nblk = (c->K + 15) / 16;
                sy.slabs = c->d_xslabs.as<double>() + ox * sy.nblk * SLAB_DOUBLES;
                sy.qhead = c->d_xcnt.as<uint32_t>() + 32 * set;  // a 128-byte line each
                sy.chunk_sq = c->d_xchunk_sq.as<double>() + ox;
                sy.chunk_tr = c->d_xchunk_tr.as<double>() + ox;
                sy.newown = c->d_xnewown.as<T>() + ox * c->Kp;
                sy.timeout = reinterpret_cast<uint32_t*>(c->d_res.as<double>() + RES_TIMEOUT);
                sy.cmax = S.cmax;
                sy.lim_slab = (uint64_t)(c->d_xslabs.bytes / sizeof(double)) - ox * sy.nblk * SLAB_DOUBLES;
                sy.lim_chunk = (uint32_t)(c->d_xchunk_sq.bytes / sizeof(double) - ox);
                sy.prof = c->kprof && set == c->kprof_set ? c->d_kprof.as<unsigned long long>() + 8 * (users ? 0 : 1) : nullptr;
                HalfArgs<T> as = a;
                as.tune = S.tune;
                HIPCHK(launch_gstream<T>(g.d_stasks[set].as<SplitTask>(), (uint32_t)S.stasks.size(), S.sgrid,
                                         g.d_xrows[set].as<SplitRow>(), (uint32_t)S.xrows.size(), as, sy,
                                         cold_block<T>(c, (2 * (int)stage + sd) * 3 + set, gres_cold<T>(as, &sy)), ss));
                if (ss == c->st) st_busy = true;
            }
            if (sov) {  // the streaming stage ends with both sets
                HIPCHK(hipEventRecord(c->oev[2], c->sto));
                HIPCHK(hipStreamWaitEvent(st, c->oev[2], 0));
            }
        }
        if (st == c->st) st_busy = true;
        // (a kind launched next on this stream starts its time at this event)
        if (timed) HIPCHK(hipEventRecord(c->kev(stage, sd, k, 1), st));
        c->launches++;
    }
    if (side) {
        HIPCHK(hipEventRecord(c->oev[1], c->sto));
        HIPCHK(hipStreamWaitEvent(c->st, c->oev[1], 0));
        if (two) {
            HIPCHK(hipEventRecord(c->oev[3], c->sto2));
            HIPCHK(hipStreamWaitEvent(c->st, c->oev[3], 0));
        }
    }
}

// After a stage of a half (users: scatter into item order, E_v; items: into
// E_u): send the stage's residuals bound for other ranks' rows, unpack what
// every rank's same stage sends here.  `with(p)` (optional) issues the stage's
// block broadcasts first, all in one RCCL group (collectives only: they run
// concurrently); the residual send/receive keeps a group of its own; the
// unpack follows it.  Offsets are taken relative to the stage's segments, so a
// transfer touches only this stage's part of the send and receive areas.
template <typename T, class F>
static void exchange_stage(sbmf_ctx* c, bool users, uint32_t p, hipStream_t st, F&& with) {
    if (c->nranks <= 1) return;
    const Side& s = users ? c->users : c->items;
    const Side::Stage& g = *s.stg[p];
    DBuf& E = users ? c->d_Ev : c->d_Eu;
    auto rel = [](const std::vector<size_t>& v, size_t base) {
        std::vector<size_t> b(v);
        for (size_t& x : b) x = (x - base) * sizeof(T);
        return b;
    };
    auto bytes = [](const std::vector<size_t>& v) {
        std::vector<size_t> b(v);
        for (size_t& x : b) x *= sizeof(T);
        return b;
    };
    c->comm->group_begin();
    with(p);
    c->comm->group_end();
    const size_t s0 = g.soff.empty() ? 0 : g.soff[0];
    c->comm->alltoallv(E.as<T>() + c->tu.size() + s0, rel(g.soff, s0), bytes(g.scnt), c->d_xrecv.as<T>() + g.rbeg,
                      rel(g.roff, g.rbeg), bytes(g.rcnt), st);
    HIPCHK(launch_unpack<T>(c->d_xrecv.as<T>() + g.rbeg, (users ? c->d_uunpack : c->d_vunpack).as<uint32_t>() + g.rbeg,
                            g.rend - g.rbeg, E.as<T>(), st));
}
// Every stage's residual exchange, on `st` (no broadcasts: the prologue's recompute)
template <typename T>
static void exchange_residuals(sbmf_ctx* c, bool users, hipStream_t st) {
    for (uint32_t p = 0; p < c->nstages; ++p) exchange_stage<T>(c, users, p, st, [](uint32_t) {});
}
// Every rank's units of stage p of `s` (its rows [sbounds[k][p], sbounds[k][p+1]))
static void bcast_stage(sbmf_ctx* c, const Side& s, uint32_t p, void* base, size_t unit_bytes) {
    std::vector<uint64_t> lo(c->nranks), hi(c->nranks);
    for (int k = 0; k < c->nranks; ++k) {
        lo[k] = s.sbounds[k][p];
        hi[k] = s.sbounds[k][p + 1];
    }
    c->comm->bcast_blocks(base, unit_bytes, lo, hi, c->stc);
}
// A half's stages, each followed -- on the comm stream, while the next stage
// computes -- by its exchange; the compute stream then waits for the last one.
template <typename T, class F>
static void run_half_pipelined(sbmf_ctx* c, const Hyper& hy, bool users, F&& bcasts, hipEvent_t start = nullptr) {
    const int sd = users ? 0 : 1;
    const size_t tb = (size_t)sd * (c->nstages + 1);
    if (c->virt) HIPCHK(hipEventRecord(c->tsev[tb], c->st));
    for (uint32_t p = 0; p < c->nstages; ++p) {
        run_half<T>(c, hy, users, p, p == 0 && !c->virt ? start : nullptr);
        if (c->nranks > 1) HIPCHK(hipEventRecord(c->sev[(size_t)sd * c->nstages + p], c->st));
        if (c->virt) HIPCHK(hipEventRecord(c->tsev[tb + p + 1], c->st));
    }
    HIPCHK(hipEventRecord(c->ev[users ? 2 : 4], c->st));
    if (c->nranks <= 1) return;  // no exchange: ev[3] / ev[5] are not recorded (the sweep uses ev[2] / ev[4])
    for (uint32_t p = 0; p < c->nstages; ++p) {
        HIPCHK(hipStreamWaitEvent(c->stc, c->sev[(size_t)sd * c->nstages + p], 0));
        exchange_stage<T>(c, users, p, c->stc, bcasts);
    }
    HIPCHK(hipEventRecord(c->cev[sd], c->stc));
    HIPCHK(hipStreamWaitEvent(c->st, c->cev[sd], 0));
}

// SBMF_KPROF=1: the streaming kernels' phase cycles of sweep `s_cur`, read and cleared
static void kprof_report(sbmf_ctx* c, uint32_t s_cur) {
    unsigned long long h[128];
    HIPCHK(hipMemcpy(h, c->d_kprof.p, sizeof(h), hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(c->d_kprof.p, 0, sizeof(h)));
    static const char* gn[7] = {"setup", "load+mfma", "barrier", "reduce", "solve+handoff", "e-update",
                                "epilogue"};
    for (int sd = 0; sd < 2; ++sd) {
        double tot = 0;
        for (int k = 0; k < 7; ++k) tot += (double)h[16 + 8 * sd + k];
        if (tot == 0) continue;
        std::fprintf(stderr, "[kprof] sweep %u %s gblock multi-wave rows (wave-0 Gcycles total):", s_cur,
                     sd ? "items" : "users");
        for (int k = 0; k < 7; ++k)
            std::fprintf(stderr, " %s %.3f (%.0f%%)", gn[k], (double)h[16 + 8 * sd + k] / 1e9,
                         100.0 * (double)h[16 + 8 * sd + k] / tot);
        std::fprintf(stderr, "\n");
    }
    static const char* nm[7] = {"stage", "apply+issue", "gather+acc", "wg-wait", "xwave+xchg", "solve", "epilogue"};
    for (int sd = 0; sd < 2; ++sd) {
        const Side& S = sd ? c->items : c->users;
        double tot = 0;
        // phase 4 (cross-wave sum + split-row exchange) comes in three parts: the sum and
        // the publish [96 + 2 sd], the publish to the first valid batch [97 + 2 sd], and
        // the rest (read + sum) in slot 4; per class at [100 + 6 sd + 2 cl]
        const unsigned long long x7 = h[96 + 2 * sd], x8 = h[97 + 2 * sd], x4 = h[8 * sd + 4];
        h[8 * sd + 4] += x7 + x8;
        for (int k = 0; k < 7; ++k) tot += (double)h[8 * sd + k];
        if (tot == 0) continue;
        std::fprintf(stderr, "[kprof] sweep %u gres %s (grid %u, %zu tasks, wave-0 Mcycles per WG):", s_cur,
                     sd ? "items" : "users", S.stg[0]->ss[c->kprof_set].sgrid,
                     S.stg[0]->ss[c->kprof_set].stasks.size());
        for (int k = 0; k < 7; ++k)
            std::fprintf(stderr, " %s %.3f (%.0f%%)", nm[k], (double)h[8 * sd + k] / S.stg[0]->ss[c->kprof_set].sgrid / 1e6,
                         100.0 * (double)h[8 * sd + k] / tot);
        std::fprintf(stderr, "\n[kprof]   xwave+xchg = xwave+publish %.3f + to-first-valid %.3f + read+sum %.3f\n",
                     (double)x7 / S.stg[0]->ss[c->kprof_set].sgrid / 1e6, (double)x8 / S.stg[0]->ss[c->kprof_set].sgrid / 1e6,
                     (double)x4 / S.stg[0]->ss[c->kprof_set].sgrid / 1e6);
        static const char* cn[3] = {"whole rows", "2-16 chunks", ">16 chunks"};
        for (int cl = 0; cl < 3; ++cl) {
            unsigned long long* hc = h + 32 + 24 * sd + 8 * cl;
            if (!hc[7]) continue;
            const unsigned long long* hx = h + 100 + 6 * sd + 2 * cl;
            const unsigned long long c4 = hc[4];
            hc[4] += hx[0] + hx[1];
            std::fprintf(stderr, "[kprof]   %s: %llu tasks, kcycles per task:", cn[cl], hc[7]);
            for (int k = 0; k < 7; ++k) std::fprintf(stderr, " %s %.1f", nm[k], (double)hc[k] / hc[7] / 1e3);
            std::fprintf(stderr, " (xwave+publish %.1f, to-first-valid %.1f, read+sum %.1f)\n", (double)hx[0] / hc[7] / 1e3,
                         (double)hx[1] / hc[7] / 1e3, (double)c4 / hc[7] / 1e3);
        }
    }
}

// ---- 2. host draws (:339-342, :375-414): a sweep's hyperparameters `next` from the previous
// sweep's `prev`, the prologue's sums `res` (the d_res layout) and the sweep's variates.  Reads
// configuration, dimensions and flags from the context and writes only `next`; returns d0
static double draw_hyper(const sbmf_ctx* c, const Hyper& prev, const double* res, const HostStream& hs, Hyper& next) {
    const sbmf_config& cf = c->cfg;
    const uint32_t K = c->K;
    const uint64_t N = c->tu.size();
    const bool q2 = cf.quirks == SBMF_QUIRKS_SBPMF2;
    const double* Su2 = &res[RES_COL];
    const double* Su1 = Su2 + K;
    const double* Sv2 = Su2 + 2 * K;
    const double* Sv1 = Su2 + 3 * K;
    auto sd = [&](double var) { return c->sd_is_var ? var : std::sqrt(var); };
    for (std::vector<double>* v : {&next.sig_u, &next.mu_u, &next.sig_v, &next.mu_v}) v->resize(K);
    double d0 = 0.0;  // biased sampler: global-bias delta, folded into the user half's residual pass
    if (c->bias) {
        // top-level gibbs_sbpmf2.cpp:366-467 (= src/libfm/gibbs_sbpmf22.cpp:345-446)
        const double es = res[RES_ES], esq = res[RES_ESQ2];
        next.tau = hs.g_tau / (cf.b0 + esq);
        next.sig_b0 = hs.g_sb0 / (cf.beta0 + (0.5 * (prev.b0 - prev.mu_b0) * (prev.b0 - prev.mu_b0)));
        const double s0 = 1.0 / (cf.nu0 + next.sig_b0);
        next.mu_b0 = s0 * ((cf.nu0 * cf.mu0) + prev.b0 * next.sig_b0) + sd(s0) * hs.z_mb0;
        const double sb0 = 1 / (next.sig_b0 + next.tau * (double)N);
        const double mb0 = sb0 * (next.sig_b0 * next.mu_b0 + next.tau * (es + (double)N * prev.b0));
        next.b0 = mb0 + sd(sb0) * hs.z_b0;
        d0 = prev.b0 - next.b0;
        for (uint32_t k = 0; k < K; ++k) {
            next.sig_u[k] = hs.g_su[k] / (cf.beta0 + (0.5) * Su2[k]);
            const double s2 = 1 / (cf.nu0 + next.sig_u[k] * c->I);
            next.mu_u[k] = s2 * (cf.nu0 * cf.mu0 + next.sig_u[k] * Su1[k]) + sd(s2) * hs.z_mu[k];
            next.sig_v[k] = hs.g_sv[k] / (cf.beta0 + (0.5) * Sv2[k]);
            const double s1 = 1 / (cf.nu0 + next.sig_v[k] * c->J);
            next.mu_v[k] = s1 * (cf.nu0 * cf.mu0 + next.sig_v[k] * Sv1[k]) + sd(s1) * hs.z_mv[k];
        }
    } else {
        const double esq = res[RES_ESQ];
        next.tau = hs.g_tau / (cf.b0 + 0.5 * esq);
        for (uint32_t k = 0; k < K; ++k) {
            const double du = prev.mu_u[k] - cf.mu0;
            const double bu = q2 ? cf.beta0 + cf.nu0 * du * du + (0.5) * Su2[k]
                                 : cf.beta0 + 0.5 * cf.nu0 * du * du + (0.5) * Su2[k];
            next.sig_u[k] = hs.g_su[k] / bu;
            const double su_star = (double)1.0 / (cf.nu0 * next.sig_u[k] + next.sig_u[k] * c->I);
            const double mu_star = su_star * (cf.nu0 * cf.mu0 * next.sig_u[k] + next.sig_u[k] * Su1[k]);
            next.mu_u[k] = mu_star + sd(su_star) * hs.z_mu[k];
            const double dv = prev.mu_v[k] - cf.mu0;
            const double bv = q2 ? cf.beta0 + cf.nu0 * dv * dv + (0.5) * Sv2[k]
                                 : cf.beta0 + 0.5 * cf.nu0 * dv * dv + (0.5) * Sv2[k];
            next.sig_v[k] = hs.g_sv[k] / bv;
            const double sv_star = (double)1.0 / (cf.nu0 * next.sig_v[k] + next.sig_v[k] * c->J);
            const double mv_star = (q2 ? su_star : sv_star) * (cf.nu0 * cf.mu0 * next.sig_v[k] + next.sig_v[k] * Sv1[k]);
            next.mu_v[k] = mv_star + sd(sv_star) * hs.z_mv[k];
        }
    }
    return d0;
}

// One run of sweeps (sbmf_run): the run's constants and the steps of a sweep, in the order
// run() takes them.  Every step that depends on the hyperparameters is given those of the sweep
// it works for.
template <typename T>
struct SweepRun {
    sbmf_ctx* const c;
    const sbmf_config& cf = c->cfg;
    const hipStream_t st = c->st;
    const uint32_t K = c->K;
    const uint64_t N = c->tu.size(), T_ = c->su.size();
    const bool ref = cf.rng_mode == SBMF_RNG_REFERENCE;
    const bool q2 = cf.quirks == SBMF_QUIRKS_SBPMF2;
    double* const d_res = c->d_res.as<double>();
    double* const scratch = c->d_scratch.as<double>();
    // Throughput mode (Philox: the draws of sweep s depend only on (seed, s)): the
    // next sweep's prologue -- residual sum of squares, column statistics and the
    // host hyperparameter draws -- is issued at the end of this sweep, its kernels
    // beside the test evaluation (one rank; before it otherwise) and its host draws
    // while the evaluation runs, so
    // the GPU does not wait for the host round trip at the start of the next
    // sweep.  The inputs are the same (U, V and the residuals do not change in
    // between), so the chain is bitwise the same.  Tune bit 26 turns it off.
    const bool overlap = !ref && !(cf.tune & 0x4000000u);
    // One rank: the evaluation runs on the second stream beside the next prologue's kernels
    // (tune bit 28: after them)
    const bool par_eval = overlap && c->nranks == 1 && !(cf.tune & 0x10000000u);
    // one rank: nothing between the halves and after the item half, so their events are the
    // halves' end events (two timing events back to back leave the device idle ~12 us)
    const hipEvent_t ev3 = c->nranks > 1 ? c->ev[3] : c->ev[2];
    const hipEvent_t ev5 = c->nranks > 1 ? c->ev[5] : c->ev[4];
    // where the user half's time starts: the sweep's start event when the start work was staged ahead
    hipEvent_t ev1(bool staged) const { return staged ? c->ev[0] : c->ev[1]; }

    // ---- 1. the prologue's kernels for sweep sw (`prev`: sweep sw - 1's hyperparameters); its
    // sums land in c->h_pre
    void prologue_gpu(uint32_t sw, const Hyper& prev) {
        // ---- 1. residual sum of squares (E recompute at sweep start, :317-334)
        const bool recompute = sw == 0 || (cf.recompute_every && sw % cf.recompute_every == 0);
        if (recompute) {
            // residuals of every rating, scattered into user order for the user half
            HIPCHK(launch_resid<T>(c->d_rtasks.as<ResidTask>(), (uint32_t)c->items.rtasks.size(),
                                   c->d_rtptr.as<uint32_t>(), c->items.r0, c->items.r1, c->d_vpart.as<uint32_t>(),
                                   (c->nranks > 1 ? c->d_vperm2 : c->d_vperm).as<uint32_t>(), c->d_vr.as<T>(),
                                   c->d_V.as<T>(), c->d_U.as<T>(), K,
                                   c->Kp, c->d_Eu.as<T>(), c->d_rtsq.as<double>(), c->d_rowsq_v.as<double>(),
                                   c->bias ? c->d_bv.as<double>() : nullptr, c->d_bu.as<double>(), prev.b0, st));
            c->launches++;
            if (c->nranks > 1) c->comm->bcast_ranges(c->d_rowsq_v.p, sizeof(double), c->items.bounds, st);
            exchange_residuals<T>(c, false, st);
        }
        HIPCHK(launch_sum(c->d_rowsq_v.as<double>(), c->J, d_res + RES_ESQ, scratch, st));
        // biased sampler: sum(E) and sum(E^2) of the sweep-start residuals (:342-359), per
        // own user row, rows exchanged, summed in row order (the same for any rank split)
        if (c->bias) {
            double* rs2 = c->d_epart.as<double>();
            HIPCHK(launch_rowsum2<T>(c->d_uptr.as<uint32_t>(), c->users.r0, c->users.r1, c->d_Eu.as<T>(), rs2, st));
            if (c->nranks > 1) c->comm->bcast_ranges(rs2, 2 * sizeof(double), c->users.bounds, st);
            HIPCHK(launch_sum_cols(rs2, c->I, 2, d_res + RES_ES, st));
        }
        // ---- column statistics with the current mu (:378-381, :397-401)
        const T* hyp = c->d_hyper.as<T>();
        double* colpart = c->d_colpart.as<double>();
        double* colpart_v = colpart + (size_t)((c->I + 255) / 256) * 2 * K;
        HIPCHK(launch_colstats<T>(c->d_U.as<T>(), c->I, hyp + c->Kp, colpart, c->d_V.as<T>(), c->J, hyp + 3 * c->Kp,
                                  colpart_v, K, c->Kp, st));
        HIPCHK(launch_sum_cols2(colpart, (c->I + 255) / 256, d_res + RES_COL, colpart_v, (c->J + 255) / 256,
                                d_res + RES_COL + 2 * K, 2 * K, st));
        c->launches += 3;
        HIPCHK(hipMemcpyAsync(c->h_pre, d_res, c->h_res.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    // the hyperparameters `hy` [sig_u | mu_u | sig_v | mu_v] into the pinned staging area
    // and on to d_hyper (stream order: after every launch already queued that reads it)
    void stage_hyper(const Hyper& hy) {
        const size_t Kp = c->Kp;
        T* h = static_cast<T*>(c->h_hyper());
        HIPCHK(hipEventSynchronize(c->hev));
        std::fill(h, h + 4 * Kp, T(0));
        for (uint32_t k = 0; k < K; ++k) {
            h[k] = (T)hy.sig_u[k];
            h[Kp + k] = (T)hy.mu_u[k];
            h[2 * Kp + k] = (T)hy.sig_v[k];
            h[3 * Kp + k] = (T)hy.mu_v[k];
        }
        HIPCHK(hipMemcpyAsync(c->d_hyper.p, h, 4 * Kp * sizeof(T), hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(c->hev, st));
    }
    // A sweep's start: its hyperparameters (drawn here, or staged at the end of the previous sweep in
    // throughput mode) and its user half.  Returns whether the start work was staged ahead, and
    // the start's kernel launches.
    struct Start {
        bool staged;
        uint32_t n_launch;
    };
    Start start_sweep(bool first) {
        c->time_kinds = first;  // every launch kind timed on the first sweep of the run
        const uint32_t n0 = c->launches;
        HIPCHK(hipEventRecord(c->ev[0], st));
        double d0;
        Hyper& hy = c->hyper_of(c->sweep);
        const Hyper& prev = c->hyper_of(c->sweep - 1);
        // throughput mode: this sweep's hyperparameters already on the device and its normals
        // filled (both queued at the end of the previous sweep)
        const bool staged = c->pre.valid && c->pre.sweep == c->sweep && c->pre.staged;
        if (!staged && c->hyper_ahead) stage_hyper(prev);
        c->hyper_ahead = false;
        if (c->pre.valid && c->pre.sweep == c->sweep) {  // drawn at the end of the previous sweep
            std::swap(hy, c->pre.h);
            d0 = c->pre.d0;
        } else {
            HostStream hs;
            if (ref) {
                draw_hyper_variates(c->grand, c, hs);
            } else {
                PhiloxStream ps(cf.seed, c->sweep, 0);
                draw_hyper_variates(ps, c, hs);
            }
            prologue_gpu(c->sweep, prev);
            HIPCHK(hipStreamSynchronize(st));
            d0 = draw_hyper(c, prev, c->h_pre, hs, hy);
        }
        c->pre.valid = false;
        c->pre.staged = false;
        if (!staged) {
            stage_hyper(hy);
            if (ref && c->bias) {
                fill_bias_variates<T>(c, hy);
            } else if (ref) {  // user variates then item variates (:485 then :529)
                fill_z<T>(c, c->I, c->d_zU);
                fill_z<T>(c, c->J, c->d_zV);
            }
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipEventRecord(c->ev[1], st));
        }
        // ---- 3. user half-sweep (throughput mode: this half's normals first)
        if (!ref && !staged)
            HIPCHK(launch_philox_fill<T>(c->d_zU.as<T>(), K, c->users.r0, c->users.r1, cf.seed, c->sweep, TAG_USERS, st));
        if (c->bias)  // per-user bias hyperparameters + b_i draw + residual shift (:470-489, :515-530)
            HIPCHK(launch_bias_rows<T>(c->d_uptr.as<uint32_t>(), c->users.r0, c->users.r1, c->d_Eu.as<T>(),
                                       c->d_bu.as<double>(), c->d_mbu.as<double>(), c->d_sbu.as<double>(),
                                       ref ? c->d_var3u.as<double>() : nullptr, bias_args(c, hy, true, d0), st));
        // several ranks: each stage's fresh U (and b_i) blocks (one RCCL group), then its
        // residuals, while the next stage computes.  One rank: the half starts from the sweep's
        // start event when nothing was queued after it (staged start work, no bias pass)
        run_half_pipelined<T>(c, hy, true, [&](uint32_t p) {
            bcast_stage(c, c->users, p, c->d_U.p, c->Kp * sizeof(T));
            if (c->bias) bcast_stage(c, c->users, p, c->d_bu.p, sizeof(double));
        }, c->nranks == 1 && staged && !c->bias ? ev1(staged) : nullptr);
        if (c->nranks > 1) HIPCHK(hipEventRecord(c->ev[3], st));
        return Start{staged, c->launches - n0};
    }
    // ---- 4. item half-sweep
    void item_half(const Hyper& hy, bool staged) {
        if (!ref && !staged)
            HIPCHK(launch_philox_fill<T>(c->d_zV.as<T>(), K, c->items.r0, c->items.r1, cf.seed, c->sweep, TAG_ITEMS, st));
        if (c->bias)  // per-item (:492-511, :563-578)
            HIPCHK(launch_bias_rows<T>(c->d_vptr.as<uint32_t>(), c->items.r0, c->items.r1, c->d_Ev.as<T>(),
                                       c->d_bv.as<double>(), c->d_mbv.as<double>(), c->d_sbv.as<double>(),
                                       ref ? c->d_var3v.as<double>() : nullptr, bias_args(c, hy, false, 0.0), st));
        // fresh V (and b_j) blocks and the per-row sums (one RCCL group), then the residuals.  One
        // rank: the half starts from the user half's end event (ev[2], just recorded)
        run_half_pipelined<T>(c, hy, false, [&](uint32_t p) {
            bcast_stage(c, c->items, p, c->d_V.p, c->Kp * sizeof(T));
            if (c->bias) bcast_stage(c, c->items, p, c->d_bv.p, sizeof(double));
            bcast_stage(c, c->items, p, c->d_rowsq_v.p, sizeof(double));
            if (cf.eval_train) bcast_stage(c, c->items, p, c->d_rowtr_v.p, sizeof(double));
        }, c->nranks == 1 && staged && !c->bias ? c->ev[2] : nullptr);
        if (c->nranks > 1) HIPCHK(hipEventRecord(c->ev[5], st));
    }
    // The sweep's evaluation on stream `se`, with `hy` the sweep's own hyperparameters
    // (cfg.pipeline: the host may hold the next sweep's by the time this work runs)
    void evaluate(hipStream_t se, const Hyper& hy, bool collect, double div) {
        if (cf.eval_test && T_) {
            HIPCHK(launch_test<T>(c->d_tu.as<uint32_t>(), c->d_ti.as<uint32_t>(), c->d_tr.as<double>(), c->t0,
                                  c->t1, c->d_U.as<T>(), c->d_V.as<T>(), K, c->Kp, (T)c->lo, (T)c->hi,
                                  collect ? 1 : 0, div, c->d_tsum.as<double>(), c->d_tpart.as<double>(),
                                  c->bias ? c->d_bu.as<double>() : nullptr, c->d_bv.as<double>(), hy.b0, se));
            if (c->nranks > 1) c->comm->bcast_ranges(c->d_tpart.p, 2 * sizeof(double), c->tbblocks, se);
            const uint32_t nb = (uint32_t)((T_ + 255) / 256);
            HIPCHK(launch_sum_cols(c->d_tpart.as<double>(), nb, 2, d_res + RES_TEST_AVG, se));
        }
        if (cf.eval_train)
            HIPCHK(launch_sum(c->d_rowtr_v.as<double>(), c->J, d_res + RES_TRSQ, scratch + c->scratch_half, se));
        // the watch list's scores of this sample (only reads U, V and the biases, like the
        // test prediction, and shares its ordering against the next sweep's user half)
        if (c->watch.n && collect) {
            HIPCHK(hipEventRecord(c->wev[0], se));
            c->watch.accumulate<T>(c, c->d_U.as<T>(), c->bias ? c->d_bu.as<double>() : nullptr, c->d_bv.as<double>(),
                                   hy.b0, se);
            HIPCHK(hipEventRecord(c->wev[1], se));
        }
        // the sample store's copy of this sample (reads what the watch list reads)
        if (c->samples.cap && collect) c->samples.keep<T>(c, hy, se);
        // the fold-in list: every guest's row drawn from this sweep's V and the user half's
        // hyperparameters (the host's values: this sweep's, whatever d_hyper holds by now),
        // then, on a collected sweep, the guests' scores of this sample
        if (c->guests.n) {
            const size_t Kp = c->Kp;
            double* h = c->h_fhyp;
            HIPCHK(hipEventSynchronize(c->fev[0]));  // the previous copy out of the staging area
            std::fill(h, h + 2 * Kp, 0.0);
            std::copy(hy.sig_u.begin(), hy.sig_u.begin() + K, h);
            std::copy(hy.mu_u.begin(), hy.mu_u.begin() + K, h + Kp);
            HIPCHK(hipMemcpyAsync(c->d_fhyp.p, h, 2 * Kp * sizeof(double), hipMemcpyHostToDevice, se));
            HIPCHK(hipEventRecord(c->fev[0], se));
            HIPCHK(launch_foldin<T>(c->guests.n, c->fcsr.d_order.as<uint32_t>(), c->fcsr.d_ptr.as<uint32_t>(),
                                    c->fcsr.d_items.as<uint32_t>(), c->fcsr.d_ratings.as<double>(), c->d_fG.as<T>(),
                                    c->d_V.as<T>(), K, c->Kp, c->d_fhyp.as<double>(), hy.tau, c->sd_is_var, cf.seed,
                                    c->sweep, c->fcsr.d_E.as<double>(), se));
            HIPCHK(hipEventRecord(c->fev[1], se));
            c->fdrawn++;
            c->launches++;
            if (collect) {
                c->guests.accumulate<T>(c, c->d_fG.as<T>(), nullptr, nullptr, 0.0, se);
                HIPCHK(hipEventRecord(c->fev[2], se));
            }
        }
        HIPCHK(hipEventRecord(c->ev[6], se));
    }
    // ---- 5. evaluation, and (overlap) the next sweep's prologue kernels.  One rank: the
    // evaluation runs on the second stream beside the prologue kernels -- both only read
    // U and V and they write different result slots, so nothing changes -- where it used
    // to follow them (tune bit 28 restores that order; measured 7.64-7.73 -> 7.61 ms, r04s22).
    // Ends with the copy of the sweep's results.
    void evaluation(const Hyper& hy, bool collect, double div) {
        if (par_eval) {
            HIPCHK(hipStreamWaitEvent(c->sto, ev5, 0));
            evaluate(c->sto, hy, collect, div);
        }
        if (overlap) {  // the next sweep's prologue kernels, ahead of the evaluation
            prologue_gpu(c->sweep + 1, hy);
            HIPCHK(hipEventRecord(c->ev[7], st));  // the host draws from here on
            // and the next sweep's normals, both tables in one launch (Philox: a function of (seed,
            // sweep) only; this sweep's halves, which read them, are queued before)
            HIPCHK(launch_philox_fill2<T>(c->d_zU.as<T>(), c->users.r0, c->users.r1, TAG_USERS, c->d_zV.as<T>(),
                                          c->items.r0, c->items.r1, TAG_ITEMS, K, cf.seed, c->sweep + 1, st));
            HIPCHK(hipEventRecord(c->ev[8], st));  // the next sweep's start work ends here
        }
        if (par_eval)
            HIPCHK(hipStreamWaitEvent(st, c->ev[6], 0));
        else
            evaluate(st, hy, collect, div);
        // the results, with the split-row timeout flag in the same copy (one copy less per sweep;
        // the prologue's sums go to the host ahead of them, so the host draws while the
        // evaluation and the normals run: one copy of everything after them put the host round
        // trip on the path, ML-1M 0.40 -> 0.43 ms, r06s11)
        HIPCHK(hipMemcpyAsync(c->h_out(), d_res, 8 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(c->ev[9], st));  // this sweep's device work ends here
    }
    // (overlap) the next sweep's draws from the copied sums and this sweep's `hy`, into c->pre
    void draw_ahead(const Hyper& hy) {
        HIPCHK(hipEventSynchronize(c->ev[7]));
        HostStream hs;
        PhiloxStream ps(cf.seed, c->sweep + 1, 0);
        draw_hyper_variates(ps, c, hs);
        c->pre.d0 = draw_hyper(c, hy, c->h_pre, hs, c->pre.h);
        c->pre.sweep = c->sweep + 1;
        c->pre.valid = true;
        // the next sweep's hyperparameters to the device now (every launch of this sweep that
        // reads d_hyper -- the halves and the prologue's column statistics -- is queued before)
        stage_hyper(c->pre.h);
        c->pre.staged = true;
        c->hyper_ahead = true;
    }
    // ---- 6. the report's times of the start, the halves and the launch kinds: every event up
    // to the item half's end (the next sweep's start records them again)
    void report_times(sbmf_sweep_info& info, bool staged) {
        c->timing.ms_hyper = staged ? 0.0 : ev_ms(c->ev[0], ev1(staged));
        c->timing.ms_user_half = ev_ms(ev1(staged), c->ev[2]);
        c->timing.ms_item_half = ev_ms(ev3, c->ev[4]);
        c->timing.ms_comm = c->nranks > 1 ? ev_ms(c->ev[2], c->ev[3]) + ev_ms(c->ev[4], c->ev[5]) : 0.0;
        for (int sd = 0; sd < 2; ++sd) {
            const Side& sdd = sd == 0 ? c->users : c->items;
            for (int k = 0; k < SBMF_NKIND; ++k) {
                if (!c->time_kinds && k != KIND_STREAM) continue;  // kept from the run's first sweep
                double ms = 0.0;
                for (uint32_t p = 0; p < c->nstages; ++p) {
                    const Side::Stage& g = *sdd.stg[p];
                    const bool ran = k < NBIN && !g.bin_rows[k].empty();
                    const int kp = ran ? c->kpv(p, sd, k) : -1;
                    if (ran) ms += ev_ms(kp >= 0 ? c->kev(p, sd, kp, 1) : c->kbg(p, sd, k), c->kev(p, sd, k, 1));
                }
                c->timing.kern_ms[sd][k] = ms;
            }
        }
        info.ms_sweep = ev_ms(c->ev[0], ev5);
    }
    // ---- 6. the report's results, once the sweep's copy of them (ev[9]) is done
    void report_results(sbmf_sweep_info& info) {
        const double* res8 = c->h_out();
        std::copy(res8, res8 + 8, c->h_res.begin());
        uint32_t split_timeout;
        std::memcpy(&split_timeout, res8 + RES_TIMEOUT, sizeof(split_timeout));
        if (c->kprof) kprof_report(c, info.sweep);
        if (split_timeout)  // a bounded spin in k_gres gave up: the sweep's results are not valid
            fail(SBMF_E_STATE, "sweep %u: split-row hand-off timed out (workgroups not co-resident)", info.sweep);
        info.rmse_avg = (cf.eval_test && T_) ? std::sqrt(c->h_res[RES_TEST_AVG] / T_) : NAN;
        info.rmse_this = (cf.eval_test && T_) ? std::sqrt(c->h_res[RES_TEST_THIS] / T_) : NAN;
        info.rmse_train = cf.eval_train && N ? std::sqrt(c->h_res[RES_TRSQ] / N) : NAN;
        // with the overlap the next sweep's start work -- the prologue's kernels and both
        // tables' normals -- runs between ev[5] and ev[8], counted here
        c->timing.ms_hyper += overlap ? ev_ms(ev5, c->ev[8]) : 0.0;
        c->timing.ms_eval = overlap && !par_eval ? ev_ms(c->ev[8], c->ev[6]) : ev_ms(ev5, c->ev[6]);
        info.ms_eval = c->timing.ms_eval;
    }

    void run(uint32_t nsweeps, sbmf_sweep_cb cb, void* user) {
        // cfg.pipeline (throughput mode): sweep s+1's start is queued before sweep s is reported, so
        // the device does not idle through the host's per-sweep work (the report, the callback, the
        // next sweep's enqueue).  A stop the callback asks for then takes effect after sweep s+1.
        bool queued = false, stop_after = false;
        Start start{};
        for (uint32_t it = 0; it < nsweeps; ++it) {
            if (!queued) start = start_sweep(it == 0);
            queued = false;
            const Hyper& hy = c->hyper_of(c->sweep);
            const uint32_t n1 = c->launches;  // this sweep's launches: its start's and those from here on
            const bool collect = q2 ? true : (c->sweep >= cf.burnin);
            if (collect) c->collected++;
            const double div = avg_collected(cf) ? (double)std::max(1u, c->collected) : (double)(c->sweep + 1);
            // The sweep's device work, from the item half to the results' copy (with the overlap the
            // next sweep's prologue kernels and normals are part of it).  (Captured once as a hipGraph
            // and replayed, one rank: ML-1M K=50 0.45 -> 0.77-0.90 ms, ML-20M 7.11 -> 7.57-7.82 ms
            // per sweep, r06s3 -- the halves unchanged, the replay slower than the eager launches;
            // removed, profiles/r06/ab/r06s3_sweep_graph.patch)
            item_half(hy, start.staged);
            evaluation(hy, collect, div);
            if (overlap) draw_ahead(hy);  // while the evaluation runs
            // ---- 6. the report.  With the overlap the host is past ev[7]: every event up to the item
            // half's end is done, so the half and launch-kind times are read first; cfg.pipeline then
            // queues the next sweep's start (which records those events again) before the host waits
            // for this sweep's results (ev[9]) and runs the callback
            if (!overlap) HIPCHK(hipEventSynchronize(c->ev[9]));
            sbmf_sweep_info info{};
            info.acc_train = info.acc_avg = info.acc_this = info.ll_this = NAN;  // regression
            info.sweep = c->sweep;
            info.collected = collect ? 1u : 0u;
            info.tau = hy.tau;
            report_times(info, start.staged);
            c->timing.n_launch = start.n_launch + (c->launches - n1);
            c->sweep++;
            if (overlap && cf.pipeline && it + 1 < nsweeps && !c->kprof && !stop_after) {
                start = start_sweep(false);
                queued = true;
            }
            if (overlap) HIPCHK(hipEventSynchronize(c->ev[9]));  // this sweep's results (not the upload after them)
            report_results(info);
            c->reported = (int)(info.sweep & 1);  // the getters describe this sweep from here on
            if (cb && cb(&info, user)) {
                if (!queued) break;
                stop_after = true;  // the next sweep's start is queued: it completes, then the run stops
            } else if (stop_after) {
                break;
            }
        }
    }
};

template <typename T>
void run_sweeps_T(sbmf_ctx* c, uint32_t nsweeps, sbmf_sweep_cb cb, void* user) {
    SweepRun<T>{c}.run(nsweeps, cb, user);
}
template void run_sweeps_T<float>(sbmf_ctx*, uint32_t, sbmf_sweep_cb, void*);
template void run_sweeps_T<double>(sbmf_ctx*, uint32_t, sbmf_sweep_cb, void*);
template void run_half<float>(sbmf_ctx*, const Hyper&, bool, uint32_t, hipEvent_t);
template void run_half<double>(sbmf_ctx*, const Hyper&, bool, uint32_t, hipEvent_t);

}  // namespace sbmf
