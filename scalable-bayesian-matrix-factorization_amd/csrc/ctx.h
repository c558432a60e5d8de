// ctx.h -- what the host runtime's files (prepare.cpp, sweep.cpp, lists.cpp, samples.cpp,
// samples_file.cpp, sbmf.cpp) share: the row layout of one orientation, the hyperparameter state, the
// score lists, the sample store and the context (lists.h: what the lists and the store share).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sbmf.h"
#include "comm.h"
#include "common.h"
#include <rccl/rccl.h>
#include "kernels.h"
#include "rng.h"
#include "fmc.h"
#include "fmm.h"
#include "fmg.h"
#include "fmq.h"
#include "foldin.h"
#include "lists.h"
#include "recommend.h"
#include "samples.h"
#include "samples_foldin.h"
#include "vbo.h"
#include "vb_lists.h"

struct sbmf_ctx;

namespace sbmf {

// ------------------------------------------------------------------ host layout
// One orientation: users (CSR by user, partner = item) or items (CSC).
static const int NBIN = GK_NUM + 1;  // row bins: Gram-block kinds GK_* (0..4), streaming rows (5)

struct Side {
    uint32_t R = 0;                     // rows
    std::vector<uint32_t> ptr;          // [R+1]
    std::vector<uint32_t> part;         // [N] partner id
    std::vector<uint32_t> perm;         // [N] position in the other orientation
    std::vector<double> r;              // [N] ratings
    uint32_t r0 = 0, r1 = 0;            // owned row range (multi-GPU)
    std::vector<uint64_t> bounds;       // [nranks+1] row ranges of every rank
    // streaming rows (k_gres): set 0 and set 1 (f64 items: rows above 1024 ratings,
    // on 16-wave workgroups) -- see prepare_T
    struct StreamSet {
        std::vector<SplitTask> stasks;  // tasks, in rounds of `sgrid` slots
        std::vector<SplitRow> xrows;    // rows split over several tasks
        uint32_t nxchunk = 0;           // tasks belonging to split rows (slab / staging slots)
        uint32_t sgrid = 0;             // persistent grid of the launch
        uint32_t cmax = 0;              // task capacity (ratings)
        uint32_t tune = 0;              // kernel variant bits of the launch
    };
    // A stage: the rows [r0, r1) of this rank's block, binned for their own launches.
    // One stage per half unless the multi-GPU exchange is pipelined: then the block is
    // cut into nnz-balanced stages and stage s's fresh rows and residuals travel while
    // stage s+1 computes (run_sweeps_T).  Results do not depend on the cut: every row's
    // draws are the same in any launch.
    struct Stage {
        uint32_t r0 = 0, r1 = 0;
        std::vector<uint32_t> bin_rows[NBIN];  // kinds: GK_* (0..4), KIND_STREAM (5)
        StreamSet ss[2];
        std::vector<std::array<uint32_t, 3>> gsub[GK_NUM];  // multi-wave bins: (waves, offset, count) sub-ranges
        DBuf d_bins[NBIN], d_stasks[2], d_xrows[2];
        // multi-GPU residual exchange of this stage: [peer] segments of the send / receive areas
        std::vector<size_t> soff, scnt, roff, rcnt;
        size_t rbeg = 0, rend = 0;  // this stage's receive elements [rbeg, rend)
    };
    std::vector<std::unique_ptr<Stage>> stg;
    std::vector<std::vector<uint64_t>> sbounds;  // [rank][stage + 1]: every rank's stage cuts
    std::vector<ResidTask> rtasks;   // residual recompute: own rows in chunks of <= RESID_CHUNK
    std::vector<uint32_t> rtptr;     // [r1-r0+1] first task of each own row
    // multi-GPU residual exchange (see build_exchange): where this rank's rows
    // scatter their residuals (the other orientation's position, or a send slot
    // past its end), and where the residuals other ranks send land
    std::vector<uint32_t> perm2, unpack;
    size_t nsend = 0, nrecv = 0;
};

static const int KIND_STREAM = GK_NUM;  // 5: streaming kernel (row bin: every streaming row)

}  // namespace sbmf

using namespace sbmf;

// One sweep's hyperparameters (fp64 host copy): the noise precision, the biased sampler's (quirks
// BIAS2 / BIAS22) global bias with its Normal-Gamma state, the factors' precisions and means
struct Hyper {
    double tau = 1.0, b0 = 0.0, mu_b0 = 0.0, sig_b0 = 0.0;
    std::vector<double> sig_u, mu_u, sig_v, mu_v;
};

// A score list: for each of n rows of a factor table (watched users; fold-in guests) the running
// first / second moments of its scores against every item, [n][Jp] doubles each, added to after
// every collected sweep and read back as mean / spread or a top-N selection (recommend.hip).
// The libFM learner's query list (fmq.h) keeps the same sums over the candidates' block rows: the
// columns are the list's own count J, not the context's items.
// Nothing here exists while no list is registered (n == 0).
struct ScoreList {
    const char* what;      // "watch list" / "fold-in list" / "query list" in messages
    const char* reg;       // the registering entry point
    uint32_t n = 0, J = 0, Jp = 0;  // rows, columns, columns rounded up to 16
    uint32_t count = 0;    // sweeps accumulated since the list was registered
    int clamp = 0;         // flags bit 0: scores clamped like the test prediction
    bool latest = false;   // the sums hold one sample, the latest (ALS): the spread reads back as exactly 0
    DBuf d_ids, d_S1, d_S2;  // the rows' indices in their table (the watched users, or 0..n-1); the sums
    Span sel;  // the last selection
    void alloc(uint32_t n_, uint32_t J_, int clamp_, hipStream_t st);  // sums zeroed; d_ids is the caller's to fill
    void drop();
    template <typename T>
    void accumulate(sbmf_ctx* c, const T* rows, const double* bu, const double* bv, double b0, hipStream_t se);
    void scores(sbmf_ctx* c, const char* fn, uint32_t row, double* mean, double* stdev);
    void recommend(sbmf_ctx* c, const uint32_t* csr_ptr, const uint32_t* csr_items, uint32_t topn, uint32_t flags,
                   double risk, uint32_t* items, double* mean, double* stdev);
};

// The posterior sample store (sbmf_keep_samples, samples.cpp): a ring of `cap` slots on the device,
// each a copy of U [I][Kp] and V [J][Kp] in the context's precision and, with the biased sampler,
// of bu [I] and bv [J]; b0 and the sweep index of every slot stay on the host.  The oldest sample
// is in slot `head`; every `every`-th collected sweep since registration is kept (`seen` counts
// them), the newest overwriting the oldest once the ring is full.  Beside b0 the host keeps, by
// slot, the hyperparameters the sweep's halves used -- [sig_u | mu_u | sig_v | mu_v] and tau, 4 K + 1
// doubles -- which a guest's draw at that sample needs (sbmf_samples_foldin_*); has_hyper is
// cleared by sbmf_load_samples, whose file does not hold them, and set by
// sbmf_load_samples_hyper.  Nothing here exists while no store is registered (cap == 0).
struct SampleStore {
    uint32_t cap = 0, every = 1, head = 0, count = 0, seen = 0;
    size_t bytes = 0;  // device bytes of the slots
    DBuf d_U, d_V, d_bu, d_bv;
    std::vector<double> b0;       // [cap], by slot
    std::vector<uint32_t> sweep;  // [cap], by slot
    std::vector<double> hyper;    // [cap][4 K + 1], by slot: sbmf_get_hyper's block, then tau
    bool has_hyper = false;       // every kept sample's entry of `hyper` is its sweep's
    Span cev, scv, sel;  // the last copy, scoring and selection
    Span gdr, gsc, gse;  // the last guest call (sbmf_samples_foldin_*): its draw, scoring and selection
    // test hook (sbmf_test_samples_tune): the temporaries' budget in bytes (0: the default) and
    // the per-sample loop of launch_watch_accum in the fused kernel's place; and the guests' draw
    // by the one fused launch in place of the default, one launch per sample and scan
    uint64_t budget = 0;
    bool unfused = false, fused_draw = false;
    uint32_t slot(uint32_t s) const { return (head + s) % cap; }  // of the s-th oldest sample
    void alloc(sbmf_ctx* c, uint32_t cap_, uint32_t every_);
    void drop();
    template <typename T>
    void keep(sbmf_ctx* c, const Hyper& hy, hipStream_t se);  // this sweep's tables into the next slot, if it is one to keep
};

// The online VB learner's lists (sbmf_vb_*, vb_lists.cpp): nothing is kept between calls but the
// user-side CSR of the train set (the rated-item masks; built at the first call that needs it)
// and the event pairs of the last transpose, scoring, selection and guest launch.  Nothing here
// exists before the first call.
struct VBLists {
    DBuf d_uptr, d_upart;
    bool csr = false, spans = false;
    Span tr, sc, sel, gu;
    uint64_t budget = 0;  // test hook (sbmf_test_vb_tune): the temporaries' budget in bytes (0: the default)
    void drop() {
        d_uptr.release();
        d_upart.release();
        for (Span* s : {&tr, &sc, &sel, &gu}) s->destroy();
        csr = spans = false;
    }
};

struct sbmf_ctx {
    sbmf_ctx() { sbmf::audit().contexts++; }
    sbmf_config cfg{};
    std::string err;
    // sbmf_test_rccl_selftest ran extra item halves on this chain (it is no longer
    // the sampler's): sweeps are refused.  dead: the self-test timed out with RCCL
    // work still queued; sbmf_destroy then leaks the context instead of waiting.
    bool spent = false, dead = false;
    // host data
    std::vector<uint32_t> tu, ti, su, si;
    std::vector<double> tr, sr;
    uint32_t I = 0, J = 0, I_req = 0, J_req = 0;
    bool prepared = false;
    // derived settings
    double init_sd = 1.0, lo = 1.0, hi = 5.0;
    int sd_is_var = 1;
    uint32_t K = 0, Kp = 0;
    // layout
    Side users, items;
    uint64_t t0 = 0, t1 = 0;  // owned test range
    std::vector<uint64_t> tbounds, tbblocks;  // every rank's test range (ratings, 256-blocks)
    std::vector<uint64_t> tperm;  // device test order (user order) -> file order
    // hyper state: sweep s's in slot s & 1, so the sweep in flight (cfg.pipeline: sweep s+1,
    // started before sweep s's callback) leaves the reported one's alone.  `reported` is the
    // slot of the last sweep whose callback has started: what sbmf_get_hyper and
    // sbmf_get_biases' b0 return
    Hyper hyp[2];
    int reported = 0;
    Hyper& hyper_of(uint32_t sw) { return hyp[sw & 1]; }
    bool bias = false;  // biased sampler (quirks BIAS2 / BIAS22)
    // reference mode: host shadow (b, mu_b, sigma_b) of the rows without train
    // ratings, whose bias walk depends only on its own variates (see fill_bias_variates)
    std::vector<uint32_t> empty_u, empty_v;
    std::vector<std::array<double, 3>> shadow_u, shadow_v;
    uint32_t sweep = 0, collected = 0;
    // rng
    GlibcRand grand{1};
    // multi-GPU
    int nranks = 1, rank = 0;
    Comm own_comm;            // this context's communicator (sbmf_comm_init) ...
    Comm* comm = &own_comm;   // ... or a process-wide one it borrows (sbmf_comm_attach)
    // device
    hipStream_t st = nullptr;
    hipEvent_t ev[10] = {};
    std::vector<hipEvent_t> kevs;  // [stage][side][kind][begin, end] launch timing
    hipEvent_t& kev(uint32_t stage, int side, int kind, int e) {
        return kevs[(((size_t)stage * 2 + side) * SBMF_NKIND + kind) * 2 + e];
    }
    // [stage][side][kind]: the kind launched just before this one on the same stream, whose
    // end event is this kind's start (no begin event recorded), or -1.  Two timing events
    // back to back on a stream cost ~12 us of idle device between the launches (r04f trace).
    std::vector<int8_t> kprev;
    int8_t& kpv(uint32_t stage, int side, int kind) { return kprev[((size_t)stage * 2 + side) * SBMF_NKIND + kind]; }
    // [stage][side][kind]: the begin event a kind's time is read from when kprev is -1 -- its own
    // kev(.., 0), or an event its half's caller had just recorded on the compute stream (the
    // sweep start, the user half's end), which then also forks the side streams
    std::vector<hipEvent_t> kbegin;
    hipEvent_t& kbg(uint32_t stage, int side, int kind) { return kbegin[((size_t)stage * 2 + side) * SBMF_NKIND + kind]; }
    uint32_t nstages = 1;          // stages per half (see Side::Stage); > 1 only with several ranks
    hipStream_t stc = nullptr;     // multi-GPU: the exchange of stage p runs here while stage p+1 computes
    std::vector<hipEvent_t> sev;   // [side][stage]: stage computed (compute stream)
    // sbmf_test_virtual_rank (timing only): one rank of an nranks-rank run on this GPU,
    // every exchange skipped; tsev [side][stage + 1] times its stages on the compute stream
    bool virt = false;
    std::vector<hipEvent_t> tsev;
    hipEvent_t cev[2] = {};        // [side]: the half's exchange done (comm stream)
    hipStream_t sto = nullptr;     // a half's Gram-block launches, beside its streaming launch
    hipStream_t sto2 = nullptr;    // tune bit 25: half of them on a second side stream
    hipEvent_t oev[4] = {};        // [fork, join] of those launches, [2]: stream set 0 done, [3]: sto2 join
    DBuf d_uptr, d_upart, d_uperm, d_ur, d_vptr, d_vpart, d_vperm, d_vr;
    DBuf d_U, d_V, d_Eu, d_Ev, d_zU, d_zV, d_hyper;
    DBuf d_rowsq_u, d_rowtr_u, d_rowsq_v, d_rowtr_v;
    DBuf d_colpart, d_res, d_scratch;
    size_t scratch_half = 0;  // doubles: d_scratch + scratch_half is the evaluation's

    bool kprof = false; // SBMF_KPROF=1: streaming-kernel phase cycles printed per sweep
    int kprof_set = 0;  // SBMF_KPROF_SET: which streaming launch of a half is stamped (0: the 8-wave one)
    DBuf d_kprof;
    DBuf d_rtasks, d_rtptr, d_rtsq;  // residual recompute (item side)
    DBuf d_xslabs, d_xcnt, d_xchunk_sq, d_xchunk_tr, d_xnewown;
    // The streaming row kernels' cold argument blocks (GresCold, kernels.h), one slot of
    // kColdSlot bytes per (stage, side, launch shape: stream set 0, set 1, k_grow), with the host's
    // copy of what the device holds: a block is uploaded when it differs from that copy (the
    // first half-sweep after set_data or a configuration change), never per half otherwise.
    static constexpr size_t kColdSlot = 256;
    DBuf d_gcold;
    std::vector<unsigned char> h_gcold;
    bool time_kinds = true;   // this sweep records every launch kind's events (else the streaming kind's only)
    size_t xset_nx = 1;  // set 0's split chunks: set 1's areas follow them
    DBuf d_tu, d_ti, d_tr, d_tsum, d_tpart;
    DBuf d_uperm2, d_vperm2, d_uunpack, d_vunpack, d_xrecv;  // multi-GPU residual exchange
    DBuf d_bu, d_bv, d_mbu, d_mbv, d_sbu, d_sbv;  // biases b_i / b_j and their per-row (mu, sigma)
    DBuf d_var3u, d_var3v, d_epart;              // reference-mode per-row bias variates; sum(E) partials
    std::vector<double> h_res;
    double* h_pre = nullptr;     // pinned: the prologue's sums (residual, column statistics)
    // pinned: the sweep's results (8 doubles), the split-row timeout flag, and the staged
    // hyperparameter upload [sig_u | mu_u | sig_v | mu_v] (4 Kp of T)
    void* h_io = nullptr;
    double* h_out() { return static_cast<double*>(h_io); }
    void* h_hyper() { return static_cast<char*>(h_io) + 128; }
    hipEvent_t hev = nullptr;  // the last upload from h_hyper done (the area is rewritten after it)
    // throughput mode: the next sweep's hyperparameters, drawn at the end of the
    // previous sweep while its test evaluation runs (run_sweeps_T)
    struct PreDraw {
        bool valid = false;
        bool staged = false;  // uploaded to d_hyper, and the sweep's normals filled, ahead
        uint32_t sweep = 0;
        double d0 = 0;
        Hyper h;
    } pre;
    // d_hyper holds the drawn-ahead values (pre), not the current ones: a sweep that does not
    // use them (pre dropped by sbmf_set_factors) restores the current ones before its
    // prologue, whose column statistics read the current mu from d_hyper
    bool hyper_ahead = false;
    double* h_pinned = nullptr;  // pinned staging for z streams
    size_t h_pinned_bytes = 0, h_pre_bytes = 0, h_io_bytes = 0;
    sbmf_timing timing{};
    uint32_t launches = 0;  // kernel launches of the sampler so far: a sweep's timing.n_launch is a difference
    // Watch list (sbmf_watch_users): the watched users' scores, from U and the biases
    ScoreList watch{"watch list", "sbmf_watch_users"};
    hipEvent_t wev[2] = {};  // the last scoring launch [begin, end] (recorded once watch.count > 0)
    // Fold-in list (sbmf_foldin_users): guests given by their ratings (fcsr: the CSR on the device),
    // their factor rows G [n + 2][Kp] in the tables' type (row n zero, row n + 1 slack: the
    // tables' layout, so the watch list's scoring kernel reads it as a U), drawn after every
    // sweep's item half (foldin.hip), and the moments of their scores as the watch
    // list keeps them.  d_fhyp is the list's own [sig_u | mu_u] (2 Kp doubles) of the sweep
    // being evaluated: d_hyper may already hold the next sweep's (stage_hyper).  guests.d_ids is
    // 0..n-1 (the scoring kernel's user list; fcsr.d_ids stays empty), fcsr.d_order the guests by
    // falling length.  Nothing here exists while no list is registered.
    ScoreList guests{"fold-in list", "sbmf_foldin_users"};
    uint32_t fdrawn = 0;   // sweeps drawn since the list was registered (guests.count: the collected ones)
    GuestCSR fcsr;
    DBuf d_fG, d_fhyp;
    double* h_fhyp = nullptr;  // pinned staging of d_fhyp
    size_t h_fhyp_bytes = 0;
    // hyper copy done = draw begin, draw end = scoring begin (recorded once fdrawn > 0), scoring
    // end (once guests.count > 0)
    hipEvent_t fev[3] = {};
    // Query list of the libFM learner (sbmf_fm_query_cases): the sums over the candidates' block
    // rows (fmq.d_ids is 0..n-1), and what the learner reads and writes each iteration (fmq.h; fm->query
    // points at it while a list is registered).  Nothing here exists while no list is registered.
    ScoreList fmq{"query list", "sbmf_fm_query_cases"};
    FMQueryList fmqd;
    SampleStore samples;
    VBLearner* vb = nullptr;  // -method vb (vbo.cpp)
    VBLists vbl;
    // -method mcmc --order libfm / als: libFM's chain (fmc.cpp) on triples (fmm.cpp) or on cases
    // with any number of features (fmg.cpp).  ctr / cte: the host copies of sbmf_set_train_cases /
    // sbmf_set_test_cases (or, with SBMF_FMM_GENERAL=1, the triples of sbmf_set_train restated
    // as cases; the model then still reads back by user / item)
    FMChain* fm = nullptr;
    FMGroups fmgroups;  // sbmf_set_attr_groups / sbmf_set_group_regular, read at sbmf_prepare
    std::vector<FMRelation> fmrels;  // sbmf_add_relation, in the order given, read at sbmf_prepare
    struct HostCases {
        std::vector<uint64_t> ptr;
        std::vector<uint32_t> attr;
        std::vector<float> x, y;
        uint32_t num_attr = 0;
        bool set = false;
        sbmf_cases view() {
            sbmf_cases c{};
            c.n = y.size();
            c.nnz = attr.size();
            c.num_attr = num_attr;
            c.ptr = ptr.data();
            c.attr = attr.data();
            c.x = x.data();
            c.target = y.data();
            return c;
        }
    } ctr, cte;
    ~sbmf_ctx();
};

// Every entry point's body sits between these: an exception becomes the return code
#define API_BEGIN try {
#define API_END(ctx) } catch (...) { return sbmf::api_error(ctx); } return SBMF_OK;

namespace sbmf {

// what the runtime's files use of each other (the templates: instantiated for float and double)
int api_error(sbmf_ctx* ctx);
// the sample store (samples.cpp), for its files (samples_file.cpp): in scope, a sample kept, its
// queued copies done; the device bytes of one slot
void samples_ready(sbmf_ctx* c, const char* fn);
size_t slot_bytes(const sbmf_ctx* c);
void partition_bounds(const uint32_t* ptr, uint32_t R, int nranks, uint64_t* bounds);
template <typename T>
void prepare_T(sbmf_ctx* c);
template <typename T>
void run_half(sbmf_ctx* c, const Hyper& hy, bool users, uint32_t stage, hipEvent_t start = nullptr);
template <typename T>
void run_sweeps_T(sbmf_ctx* c, uint32_t nsweeps, sbmf_sweep_cb cb, void* user);

// d_res slots; RES_TIMEOUT holds k_gres's split-row timeout flag (a uint32, sticky), so the
// sweep's one result copy carries it
enum { RES_ESQ = 0, RES_TRSQ = 1, RES_TEST_AVG = 2, RES_TEST_THIS = 3, RES_ES = 4, RES_ESQ2 = 5, RES_TIMEOUT = 7, RES_COL = 8 };

static size_t tsize(const sbmf_ctx* c) { return c->cfg.precision == SBMF_F32 ? 4 : 8; }

// running-mean divisor: collected sweeps (average 1, or quirks none by default) or sweep + 1
static bool avg_collected(const sbmf_config& cf) {
    return cf.average == 1 || (cf.average == 0 && cf.quirks == SBMF_QUIRKS_NONE);
}

template <typename T>
static std::vector<T> to_T(const std::vector<double>& v) {
    return std::vector<T>(v.begin(), v.end());
}

// table [R][Kp] (T) from row-major doubles [R][K]
template <typename T>
static void upload_table(sbmf_ctx* c, DBuf& d, const double* src, uint32_t R) {
    std::vector<T> h((size_t)R * c->Kp, T(0));
    for (uint32_t r = 0; r < R; ++r)
        for (uint32_t k = 0; k < c->K; ++k) h[(size_t)r * c->Kp + k] = (T)src[(size_t)r * c->K + k];
    HIPCHK(hipMemcpy(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
}
template <typename T>
static void download_table(sbmf_ctx* c, const DBuf& d, double* dst, uint32_t R) {
    std::vector<T> h((size_t)R * c->Kp);
    HIPCHK(hipMemcpy(h.data(), d.p, h.size() * sizeof(T), hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < R; ++r)
        for (uint32_t k = 0; k < c->K; ++k) dst[(size_t)r * c->K + k] = (double)h[(size_t)r * c->Kp + k];
}
// both, for a table in the context's precision
static void upload_table(sbmf_ctx* c, DBuf& d, const double* src, uint32_t R) {
    c->cfg.precision == SBMF_F32 ? upload_table<float>(c, d, src, R) : upload_table<double>(c, d, src, R);
}
static void download_table(sbmf_ctx* c, const DBuf& d, double* dst, uint32_t R) {
    c->cfg.precision == SBMF_F32 ? download_table<float>(c, d, dst, R) : download_table<double>(c, d, dst, R);
}

static void ensure_pinned(sbmf_ctx* c, size_t bytes) {
    if (c->h_pinned_bytes >= bytes) return;
    pinned_free(c->h_pinned, c->h_pinned_bytes);
    c->h_pinned_bytes = 0;
    pinned_alloc((void**)&c->h_pinned, bytes);
    c->h_pinned_bytes = bytes;
}

}  // namespace sbmf
