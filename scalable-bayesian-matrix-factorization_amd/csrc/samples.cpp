// samples.cpp -- the posterior sample store (SampleStore, ctx.h) and its entry points: keeping
// thinned samples of the SBPMF chain on the device (sbmf_keep_samples; the copy runs in the sweep's
// evaluation, sweep.cpp), scoring users and pairs from them after the run (samples.hip), and the
// sample file (sbmf_save_samples / sbmf_load_samples / sbmf_samples_file_info); the
// samples' hyperparameters, their companion file, and guests drawn from the stored samples after the
// run (sbmf_samples_foldin_*; samples_foldin.hip).
#include <sys/stat.h>

#include "ctx.h"

namespace {

// ------------------------------------------------------------------ the file
// Little-endian throughout (the only byte order this library is built for).
constexpr char kMagic[8] = {'S', 'B', 'M', 'F', 'S', 'M', 'P', '\n'};
constexpr uint32_t kVersion = 1;
struct FileHeader {  // 40 bytes
    char magic[8];
    uint32_t version, precision, I, J, K, count, bias, reserved;
};
static_assert(sizeof(FileHeader) == 40, "the sample file's header is 40 bytes");

struct File {
    FILE* f = nullptr;
    ~File() {
        if (f) std::fclose(f);
    }
};

uint64_t sample_bytes(const FileHeader& h) {
    const uint64_t ts = h.precision == SBMF_F32 ? 4 : 8;
    return ((uint64_t)h.I + h.J) * h.K * ts + (h.bias ? (1 + (uint64_t)h.I + h.J) * 8 : 0);
}
uint64_t file_bytes(const FileHeader& h) { return sizeof(FileHeader) + (uint64_t)h.count * 4 + (uint64_t)h.count * sample_bytes(h); }

// opens `path`, reads and validates the header against the file's size; the stream is left
// behind the header
void open_sample_file(const char* fn, const char* path, File& file, FileHeader& h) {
    file.f = std::fopen(path, "rb");
    struct stat sb;
    if (!file.f || fstat(fileno(file.f), &sb) != 0) sbmf::fail(SBMF_E_IO, "%s: cannot open %s", fn, path);
    const uint64_t size = (uint64_t)sb.st_size;
    if (size < sizeof(FileHeader) || std::fread(&h, sizeof(FileHeader), 1, file.f) != 1)
        sbmf::fail(SBMF_E_IO, "%s: %s is truncated in its header: %llu bytes, a sample file's header has %zu", fn, path,
                   (unsigned long long)size, sizeof(FileHeader));
    if (std::memcmp(h.magic, kMagic, sizeof kMagic) != 0)
        sbmf::fail(SBMF_E_IO, "%s: %s is not a sample file (bad magic)", fn, path);
    if (h.version != kVersion)
        sbmf::fail(SBMF_E_IO, "%s: %s has the unknown format version %u; this build reads version %u", fn, path, h.version,
                   kVersion);
    if (h.precision > SBMF_F32 || h.bias > 1 || h.K == 0 || h.K > 256 || h.count > 65535)
        sbmf::fail(SBMF_E_IO, "%s: %s has a bad header (precision %u, bias %u, K %u, count %u)", fn, path, h.precision,
                   h.bias, h.K, h.count);
    const uint64_t want = file_bytes(h);
    if (size < want)
        sbmf::fail(SBMF_E_IO, "%s: %s is truncated in its body: %llu bytes, its header implies %llu", fn, path,
                   (unsigned long long)size, (unsigned long long)want);
    if (size > want)
        sbmf::fail(SBMF_E_IO, "%s: %s has %llu trailing bytes: %llu bytes, its header implies %llu", fn, path,
                   (unsigned long long)(size - want), (unsigned long long)size, (unsigned long long)want);
}

// ------------------------------------------------------------------ scope and state
// The contexts the store covers; everything else is SBMF_E_STATE (as list_scope, lists.cpp).
void samples_scope(const sbmf_ctx* c, const char* fn) {
    if (c->cfg.method != SBMF_METHOD_MCMC)
        sbmf::fail(SBMF_E_STATE, "%s: the sample store is offered by the SBPMF sampler (SBMF_METHOD_MCMC) only; this "
                                 "context runs the %s learner", fn,
                   c->cfg.method == SBMF_METHOD_VB ? "online VB" : c->cfg.method == SBMF_METHOD_ALS ? "ALS" : "libFM MCMC");
    if (c->virt) sbmf::fail(SBMF_E_STATE, "%s: a virtual rank's numbers are not a chain; no sample store there", fn);
    if (c->nranks > 1 || c->comm->active() || c->comm != &c->own_comm)
        sbmf::fail(SBMF_E_STATE, "%s: the sample store runs on one rank; this context joined a communicator", fn);
    if (!c->prepared) sbmf::fail(SBMF_E_STATE, "%s: not prepared (sbmf_prepare)", fn);
}
// the store's queued copies are done (they run on the evaluation's stream)
void samples_sync(sbmf_ctx* c) {
    HIPCHK(hipSetDevice(c->cfg.device));
    HIPCHK(hipStreamSynchronize(c->sto));
    HIPCHK(hipStreamSynchronize(c->st));
}
void samples_ready(sbmf_ctx* c, const char* fn) {
    samples_scope(c, fn);
    if (!c->samples.cap || !c->samples.count)
        sbmf::fail(SBMF_E_STATE, "%s: no sample kept yet (sbmf_keep_samples, then a collected sweep; or sbmf_load_samples)", fn);
    samples_sync(c);
}
size_t slot_bytes(const sbmf_ctx* c) {
    return ((size_t)c->I + c->J) * c->Kp * sbmf::tsize(c) + (c->bias ? ((size_t)c->I + c->J) * sizeof(double) : 0);
}

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

// one stored sample's tables and biases, without padding, as the store holds them
template <typename T>
void download_slot(sbmf_ctx* c, uint32_t p, std::vector<T>& U, std::vector<T>& V, std::vector<double>& bu,
                   std::vector<double>& bv) {
    const SampleStore& ss = c->samples;
    const size_t I = c->I, J = c->J, K = c->K, Kp = c->Kp;
    std::vector<T> h((I > J ? I : J) * Kp);
    auto table = [&](const sbmf::DBuf& d, size_t R, std::vector<T>& out) {
        HIPCHK(hipMemcpy(h.data(), d.as<T>() + (size_t)p * R * Kp, R * Kp * sizeof(T), hipMemcpyDeviceToHost));
        out.resize(R * K);
        for (size_t r = 0; r < R; ++r) std::copy(h.begin() + r * Kp, h.begin() + r * Kp + K, out.begin() + r * K);
    };
    table(ss.d_U, I, U);
    table(ss.d_V, J, V);
    if (c->bias) {
        bu.resize(I);
        bv.resize(J);
        HIPCHK(hipMemcpy(bu.data(), ss.d_bu.as<double>() + (size_t)p * I, I * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(bv.data(), ss.d_bv.as<double>() + (size_t)p * J, J * sizeof(double), hipMemcpyDeviceToHost));
    }
}

template <typename T>
void save_T(sbmf_ctx* c, FILE* f, const char* path) {
    const SampleStore& ss = c->samples;
    std::vector<T> U, V;
    std::vector<double> bu, bv;
    for (uint32_t s = 0; s < ss.count; ++s) {
        const uint32_t p = ss.slot(s);
        download_slot<T>(c, p, U, V, bu, bv);
        bool ok = std::fwrite(U.data(), sizeof(T), U.size(), f) == U.size() &&
                  std::fwrite(V.data(), sizeof(T), V.size(), f) == V.size();
        if (ok && c->bias)
            ok = std::fwrite(&ss.b0[p], sizeof(double), 1, f) == 1 && std::fwrite(bu.data(), sizeof(double), bu.size(), f) == bu.size() &&
                 std::fwrite(bv.data(), sizeof(double), bv.size(), f) == bv.size();
        if (!ok) sbmf::fail(SBMF_E_IO, "sbmf_save_samples: writing %s failed", path);
    }
}

template <typename T>
void load_T(sbmf_ctx* c, FILE* f, const char* path, uint32_t count) {
    SampleStore& ss = c->samples;
    const size_t I = c->I, J = c->J, K = c->K, Kp = c->Kp;
    std::vector<T> packed((I > J ? I : J) * K), h((I > J ? I : J) * Kp, T(0));
    std::vector<double> b(I > J ? I : J);
    auto rd = [&](void* dst, size_t size, size_t cnt) {
        if (std::fread(dst, size, cnt, f) != cnt) sbmf::fail(SBMF_E_IO, "sbmf_load_samples: reading %s failed", path);
    };
    for (uint32_t s = 0; s < count; ++s) {
        auto table = [&](sbmf::DBuf& d, size_t R) {
            rd(packed.data(), sizeof(T), R * K);
            for (size_t r = 0; r < R; ++r) std::copy(packed.begin() + r * K, packed.begin() + (r + 1) * K, h.begin() + r * Kp);
            HIPCHK(hipMemcpy(d.as<T>() + (size_t)s * R * Kp, h.data(), R * Kp * sizeof(T), hipMemcpyHostToDevice));
        };
        table(ss.d_U, I);
        table(ss.d_V, J);
        if (c->bias) {
            rd(&ss.b0[s], sizeof(double), 1);
            rd(b.data(), sizeof(double), I);
            HIPCHK(hipMemcpy(ss.d_bu.as<double>() + (size_t)s * I, b.data(), I * sizeof(double), hipMemcpyHostToDevice));
            rd(b.data(), sizeof(double), J);
            HIPCHK(hipMemcpy(ss.d_bv.as<double>() + (size_t)s * J, b.data(), J * sizeof(double), hipMemcpyHostToDevice));
        }
    }
}

// the temporaries' budget of sbmf_samples_recommend: S1 and S2 of one slice of users
constexpr uint64_t kBudget = 1ull << 30;

// ------------------------------------------------------------------ the hyperparameters' file
constexpr char kHyperMagic[8] = {'S', 'B', 'M', 'F', 'S', 'H', 'P', '\n'};
constexpr uint32_t kHyperVersion = 1;
struct HyperHeader {  // 24 bytes
    char magic[8];
    uint32_t version, K, count, reserved;
};
static_assert(sizeof(HyperHeader) == 24, "the companion file's header is 24 bytes");
uint64_t hyper_file_bytes(const HyperHeader& h) {
    return sizeof(HyperHeader) + (uint64_t)h.count * 4 + (uint64_t)h.count * (4 * (uint64_t)h.K + 1) * 8;
}
// open_sample_file for the companion file
void open_hyper_file(const char* fn, const char* path, File& file, HyperHeader& h) {
    file.f = std::fopen(path, "rb");
    struct stat sb;
    if (!file.f || fstat(fileno(file.f), &sb) != 0) sbmf::fail(SBMF_E_IO, "%s: cannot open %s", fn, path);
    const uint64_t size = (uint64_t)sb.st_size;
    if (size < sizeof(HyperHeader) || std::fread(&h, sizeof(HyperHeader), 1, file.f) != 1)
        sbmf::fail(SBMF_E_IO, "%s: %s is truncated in its header: %llu bytes, a sample hyperparameter file's header has %zu",
                   fn, path, (unsigned long long)size, sizeof(HyperHeader));
    if (std::memcmp(h.magic, kHyperMagic, sizeof kHyperMagic) != 0)
        sbmf::fail(SBMF_E_IO, "%s: %s is not a sample hyperparameter file (bad magic)", fn, path);
    if (h.version != kHyperVersion)
        sbmf::fail(SBMF_E_IO, "%s: %s has the unknown format version %u; this build reads version %u", fn, path, h.version,
                   kHyperVersion);
    if (h.K == 0 || h.K > 256 || h.count > 65535 || h.reserved != 0)
        sbmf::fail(SBMF_E_IO, "%s: %s has a bad header (K %u, count %u, reserved %u)", fn, path, h.K, h.count, h.reserved);
    const uint64_t want = hyper_file_bytes(h);
    if (size < want)
        sbmf::fail(SBMF_E_IO, "%s: %s is truncated in its body: %llu bytes, its header implies %llu", fn, path,
                   (unsigned long long)size, (unsigned long long)want);
    if (size > want)
        sbmf::fail(SBMF_E_IO, "%s: %s has %llu trailing bytes: %llu bytes, its header implies %llu", fn, path,
                   (unsigned long long)(size - want), (unsigned long long)size, (unsigned long long)want);
}

// ------------------------------------------------------------------ guests from the stored samples
// What the three guest calls check before anything is allocated.
void guests_ready(sbmf_ctx* c, const char* fn, uint32_t n, const uint32_t* ptr, const uint32_t* items, const double* ratings,
                  uint32_t scans) {
    samples_scope(c, fn);
    if (c->bias)
        sbmf::fail(SBMF_E_STATE, "%s: guests are folded into a store of the unbiased quirk sets (final, sbpmf2, none); a "
                                 "guest bias would need a draw of its own", fn);
    if (scans < 1 || scans > sbmf::SAMPLES_FOLDIN_SCANS_MAX)
        sbmf::fail(SBMF_E_ARG, "%s: scans %u is not in 1..%u", fn, scans, sbmf::SAMPLES_FOLDIN_SCANS_MAX);
    if (n && !ptr) sbmf::fail(SBMF_E_ARG, "%s: null ptr with n > 0", fn);
    if (n >= 0xfffffffeu) sbmf::fail(SBMF_E_ARG, "%s: %u guests are too many", fn, n);
    for (uint32_t g = 0; g < n; ++g)
        if (ptr[g + 1] < ptr[g]) sbmf::fail(SBMF_E_ARG, "%s: ptr decreases at guest %u (%u then %u)", fn, g, ptr[g], ptr[g + 1]);
    const uint32_t p0 = n ? ptr[0] : 0, nnz = n ? ptr[n] - p0 : 0;
    if (nnz && (!items || !ratings)) sbmf::fail(SBMF_E_ARG, "%s: null items / ratings with ratings listed", fn);
    for (uint32_t q = 0; q < nnz; ++q)
        if (items[p0 + q] >= c->J)
            sbmf::fail(SBMF_E_ARG, "%s: items[%u] = %u is not below the %u items", fn, p0 + q, items[p0 + q], c->J);
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
    sbmf::DBuf d_ptr, d_items, d_ratings, d_order, d_ident, d_E, d_hyp, d_tau, d_sw, d_GS, d_S1, d_S2, d_b0;
    std::vector<uint32_t> hp;  // the CSR's ptr, from 0
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
            const uint32_t p0 = ptr[0];
            hp.resize(n + 1);
            for (uint32_t g = 0; g <= n; ++g) hp[g] = ptr[g] - p0;  // the device CSR starts at 0
            std::vector<uint32_t> ident(n), sw(count);
            std::iota(ident.begin(), ident.end(), 0u);
            // within each slice the launch ends with its longest row: those start first
            std::vector<uint32_t> order(ident);
            for (uint32_t off = 0; off < n; off += rows)
                std::stable_sort(order.begin() + off, order.begin() + std::min(n, off + rows),
                                 [&](uint32_t x, uint32_t y) { return hp[x + 1] - hp[x] > hp[y + 1] - hp[y]; });
            // the samples' [sig_u | mu_u], tau and sweep index, oldest first
            std::vector<double> hyp((size_t)count * 2 * Kp, 0.0), tau(count);
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
            d_E.alloc((size_t)nnz * sizeof(double));
            d_items.alloc((size_t)nnz * sizeof(uint32_t));
            d_ratings.alloc((size_t)nnz * sizeof(double));
            sbmf::upload(d_ptr, hp, st);
            sbmf::upload(d_order, order, st);
            sbmf::upload(d_ident, ident, st);
            sbmf::upload(d_hyp, hyp, st);
            sbmf::upload(d_tau, tau, st);
            sbmf::upload(d_sw, sw, st);
            if (nnz) {
                HIPCHK(hipMemcpyAsync(d_items.p, items + p0, (size_t)nnz * sizeof(uint32_t), hipMemcpyHostToDevice, st));
                HIPCHK(hipMemcpyAsync(d_ratings.p, ratings + p0, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, st));
            }
            a.sv = view_of(c, d_b0, st);
            HIPCHK(hipStreamSynchronize(st));  // the vectors are locals
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
        a.ptr = d_ptr.as<uint32_t>();
        a.items = d_items.as<uint32_t>();
        a.ratings = d_ratings.as<double>();
        a.K = K;
        a.Kp = Kp;
        a.hyper = d_hyp.as<double>();
        a.tau = d_tau.as<double>();
        a.sweeps = d_sw.as<uint32_t>();
        a.scans = scans;
        a.sd_is_var = c->sd_is_var;
        a.seed = c->cfg.seed;
        a.E = d_E.as<double>();
    }

    // the rows of the guests off .. off + m - 1 at every sample into GS (events: ss.gdr)
    template <typename T>
    void draw_T(uint32_t off, uint32_t m) {
        SampleStore& ss = c->samples;
        hipStream_t st = c->st;
        a.n = m;
        a.g0 = off;
        a.order = d_order.as<uint32_t>() + off;
        HIPCHK(hipMemsetAsync(d_GS.p, 0, d_GS.bytes, st));
        HIPCHK(hipEventRecord(ss.gdr[0], st));
        if (ss.fused_draw) {
            HIPCHK(sbmf::launch_samples_foldin<T>(a, st));
        } else {  // the memset above zeroed the carry too
            double* carry = reinterpret_cast<double*>(static_cast<char*>(d_GS.p) + (size_t)ss.count * gs * sizeof(T));
            for (uint32_t s = 0; s < ss.count; ++s)
                for (uint32_t r = 0; r < scans; ++r) HIPCHK(sbmf::launch_samples_foldin_step<T>(a, s, r, carry, st));
        }
        HIPCHK(hipEventRecord(ss.gdr[1], st));
        ss.timed_gdraw = true;
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
        HIPCHK(hipEventRecord(ss.gsc[0], c->st));
        score_rows(c, v, d_ident.as<uint32_t>(), m, clamp, d_S1.as<double>(), d_S2.as<double>(), c->st);
        HIPCHK(hipEventRecord(ss.gsc[1], c->st));
        ss.timed_gscore = true;
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
    for (hipEvent_t* e : {cev, scv, sel, gdr, gsc, gse}) {
        sbmf::event_create(&e[0]);
        sbmf::event_create(&e[1]);
    }
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
    for (hipEvent_t* e : {cev, scv, sel, gdr, gsc, gse}) {
        sbmf::event_destroy(e[0]);
        sbmf::event_destroy(e[1]);
    }
    b0.clear();
    sweep.clear();
    hyper.clear();
    has_hyper = false;
    cap = head = count = seen = 0;
    every = 1;
    bytes = 0;
    timed_copy = timed_score = timed_select = false;
    timed_gdraw = timed_gscore = timed_gselect = false;
}
// (the caller has checked that the sweep is a collected one)
template <typename T>
void SampleStore::keep(sbmf_ctx* c, const Hyper& hy, hipStream_t se) {
    if (seen++ % every) return;
    const uint32_t p = count < cap ? slot(count) : head;  // the next free slot, or the oldest sample's
    const size_t I = c->I, J = c->J, Kp = c->Kp;
    HIPCHK(hipEventRecord(cev[0], se));
    HIPCHK(hipMemcpyAsync(d_U.as<T>() + p * I * Kp, c->d_U.p, I * Kp * sizeof(T), hipMemcpyDeviceToDevice, se));
    HIPCHK(hipMemcpyAsync(d_V.as<T>() + p * J * Kp, c->d_V.p, J * Kp * sizeof(T), hipMemcpyDeviceToDevice, se));
    if (c->bias) {
        HIPCHK(hipMemcpyAsync(d_bu.as<double>() + p * I, c->d_bu.p, I * sizeof(double), hipMemcpyDeviceToDevice, se));
        HIPCHK(hipMemcpyAsync(d_bv.as<double>() + p * J, c->d_bv.p, J * sizeof(double), hipMemcpyDeviceToDevice, se));
    }
    HIPCHK(hipEventRecord(cev[1], se));
    timed_copy = true;
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
    samples_scope(ctx, "sbmf_keep_samples");
    if (every == 0) sbmf::fail(SBMF_E_ARG, "sbmf_keep_samples: every = 0 (1 keeps every collected sweep)");
    if (cap > 65535) sbmf::fail(SBMF_E_ARG, "sbmf_keep_samples: cap %u is above 65535", cap);
    samples_sync(ctx);
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
    samples_scope(ctx, "sbmf_samples_info");
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
    samples_scope(ctx, fn);
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
    const uint32_t J = ctx->J, Jp = sbmf::watch_jp(J), Jw = sbmf::watch_jw(J);
    const bool exclude = !(flags & 1u);
    const int clamp = (flags & 2u) ? 1 : 0;
    // users per slice: as many as the budget's two sums hold, in whole workgroups of 64, one at least
    const uint64_t budget = ss.budget ? ss.budget : kBudget;
    const uint64_t fit = budget / ((uint64_t)2 * Jp * sizeof(double)) / 64 * 64;
    const uint32_t rows = (uint32_t)std::min<uint64_t>(n, std::max<uint64_t>(fit, 64));
    sbmf::DBuf d_b0, d_ids, d_S1, d_S2, d_it, d_ms, d_mask;
    const sbmf::SampleView v = view_of(ctx, d_b0, st);
    const size_t slots = (size_t)rows * topn;
    d_ids.alloc((size_t)rows * sizeof(uint32_t));
    d_S1.alloc((size_t)rows * Jp * sizeof(double));
    d_S2.alloc((size_t)rows * Jp * sizeof(double));
    d_it.alloc(slots * sizeof(uint32_t));
    d_ms.alloc(2 * slots * sizeof(double));
    if (exclude) d_mask.alloc((size_t)rows * Jw * sizeof(uint32_t));
    for (uint32_t off = 0; off < n; off += rows) {
        const uint32_t m = std::min(rows, n - off);
        const size_t ms = (size_t)m * topn, o = (size_t)off * topn;
        HIPCHK(hipMemcpyAsync(d_ids.p, users + off, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(ss.scv[0], st));
        score_rows(ctx, v, d_ids.as<uint32_t>(), m, clamp, d_S1.as<double>(), d_S2.as<double>(), st);
        HIPCHK(hipEventRecord(ss.scv[1], st));
        HIPCHK(hipEventRecord(ss.sel[0], st));
        if (exclude) {
            HIPCHK(hipMemsetAsync(d_mask.p, 0, (size_t)m * Jw * sizeof(uint32_t), st));
            HIPCHK(sbmf::launch_watch_mask(d_ids.as<uint32_t>(), m, ctx->d_uptr.as<uint32_t>(), ctx->d_upart.as<uint32_t>(),
                                           d_mask.as<uint32_t>(), Jw, st));
        }
        HIPCHK(sbmf::launch_watch_select(m, d_S1.as<double>(), d_S2.as<double>(), J, (double)ss.count, risk,
                                         exclude ? d_mask.as<uint32_t>() : nullptr, topn, d_it.as<uint32_t>(),
                                         d_ms.as<double>(), d_ms.as<double>() + ms, st));
        HIPCHK(hipEventRecord(ss.sel[1], st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(items + o, d_it.p, ms * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(mean + o, d_ms.p, ms * sizeof(double), hipMemcpyDeviceToHost));
        if (stdev) HIPCHK(hipMemcpy(stdev + o, d_ms.as<double>() + ms, ms * sizeof(double), hipMemcpyDeviceToHost));
    }
    ss.timed_score = ss.timed_select = true;
    API_END(ctx)
}

int sbmf_samples_scores(sbmf_ctx* ctx, uint32_t user, uint32_t flags, double* mean, double* stdev) {
    API_BEGIN
    const char* fn = "sbmf_samples_scores";
    if (!ctx || !mean) sbmf::fail(SBMF_E_ARG, "null argument");
    samples_scope(ctx, fn);
    if (flags & ~2u) sbmf::fail(SBMF_E_ARG, "%s: unknown flags 0x%x (bit 1 = clamp)", fn, flags & ~2u);
    check_users(ctx, fn, 1, &user);
    samples_ready(ctx, fn);
    SampleStore& ss = ctx->samples;
    hipStream_t st = ctx->st;
    const uint32_t J = ctx->J, Jp = sbmf::watch_jp(J);
    sbmf::DBuf d_b0, d_id, d_S, d_out;
    const sbmf::SampleView v = view_of(ctx, d_b0, st);
    d_id.alloc(sizeof(uint32_t));
    d_S.alloc((size_t)2 * Jp * sizeof(double));
    d_out.alloc((size_t)2 * J * sizeof(double));
    double *S = d_S.as<double>(), *d = d_out.as<double>();
    HIPCHK(hipMemcpyAsync(d_id.p, &user, sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(ss.scv[0], st));
    score_rows(ctx, v, d_id.as<uint32_t>(), 1, (flags & 2u) ? 1 : 0, S, S + Jp, st);
    HIPCHK(hipEventRecord(ss.scv[1], st));
    ss.timed_score = true;
    HIPCHK(sbmf::launch_watch_moments(S, S + Jp, J, (double)ss.count, d, d + J, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(mean, d, (size_t)J * sizeof(double), hipMemcpyDeviceToHost));
    if (stdev) HIPCHK(hipMemcpy(stdev, d + J, (size_t)J * sizeof(double), hipMemcpyDeviceToHost));
    API_END(ctx)
}

int sbmf_samples_predict(sbmf_ctx* ctx, uint64_t n, const uint32_t* users, const uint32_t* items, uint32_t flags,
                         double* mean, double* stdev) {
    API_BEGIN
    const char* fn = "sbmf_samples_predict";
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    samples_scope(ctx, fn);
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
    samples_scope(ctx, "sbmf_samples_timing");
    SampleStore& ss = ctx->samples;
    if (!ss.cap) sbmf::fail(SBMF_E_STATE, "sbmf_samples_timing: no sample store registered (sbmf_keep_samples)");
    samples_sync(ctx);
    if (ms_copy) *ms_copy = ss.timed_copy ? sbmf::ev_ms(ss.cev[0], ss.cev[1]) : 0.0;
    if (ms_score) *ms_score = ss.timed_score ? sbmf::ev_ms(ss.scv[0], ss.scv[1]) : 0.0;
    if (ms_select) *ms_select = ss.timed_select ? sbmf::ev_ms(ss.sel[0], ss.sel[1]) : 0.0;
    API_END(ctx)
}

int sbmf_save_samples(sbmf_ctx* ctx, const char* path) {
    API_BEGIN
    if (!ctx || !path) sbmf::fail(SBMF_E_ARG, "null argument");
    samples_ready(ctx, "sbmf_save_samples");
    const SampleStore& ss = ctx->samples;
    FileHeader h{};
    std::memcpy(h.magic, kMagic, sizeof kMagic);
    h.version = kVersion;
    h.precision = (uint32_t)ctx->cfg.precision;
    h.I = ctx->I;
    h.J = ctx->J;
    h.K = ctx->K;
    h.count = ss.count;
    h.bias = ctx->bias ? 1u : 0u;
    File file;
    file.f = std::fopen(path, "wb");
    if (!file.f) sbmf::fail(SBMF_E_IO, "sbmf_save_samples: cannot open %s for writing", path);
    std::vector<uint32_t> sweeps(ss.count);
    for (uint32_t s = 0; s < ss.count; ++s) sweeps[s] = ss.sweep[ss.slot(s)];
    if (std::fwrite(&h, sizeof h, 1, file.f) != 1 || std::fwrite(sweeps.data(), 4, sweeps.size(), file.f) != sweeps.size())
        sbmf::fail(SBMF_E_IO, "sbmf_save_samples: writing %s failed", path);
    ctx->cfg.precision == SBMF_F32 ? save_T<float>(ctx, file.f, path) : save_T<double>(ctx, file.f, path);
    const int rc = std::fclose(file.f);
    file.f = nullptr;
    if (rc != 0) sbmf::fail(SBMF_E_IO, "sbmf_save_samples: writing %s failed", path);
    API_END(ctx)
}

int sbmf_load_samples(sbmf_ctx* ctx, const char* path) {
    API_BEGIN
    const char* fn = "sbmf_load_samples";
    if (!ctx || !path) sbmf::fail(SBMF_E_ARG, "null argument");
    samples_scope(ctx, fn);
    File file;
    FileHeader h;
    open_sample_file(fn, path, file, h);
    static const char* const prec[] = {"f64", "f32"};
    if (h.precision != (uint32_t)ctx->cfg.precision)
        sbmf::fail(SBMF_E_ARG, "%s: %s holds precision %s; this context computes in %s", fn, path, prec[h.precision],
                   prec[ctx->cfg.precision]);
    if (h.I != ctx->I) sbmf::fail(SBMF_E_ARG, "%s: %s holds num_users = %u; this context has %u", fn, path, h.I, ctx->I);
    if (h.J != ctx->J) sbmf::fail(SBMF_E_ARG, "%s: %s holds num_items = %u; this context has %u", fn, path, h.J, ctx->J);
    if (h.K != ctx->K) sbmf::fail(SBMF_E_ARG, "%s: %s holds num_factor K = %u; this context has K = %u", fn, path, h.K, ctx->K);
    if (h.bias != (ctx->bias ? 1u : 0u))
        sbmf::fail(SBMF_E_ARG, "%s: %s holds bias = %u (%s biases); this context's quirk set is %s", fn, path, h.bias,
                   h.bias ? "with" : "without", ctx->bias ? "biased (bias = 1)" : "unbiased (bias = 0)");
    if (h.count == 0) sbmf::fail(SBMF_E_ARG, "%s: %s holds no sample", fn, path);
    samples_sync(ctx);
    SampleStore& ss = ctx->samples;
    if (ss.cap < h.count) {
        const uint32_t every = ss.every;
        ss.drop();
        try {
            ss.alloc(ctx, h.count, every);
        } catch (const sbmf::Error& e) {
            ss.drop();
            if (e.code == SBMF_E_NOMEM)
                sbmf::fail(SBMF_E_NOMEM, "%s: %u samples of %zu bytes need %zu bytes of device memory: %s", fn, h.count,
                           slot_bytes(ctx), (size_t)h.count * slot_bytes(ctx), e.msg.c_str());
            throw;
        }
    }
    ss.head = ss.count = ss.seen = 0;
    ss.has_hyper = false;  // the file holds none (sbmf_load_samples_hyper)
    std::vector<uint32_t> sweeps(h.count);
    if (std::fread(sweeps.data(), 4, h.count, file.f) != h.count) sbmf::fail(SBMF_E_IO, "%s: reading %s failed", fn, path);
    std::copy(sweeps.begin(), sweeps.end(), ss.sweep.begin());
    ctx->cfg.precision == SBMF_F32 ? load_T<float>(ctx, file.f, path, h.count) : load_T<double>(ctx, file.f, path, h.count);
    ss.count = h.count;
    API_END(ctx)
}

int sbmf_samples_file_info(const char* path, uint32_t* version, uint32_t* precision, uint32_t* num_users,
                           uint32_t* num_items, uint32_t* num_factor, uint32_t* count, uint32_t* bias, uint64_t* bytes) {
    sbmf_ctx* ctx = nullptr;
    API_BEGIN
    if (!path) sbmf::fail(SBMF_E_ARG, "null path");
    File file;
    FileHeader h;
    open_sample_file("sbmf_samples_file_info", path, file, h);
    if (version) *version = h.version;
    if (precision) *precision = h.precision;
    if (num_users) *num_users = h.I;
    if (num_items) *num_items = h.J;
    if (num_factor) *num_factor = h.K;
    if (count) *count = h.count;
    if (bias) *bias = h.bias;
    if (bytes) *bytes = file_bytes(h);
    API_END(ctx)
}

// --- the samples' hyperparameters and their file ------------------------------------------------
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

int sbmf_save_samples_hyper(sbmf_ctx* ctx, const char* path) {
    API_BEGIN
    const char* fn = "sbmf_save_samples_hyper";
    if (!ctx || !path) sbmf::fail(SBMF_E_ARG, "null argument");
    samples_ready(ctx, fn);
    const SampleStore& ss = ctx->samples;
    if (!ss.has_hyper) sbmf::fail(SBMF_E_STATE, "%s: the stored samples have no hyperparameters to save", fn);
    HyperHeader h{};
    std::memcpy(h.magic, kHyperMagic, sizeof kHyperMagic);
    h.version = kHyperVersion;
    h.K = ctx->K;
    h.count = ss.count;
    File file;
    file.f = std::fopen(path, "wb");
    if (!file.f) sbmf::fail(SBMF_E_IO, "%s: cannot open %s for writing", fn, path);
    const size_t per = 4 * (size_t)ctx->K + 1;
    std::vector<uint32_t> sweeps(ss.count);
    std::vector<double> body(ss.count * per);
    for (uint32_t s = 0; s < ss.count; ++s) {
        const uint32_t p = ss.slot(s);
        sweeps[s] = ss.sweep[p];
        std::copy(ss.hyper.begin() + p * per, ss.hyper.begin() + (p + 1) * per, body.begin() + s * per);
    }
    bool ok = std::fwrite(&h, sizeof h, 1, file.f) == 1 && std::fwrite(sweeps.data(), 4, sweeps.size(), file.f) == sweeps.size() &&
              std::fwrite(body.data(), 8, body.size(), file.f) == body.size();
    const int rc = std::fclose(file.f);
    file.f = nullptr;
    if (!ok || rc != 0) sbmf::fail(SBMF_E_IO, "%s: writing %s failed", fn, path);
    API_END(ctx)
}

int sbmf_load_samples_hyper(sbmf_ctx* ctx, const char* path) {
    API_BEGIN
    const char* fn = "sbmf_load_samples_hyper";
    if (!ctx || !path) sbmf::fail(SBMF_E_ARG, "null argument");
    samples_scope(ctx, fn);
    File file;
    HyperHeader h;
    open_hyper_file(fn, path, file, h);
    samples_ready(ctx, fn);
    SampleStore& ss = ctx->samples;
    if (h.K != ctx->K) sbmf::fail(SBMF_E_ARG, "%s: %s holds num_factor K = %u; this context has K = %u", fn, path, h.K, ctx->K);
    if (h.count != ss.count) sbmf::fail(SBMF_E_ARG, "%s: %s holds count = %u samples; the store holds %u", fn, path, h.count, ss.count);
    const size_t per = 4 * (size_t)ctx->K + 1;
    std::vector<uint32_t> sweeps(h.count);
    std::vector<double> body(h.count * per);
    if (std::fread(sweeps.data(), 4, sweeps.size(), file.f) != sweeps.size() ||
        std::fread(body.data(), 8, body.size(), file.f) != body.size())
        sbmf::fail(SBMF_E_IO, "%s: reading %s failed", fn, path);
    for (uint32_t s = 0; s < h.count; ++s)
        if (sweeps[s] != ss.sweep[ss.slot(s)])
            sbmf::fail(SBMF_E_ARG, "%s: %s holds sweep index %u for sample %u; the store's sample %u is sweep %u", fn, path,
                       sweeps[s], s, s, ss.sweep[ss.slot(s)]);
    for (uint32_t s = 0; s < h.count; ++s)
        std::copy(body.begin() + s * per, body.begin() + (s + 1) * per, ss.hyper.begin() + ss.slot(s) * per);
    ss.has_hyper = true;
    API_END(ctx)
}

int sbmf_samples_hyper_file_info(const char* path, uint32_t* version, uint32_t* num_factor, uint32_t* count, uint64_t* bytes) {
    sbmf_ctx* ctx = nullptr;
    API_BEGIN
    if (!path) sbmf::fail(SBMF_E_ARG, "null path");
    File file;
    HyperHeader h;
    open_hyper_file("sbmf_samples_hyper_file_info", path, file, h);
    if (version) *version = h.version;
    if (num_factor) *num_factor = h.K;
    if (count) *count = h.count;
    if (bytes) *bytes = hyper_file_bytes(h);
    API_END(ctx)
}

// --- guests from the stored samples -----------------------------------------------------------
int sbmf_samples_foldin_recommend(sbmf_ctx* ctx, uint32_t n, const uint32_t* ptr, const uint32_t* items,
                                  const double* ratings, uint32_t scans, uint32_t topn, uint32_t flags, double risk,
                                  uint32_t* out_items, double* mean, double* stdev) {
    API_BEGIN
    const char* fn = "sbmf_samples_foldin_recommend";
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    samples_scope(ctx, fn);
    if (n && (!out_items || !mean)) sbmf::fail(SBMF_E_ARG, "%s: null argument", fn);
    if (topn < 1 || topn > 1024) sbmf::fail(SBMF_E_ARG, "%s: topn %u is not in 1..1024", fn, topn);
    if (flags & ~3u)
        sbmf::fail(SBMF_E_ARG, "%s: unknown flags 0x%x (bit 0 = keep the guest's own items, bit 1 = clamp)", fn, flags & ~3u);
    if (!(risk == risk)) sbmf::fail(SBMF_E_ARG, "%s: risk is NaN", fn);
    guests_ready(ctx, fn, n, ptr, items, ratings, scans);
    if (n == 0) return SBMF_OK;
    SampleStore& ss = ctx->samples;
    hipStream_t st = ctx->st;
    const uint32_t J = ctx->J, Jw = sbmf::watch_jw(J);
    const bool exclude = !(flags & 1u);
    GuestCall gc(ctx, fn, n, ptr, items, ratings, scans, true);
    const uint32_t rows = gc.rows;
    const size_t slots = (size_t)rows * topn;
    sbmf::DBuf d_it, d_ms, d_mask;
    try {
        d_it.alloc(slots * sizeof(uint32_t));
        d_ms.alloc(2 * slots * sizeof(double));
        if (exclude) d_mask.alloc((size_t)rows * Jw * sizeof(uint32_t));
    } catch (const sbmf::Error& e) {
        if (e.code == SBMF_E_NOMEM)
            sbmf::fail(SBMF_E_NOMEM, "%s: the selection of %u guests needs %zu bytes of device memory: %s", fn, rows,
                       slots * (sizeof(uint32_t) + 2 * sizeof(double)) + (exclude ? (size_t)rows * Jw * sizeof(uint32_t) : 0),
                       e.msg.c_str());
        throw;
    }
    for (uint32_t off = 0; off < n; off += rows) {
        const uint32_t m = std::min(rows, n - off);
        const size_t ms = (size_t)m * topn, o = (size_t)off * topn;
        gc.draw(off, m);
        gc.score(m, (flags & 2u) ? 1 : 0);
        HIPCHK(hipEventRecord(ss.gse[0], st));
        if (exclude) {  // "rated": the guest's own items (the guest CSR in the user-side CSR's place)
            HIPCHK(hipMemsetAsync(d_mask.p, 0, (size_t)m * Jw * sizeof(uint32_t), st));
            HIPCHK(sbmf::launch_watch_mask(gc.d_ident.as<uint32_t>() + off, m, gc.d_ptr.as<uint32_t>(), gc.d_items.as<uint32_t>(),
                                           d_mask.as<uint32_t>(), Jw, st));
        }
        HIPCHK(sbmf::launch_watch_select(m, gc.d_S1.as<double>(), gc.d_S2.as<double>(), J, (double)ss.count, risk,
                                         exclude ? d_mask.as<uint32_t>() : nullptr, topn, d_it.as<uint32_t>(),
                                         d_ms.as<double>(), d_ms.as<double>() + ms, st));
        HIPCHK(hipEventRecord(ss.gse[1], st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(out_items + o, d_it.p, ms * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(mean + o, d_ms.p, ms * sizeof(double), hipMemcpyDeviceToHost));
        if (stdev) HIPCHK(hipMemcpy(stdev + o, d_ms.as<double>() + ms, ms * sizeof(double), hipMemcpyDeviceToHost));
    }
    ss.timed_gselect = true;
    API_END(ctx)
}

int sbmf_samples_foldin_rows(sbmf_ctx* ctx, uint32_t n, const uint32_t* ptr, const uint32_t* items, const double* ratings,
                             uint32_t scans, double* rows) {
    API_BEGIN
    const char* fn = "sbmf_samples_foldin_rows";
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    samples_scope(ctx, fn);
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
    samples_scope(ctx, fn);
    if (flags & ~2u) sbmf::fail(SBMF_E_ARG, "%s: unknown flags 0x%x (bit 1 = clamp)", fn, flags & ~2u);
    const uint32_t ptr[2] = {0, len};
    guests_ready(ctx, fn, 1, ptr, items, ratings, scans);
    const SampleStore& ss = ctx->samples;
    hipStream_t st = ctx->st;
    const uint32_t J = ctx->J;
    GuestCall gc(ctx, fn, 1, ptr, items, ratings, scans, true);
    sbmf::DBuf d_out;
    d_out.alloc((size_t)2 * J * sizeof(double));
    double* d = d_out.as<double>();
    gc.draw(0, 1);
    gc.score(1, (flags & 2u) ? 1 : 0);
    HIPCHK(sbmf::launch_watch_moments(gc.d_S1.as<double>(), gc.d_S2.as<double>(), J, (double)ss.count, d, d + J, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(mean, d, (size_t)J * sizeof(double), hipMemcpyDeviceToHost));
    if (stdev) HIPCHK(hipMemcpy(stdev, d + J, (size_t)J * sizeof(double), hipMemcpyDeviceToHost));
    API_END(ctx)
}

int sbmf_samples_foldin_timing(sbmf_ctx* ctx, double* ms_draw, double* ms_score, double* ms_select) {
    API_BEGIN
    if (!ctx) sbmf::fail(SBMF_E_ARG, "null context");
    samples_scope(ctx, "sbmf_samples_foldin_timing");
    SampleStore& ss = ctx->samples;
    if (!ss.cap) sbmf::fail(SBMF_E_STATE, "sbmf_samples_foldin_timing: no sample store registered (sbmf_keep_samples)");
    samples_sync(ctx);
    if (ms_draw) *ms_draw = ss.timed_gdraw ? sbmf::ev_ms(ss.gdr[0], ss.gdr[1]) : 0.0;
    if (ms_score) *ms_score = ss.timed_gscore ? sbmf::ev_ms(ss.gsc[0], ss.gsc[1]) : 0.0;
    if (ms_select) *ms_select = ss.timed_gselect ? sbmf::ev_ms(ss.gse[0], ss.gse[1]) : 0.0;
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
