// prepare.cpp -- sbmf_prepare for the sampler: the row layout of both orientations, the rank and
// stage partition, the row bins and streaming tasks, and every device buffer of a context.
#include "ctx.h"

namespace sbmf {

// Multi-GPU residuals.  A half-sweep on rank p updates the residuals of its
// own rows' ratings and scatters them into the other orientation's order
// (E_other[perm[idx]]); the next half on rank q reads the residuals of q's
// rows, which every rank contributed to.  So each half ends with a
// point-to-point exchange: rank p's kernels write the residuals bound for
// rank q into a send area past the end of E_other (perm2 = N + slot), in
// rating order, and rank q unpacks what arrives from p into its positions
// (unpack, the same order).  Both lists follow from the rating structure,
// which every rank holds, so no index travels.  About N / P residuals per
// rank per half cross xGMI -- instead of recomputing every residual from
// r - own.partner, which re-reads every partner row.
static void build_exchange(Side& s, const Side& other, int nranks, int rank) {
    const uint64_t N = s.perm.size();
    const size_t P = s.stg.size();
    std::vector<uint64_t> obase(nranks + 1);
    for (int k = 0; k <= nranks; ++k) obase[k] = other.ptr[other.bounds[k]];
    auto owner = [&](uint32_t pos) {
        return (int)(std::upper_bound(obase.begin(), obase.end(), (uint64_t)pos) - obase.begin()) - 1;
    };
    // send area: [stage][peer] segments, each in rating order
    size_t off = 0;
    for (size_t p = 0; p < P; ++p) {
        Side::Stage& g = *s.stg[p];
        g.scnt.assign(nranks, 0);
        for (uint64_t idx = s.ptr[g.r0]; idx < s.ptr[g.r1]; ++idx) {
            const int q = owner(s.perm[idx]);
            if (q != rank) g.scnt[q]++;
        }
        g.soff.assign(nranks, 0);
        for (int k = 0; k < nranks; ++k) {
            g.soff[k] = off;
            off += g.scnt[k];
        }
    }
    s.nsend = off;
    s.perm2.assign(s.perm.begin(), s.perm.end());
    for (size_t p = 0; p < P; ++p) {
        Side::Stage& g = *s.stg[p];
        std::vector<size_t> fill(g.soff);
        for (uint64_t idx = s.ptr[g.r0]; idx < s.ptr[g.r1]; ++idx) {
            const int q = owner(s.perm[idx]);
            if (q != rank) s.perm2[idx] = (uint32_t)(N + fill[q]++);
        }
    }
    // receive area: what rank k's stage p sends here, in k's rating order, [stage][peer]
    s.unpack.clear();
    for (size_t p = 0; p < P; ++p) {
        Side::Stage& g = *s.stg[p];
        g.roff.assign(nranks, 0);
        g.rcnt.assign(nranks, 0);
        g.rbeg = s.unpack.size();
        for (int k = 0; k < nranks; ++k) {
            g.roff[k] = s.unpack.size();
            if (k == rank) continue;
            for (uint64_t idx = s.ptr[s.sbounds[k][p]]; idx < s.ptr[s.sbounds[k][p + 1]]; ++idx)
                if (owner(s.perm[idx]) == rank) s.unpack.push_back(s.perm[idx]);
            g.rcnt[k] = s.unpack.size() - g.roff[k];
        }
        g.rend = s.unpack.size();
    }
    s.nrecv = s.unpack.size();
    if (N + s.nsend >= 0xffffffffull) fail(SBMF_E_ARG, "too many ratings for the 32-bit residual exchange");
}

static void build_side(uint64_t N, const uint32_t* key, const uint32_t* other, const double* rat, uint32_t R,
                       Side& s, std::vector<uint32_t>& pos_of_case) {
    s.R = R;
    s.ptr.assign((size_t)R + 1, 0);
    for (uint64_t c = 0; c < N; ++c) s.ptr[key[c] + 1]++;
    for (uint32_t i = 0; i < R; ++i) s.ptr[i + 1] += s.ptr[i];
    std::vector<uint32_t> fill(s.ptr.begin(), s.ptr.end() - 1);
    s.part.resize(N);
    s.r.resize(N);
    pos_of_case.resize(N);
    for (uint64_t c = 0; c < N; ++c) {  // file order within a row (gibbs_sbpmf_final.cpp:204-209)
        const uint32_t p = fill[key[c]]++;
        s.part[p] = other[c];
        s.r[p] = rat[c];
        pos_of_case[c] = p;
    }
}

// nnz-balanced contiguous partition, boundaries aligned to 256 rows.
void partition_bounds(const uint32_t* ptr, uint32_t R, int nranks, uint64_t* bounds) {
    bounds[0] = 0;
    for (int k = 1; k <= nranks; ++k) {
        uint32_t row = R;
        if (k < nranks) {
            const double target = (double)ptr[R] * k / nranks;
            row = (uint32_t)(std::lower_bound(ptr, ptr + R + 1, (uint32_t)std::llround(target)) - ptr);
            row = std::min((row + 128) / 256 * 256, R);
        }
        bounds[k] = std::max<uint64_t>(bounds[k - 1], row);
    }
}
static void partition(Side& s, int nranks, int rank, uint32_t nstages) {
    s.bounds.assign(nranks + 1, 0);
    partition_bounds(s.ptr.data(), (uint32_t)s.ptr.size() - 1, nranks, s.bounds.data());
    s.r0 = (uint32_t)s.bounds[rank];
    s.r1 = (uint32_t)s.bounds[rank + 1];
    // every rank's block cut into nstages nnz-balanced stages (known to every rank:
    // the exchange of stage p involves every rank's stage p)
    s.sbounds.assign(nranks, std::vector<uint64_t>(nstages + 1, 0));
    for (int k = 0; k < nranks; ++k) {
        const uint64_t b0 = s.bounds[k], b1 = s.bounds[k + 1];
        std::vector<uint64_t>& sb = s.sbounds[k];
        sb[0] = b0;
        for (uint32_t p = 1; p <= nstages; ++p) {
            uint64_t row = b1;
            if (p < nstages) {
                const double target = s.ptr[b0] + (double)(s.ptr[b1] - s.ptr[b0]) * p / nstages;
                row = (uint64_t)(std::lower_bound(s.ptr.begin() + b0, s.ptr.begin() + b1 + 1,
                                                  (uint32_t)std::llround(target)) - s.ptr.begin());
                row = std::min<uint64_t>(std::max<uint64_t>(row, b0), b1);
            }
            sb[p] = std::max<uint64_t>(sb[p - 1], row);
        }
    }
    s.stg.clear();
    for (uint32_t p = 0; p < nstages; ++p) {
        s.stg.emplace_back(new Side::Stage);
        s.stg.back()->r0 = (uint32_t)s.sbounds[rank][p];
        s.stg.back()->r1 = (uint32_t)s.sbounds[rank][p + 1];
    }
}

static void build_bins(const Side& s, Side::Stage& g, uint32_t stream_thr, bool f64, bool wide) {
    for (auto& b : g.bin_rows) b.clear();
    std::vector<uint32_t> order(g.r1 - g.r0);
    std::iota(order.begin(), order.end(), g.r0);
    auto deg = [&](uint32_t r) { return s.ptr[r + 1] - s.ptr[r]; };
    // heaviest first: blocks are dispatched roughly in index order, so the
    // longest rows start earliest (LPT)
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return deg(a) > deg(b); });
    for (uint32_t r : order) {
        const uint32_t d = deg(r);
        if (d > stream_thr) {
            g.bin_rows[KIND_STREAM].push_back(r);
            continue;
        }
        int kind = GK_W4;
        while (d > gk_maxdeg(kind, f64, wide)) ++kind;
        g.bin_rows[kind].push_back(r);
    }
}

static void fill_kernel_bytes(sbmf_ctx* c);
static void build_stream_tasks(const Side& s, Side::StreamSet& S, const std::vector<uint32_t>& rows, uint32_t gres,
                               uint32_t nblk);

// ------------------------------------------------------------------ prepare
template <typename T>
void prepare_T(sbmf_ctx* c) {
    const sbmf_config& cf = c->cfg;
    const uint64_t N = c->tu.size();  // > 0, and c->I, c->J are set (the caller: sbmf.cpp prepare_ctx)
    if (N >= 0xffffffffull) fail(SBMF_E_ARG, "more than 2^32-1 ratings are not supported");
    c->K = cf.num_factor;
    c->Kp = (c->K + 15) / 16 * 16;  // k-blocks of 16 start on 128-byte (f64) / 64-byte (f32) boundaries
    // the streaming kernel keeps partner-row element offsets (row * Kp) in 32 bits
    if ((uint64_t)(std::max(c->I, c->J) + 2) * c->Kp >= 0xffffffffull)
        fail(SBMF_E_ARG, "factor tables of %u x %u rows at K=%u exceed 2^32 elements", c->I, c->J, c->K);

    std::vector<uint32_t> pos_u, pos_v;
    build_side(N, c->tu.data(), c->ti.data(), c->tr.data(), c->I, c->users, pos_u);
    build_side(N, c->ti.data(), c->tu.data(), c->tr.data(), c->J, c->items, pos_v);
    c->users.perm.resize(N);
    c->items.perm.resize(N);
    for (uint64_t x = 0; x < N; ++x) {
        c->users.perm[pos_u[x]] = pos_v[x];
        c->items.perm[pos_v[x]] = pos_u[x];
    }
    // stages per half: the multi-GPU exchange of a stage overlaps the next stage's
    // compute; one rank needs no exchange (SBMF_STAGES overrides, for tests).  Two: each
    // extra stage costs its launches' fixed latency -- per-rank compute of the 8-way split
    // at 1 / 2 / 4 stages is 1.25 / 1.50 / 1.99 ms at K=100 and 2.01 / 2.31 / 2.90 ms at
    // K=200 (virtual ranks, r05s6) -- against about half the exchange hidden per doubling
    // (0.6 / 0.9 ms per sweep at an assumed 330 GB/s all-gather): two stages are the best
    // or tied over 150-600 GB/s at both K
    c->nstages = c->nranks > 1 ? 2u : 1u;
    if (const char* e = std::getenv("SBMF_STAGES")) c->nstages = std::max(1, std::min(16, std::atoi(e)));
    partition(c->users, c->nranks, c->rank, c->nstages);
    partition(c->items, c->nranks, c->rank, c->nstages);
    if (c->nranks > 1) {
        build_exchange(c->users, c->items, c->nranks, c->rank);  // user half -> item order
        build_exchange(c->items, c->users, c->nranks, c->rank);  // item half -> user order
    }
    // Gram-block kernels for rows <= the stream threshold, the streaming kernel above it
    const bool f64 = sizeof(T) == 8;
    const bool wide = !(cf.tune & 8u);  // f64 rows <= 64 ratings on one wave (default)
    const uint32_t gkmax = gk_maxdeg(GK_NUM - 1, f64, wide);
    const uint32_t sthr = std::min<uint32_t>(cf.stream_threshold ? cf.stream_threshold : gkmax, gkmax);
    for (Side* sd : {&c->users, &c->items})
        for (auto& g : sd->stg) build_bins(*sd, *g, sthr, f64, wide);
    // multi-wave Gram-block bins: ceil(deg / ratings-per-wave) waves per row,
    // contiguous sub-ranges since each bin is degree-descending
    for (Side* sd : {&c->users, &c->items})
        for (auto& gp : sd->stg)
        for (int k = GK_B2; k < GK_NUM; ++k) {
            Side::Stage& g = *gp;
            g.gsub[k].clear();
            const std::vector<uint32_t>& rows = g.bin_rows[k];
            const uint32_t per_wave = f64 ? 32 : 64;
            for (uint32_t i = 0; i < rows.size();) {
                const uint32_t d = sd->ptr[rows[i] + 1] - sd->ptr[rows[i]];
                const uint32_t nw = std::max(2u, (d + per_wave - 1) / per_wave);
                uint32_t j = i;
                while (j < rows.size() &&
                       std::max(2u, (sd->ptr[rows[j] + 1] - sd->ptr[rows[j]] + per_wave - 1) / per_wave) == nw)
                    ++j;
                // f64 rows of 5-8 eight-vector waves run as (nw + 1) / 2 sixteen-vector waves
                // (launch_gblock_nw): groups that launch the same kernel shape are one launch
                // (nw 5+6 and 7+8; the merged group carries its larger nw)
                auto shape = [&](uint32_t w) { return f64 && w >= 5 ? 100 + (w + 1) / 2 : w; };
                if (!g.gsub[k].empty() && shape(g.gsub[k].back()[0]) == shape(nw)) {
                    auto& last = g.gsub[k].back();  // degree-descending: the earlier group has the larger nw
                    last[2] += j - i;
                } else {
                    g.gsub[k].push_back({nw, i, j - i});
                }
                i = j;
            }
        }
    const uint32_t nblk = (c->K + 15) / 16;
    {
        int dev_cus = 0;
        HIPCHK(hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, cf.device));
        for (Side* sd : {&c->users, &c->items}) {
            // f64 item rows above 1024 ratings (75 % of the item ratings sit in rows
            // split over several tasks) on 16-wave k_gres workgroups, 2048-rating
            // tasks: half the chunks per split row, a quarter of the all-read
            // exchange; shorter item rows and every user row on 8-wave workgroups
            // (two independent tasks per CU).  Measured item launch 4.04 ms (all
            // 8-wave) / 3.88 (all 16-wave) / 3.70 (this split); the user side is
            // slower with any 16-wave share (1.59 / 2.23 / 1.66 ms).  Tune bit 27,
            // or an explicit workgroup-shape or hybrid bit, keeps 8-wave items.
            const bool item16 = sd == &c->items && sizeof(T) == 8 && !(cf.tune & (128u | 0x20000u | 0x8000000u));
            // f64 user rows on 4-wave k_gres workgroups (512-rating tasks, four workgroups per
            // CU): measured user streaming 1.49 -> 1.40 ms against 8-wave (r03s10); tune bit 23,
            // or an explicit workgroup-shape bit, keeps them on 8-wave workgroups
            const bool user4 = sd == &c->users && sizeof(T) == 8 && !(cf.tune & (128u | 0x20000u | 0x800000u));
            // f64 user rows above 512 ratings as a second set on 8-wave workgroups (1024-rating tasks:
            // rows up to 1024 whole, longer ones in half as many chunks) beside the 4-wave set of the
            // rest: the r05s26 phase profile had the 4-wave set's split-row chunks 63 % in the hand-off
            // phase; user half 2.85-2.89 -> 2.80-2.81 ms (r05s27, 3 rounds).  Tune bit 13 keeps one
            // 4-wave set; bit 14 (experiment) puts the long rows on 16-wave workgroups instead (slower)
            const bool user2 = user4 && (!(cf.tune & 0x2000u) || (cf.tune & 0x4000u));
            const uint32_t stunes[2] = {user4 ? cf.tune | 128u : cf.tune,
                                        user2 && !(cf.tune & 0x4000u) ? cf.tune : cf.tune | 0x20000u};
            // (round 4 measured a second user set neutral to slower -- rows above 1024 / 2048 ratings
            // on 16-wave workgroups, above 512 / 1024 on 8-wave ones: r04s9, r04s15 -- with the user
            // rows of 9..256 ratings still on the Gram-block kinds)
            for (auto& gp : sd->stg) {
            std::vector<uint32_t> rows[2];
            for (uint32_t r : gp->bin_rows[KIND_STREAM]) {  // degree-descending
                const uint32_t d = sd->ptr[r + 1] - sd->ptr[r];
                rows[(item16 && d > 1024u) || (user2 && d > 512u) ? 1 : 0].push_back(r);
            }
            for (int k = 0; k < 2; ++k) {
                Side::StreamSet& S = gp->ss[k];
                S.tune = stunes[k];
                // task capacity: the kernel's on-chip maximum, or smaller if split_chunk asks
                S.cmax = gstream_cmax<T>(S.tune);
                if (cf.split_chunk) S.cmax = std::min(S.cmax, std::max(cf.split_chunk, 1u));
                // (fewer persistent workgroups per CU, leaving CU slots to the Gram-block launches
                // beside the streaming one from its start: user 3 / 2 per CU +0.03 / +0.13 ms, item
                // 8-wave set 1 per CU +0.2 ms per sweep, r05s8)
                const int per_cu =
                    std::max(1, std::min(gstream_wg_target(S.tune), gstream_blocks_per_cu<T>(S.cmax, S.tune)));
                // (per-XCD task queues, each split row on one XCD: item stage 3.59 -> 3.77 ms standalone,
                // r06s3; removed, profiles/r06/ab/r06s3_xcd_queues.patch)
                build_stream_tasks(*sd, S, rows[k], (uint32_t)(dev_cus * per_cu), nblk);
            }
            }
        }
    }
    {  // test split in 256-aligned blocks
        const uint64_t T_ = c->su.size(), nb = (T_ + 255) / 256;
        c->tbounds.assign(c->nranks + 1, 0);
        c->tbblocks.assign(c->nranks + 1, 0);
        for (int k = 0; k <= c->nranks; ++k) {
            c->tbblocks[k] = nb * k / c->nranks;
            c->tbounds[k] = std::min<uint64_t>(T_, c->tbblocks[k] * 256);
        }
        c->t0 = c->tbounds[c->rank];
        c->t1 = c->tbounds[c->rank + 1];
    }

    hipStream_t st = c->st;
    upload(c->d_uptr, c->users.ptr, st);
    upload(c->d_upart, c->users.part, st);
    upload(c->d_uperm, c->users.perm, st);
    upload(c->d_ur, to_T<T>(c->users.r), st);
    upload(c->d_vptr, c->items.ptr, st);
    upload(c->d_vpart, c->items.part, st);
    upload(c->d_vperm, c->items.perm, st);
    upload(c->d_vr, to_T<T>(c->items.r), st);
    for (Side* sd : {&c->users, &c->items})
        for (auto& g : sd->stg)
            for (int k = 0; k < NBIN; ++k) upload(g->d_bins[k], g->bin_rows[k], st);
    {  // residual recompute tasks over the own item rows
        Side& s = c->items;
        s.rtasks.clear();
        s.rtptr.assign(1, 0);
        for (uint32_t r = s.r0; r < s.r1; ++r) {
            for (uint32_t b = s.ptr[r]; b < s.ptr[r + 1]; b += RESID_CHUNK)
                s.rtasks.push_back(ResidTask{r, b, std::min<uint32_t>(RESID_CHUNK, s.ptr[r + 1] - b), 0});
            s.rtptr.push_back((uint32_t)s.rtasks.size());
        }
        upload(c->d_rtasks, s.rtasks, st);
        upload(c->d_rtptr, s.rtptr, st);
        c->d_rtsq.alloc(std::max<size_t>(s.rtasks.size(), 1) * sizeof(double));
    }
    // split-row slots of stream set k: the largest over the stages and sides (set 0 and
    // set 1 of a half may run at the same time, so each set has an area of its own)
    size_t nxk[2] = {0, 0};
    for (Side* sd : {&c->users, &c->items})
        for (auto& g : sd->stg)
            for (int k = 0; k < 2; ++k) {
                const Side::StreamSet& S = g->ss[k];
                upload(g->d_stasks[k], S.stasks, st);
                upload(g->d_xrows[k], S.xrows, st);
                nxk[k] = std::max<size_t>(nxk[k], S.nxchunk);
            }
    c->xset_nx = std::max<size_t>(nxk[0], 1);
    {
        const size_t nx = c->xset_nx + std::max<size_t>(nxk[1], 1);
        // the streaming kernel addresses a set's slabs with 32-bit byte offsets (SplitTask::xrow ...)
        if ((uint64_t)nx * nblk * SLAB_DOUBLES * sizeof(double) >= 0xffffffffull)
            fail(SBMF_E_ARG, "split-row exchange area of %zu chunks at K=%u exceeds 2^32 bytes", nx, c->K);
        // Every slab word starts as the sentinel (all ones: "not published yet", kernels.hip XSENT)
        // and is the sentinel again when a streaming launch has run with its k_split_finish: a
        // chunk resets its slab of block t-1 after reading block t, k_split_finish the last
        // block's.  An area is used by one launch at a time: set 0 and set 1 have an area each
        // (they may run side by side), and the launches of one set -- both sides, every stage
        // (SBMF_STAGES) -- follow each other in stream order (run_half: each set's launches go
        // to one stream, or the stage ends with the compute stream waiting for the other).
        c->d_xslabs.alloc(nx * nblk * SLAB_DOUBLES * sizeof(double));
        HIPCHK(hipMemsetAsync(c->d_xslabs.p, 0xff, c->d_xslabs.bytes, st));
        c->d_gcold.alloc((size_t)c->nstages * 6 * sbmf_ctx::kColdSlot);
        c->h_gcold.assign((size_t)c->nstages * 6 * sbmf_ctx::kColdSlot, 0xff);  // nothing uploaded yet
        // each set's task-queue head.  Zeroed once here: every streaming launch leaves its set's
        // zero again (k_split_finish clears it after k_gres)
        c->d_xcnt.alloc(64 * sizeof(uint32_t));
        HIPCHK(hipMemsetAsync(c->d_xcnt.p, 0, c->d_xcnt.bytes, st));
        c->d_xchunk_sq.alloc(nx * sizeof(double));
        c->d_xchunk_tr.alloc(nx * sizeof(double));
        HIPCHK(hipMemsetAsync(c->d_xchunk_tr.p, 0, c->d_xchunk_tr.bytes, st));
        c->d_xnewown.alloc(nx * c->Kp * sizeof(T));
    }
    // factor tables [rows + 2][Kp]: row `rows` stays zero (the sentinel partner of
    // padded rating slots), row `rows + 1` is slack for the next-block prefetch
    // past the last column block; padding columns K..Kp-1 stay zero.
    c->d_U.alloc((size_t)(c->I + 2) * c->Kp * sizeof(T));
    c->d_V.alloc((size_t)(c->J + 2) * c->Kp * sizeof(T));
    HIPCHK(hipMemsetAsync(c->d_U.p, 0, c->d_U.bytes, st));
    HIPCHK(hipMemsetAsync(c->d_V.p, 0, c->d_V.bytes, st));
    // E_v: the user half's scatter target (+ its send area), E_u: the item half's
    c->d_Eu.alloc(std::max<uint64_t>(N + c->items.nsend, 1) * sizeof(T));
    c->d_Ev.alloc(std::max<uint64_t>(N + c->users.nsend, 1) * sizeof(T));
    if (c->nranks > 1) {
        upload(c->d_uperm2, c->users.perm2, st);
        upload(c->d_vperm2, c->items.perm2, st);
        upload(c->d_uunpack, c->users.unpack, st);
        upload(c->d_vunpack, c->items.unpack, st);
        c->d_xrecv.alloc(std::max<size_t>(std::max(c->users.nrecv, c->items.nrecv), 1) * sizeof(T));
        HIPCHK(hipMemsetAsync(c->d_xrecv.p, 0, c->d_xrecv.bytes, st));  // read as 0 by a virtual rank
    }
    HIPCHK(hipMemsetAsync(c->d_Eu.p, 0, c->d_Eu.bytes, st));
    HIPCHK(hipMemsetAsync(c->d_Ev.p, 0, c->d_Ev.bytes, st));
    c->d_rowsq_u.alloc((size_t)c->I * sizeof(double));
    c->d_rowtr_u.alloc((size_t)c->I * sizeof(double));
    c->d_rowsq_v.alloc((size_t)c->J * sizeof(double));
    c->d_rowtr_v.alloc((size_t)c->J * sizeof(double));
    HIPCHK(hipMemsetAsync(c->d_rowsq_v.p, 0, c->d_rowsq_v.bytes, st));
    HIPCHK(hipMemsetAsync(c->d_rowtr_v.p, 0, c->d_rowtr_v.bytes, st));
    // [sig_u | mu_u | sig_v | mu_v], each Kp long and zero padded, + 16 slack for prefetch
    c->d_hyper.alloc((4 * (size_t)c->Kp + 16) * sizeof(T));
    HIPCHK(hipMemsetAsync(c->d_hyper.p, 0, c->d_hyper.bytes, st));
    const uint32_t nchunk = (c->I + 255) / 256 + (c->J + 255) / 256;  // both tables' 256-row chunks
    c->d_colpart.alloc((size_t)nchunk * 2 * c->K * sizeof(double));
    c->h_res.assign(RES_COL + 4 * (size_t)c->K, 0.0);
    c->d_res.alloc(c->h_res.size() * sizeof(double));
    HIPCHK(hipMemsetAsync(c->d_res.p, 0, c->d_res.bytes, st));
    pinned_free(c->h_pre, c->h_pre_bytes);
    c->h_pre_bytes = c->h_res.size() * sizeof(double);
    pinned_alloc((void**)&c->h_pre, c->h_pre_bytes);
    pinned_free(c->h_io, c->h_io_bytes);
    c->h_io_bytes = 128 + 4 * (size_t)c->Kp * sizeof(T);
    pinned_alloc(&c->h_io, c->h_io_bytes);
    c->pre.valid = false;
    c->hyper_ahead = false;
    const uint64_t big = std::max<uint64_t>({(uint64_t)c->I, (uint64_t)c->J, c->su.size() / 128 + 2});
    // two halves: the prologue's sums and the evaluation's, which run side by side (one rank)
    c->d_scratch.alloc((big / 1024 + 16) * 4 * sizeof(double));
    c->scratch_half = (big / 1024 + 16) * 2;
    // test set, on the device in user order (a counting sort, stable: file order within a
    // user), so the evaluation's consecutive ratings share their user's row in cache; the
    // file order comes back through tperm in sbmf_predict.  The RMSE partial sums run in
    // this order.
    const uint64_t T_ = c->su.size();
    {
        std::vector<uint64_t> start((size_t)c->I + 1, 0);
        for (uint64_t x = 0; x < T_; ++x) ++start[c->su[x] + 1];
        for (uint32_t u = 0; u < c->I; ++u) start[u + 1] += start[u];
        c->tperm.resize(T_);
        std::vector<uint32_t> su2(T_), si2(T_);
        std::vector<double> sr2(T_);
        for (uint64_t x = 0; x < T_; ++x) {
            const uint64_t j = start[c->su[x]]++;
            c->tperm[j] = x;
            su2[j] = c->su[x];
            si2[j] = c->si[x];
            sr2[j] = c->sr[x];
        }
        upload(c->d_tu, su2, st);
        upload(c->d_ti, si2, st);
        upload(c->d_tr, sr2, st);
        HIPCHK(hipStreamSynchronize(st));  // the sorted copies are locals
    }
    c->d_tsum.alloc(std::max<uint64_t>(T_, 1) * sizeof(double));
    HIPCHK(hipMemsetAsync(c->d_tsum.p, 0, c->d_tsum.bytes, st));
    c->d_tpart.alloc(((T_ + 255) / 256 + 1) * 2 * sizeof(double));
    HIPCHK(hipMemsetAsync(c->d_tpart.p, 0, c->d_tpart.bytes, st));
    {  // per-half normals: host reference stream, or launch_philox_fill in throughput mode
        c->d_zU.alloc((size_t)c->I * c->K * sizeof(T));
        c->d_zV.alloc((size_t)c->J * c->K * sizeof(T));
    }
    {  // biased sampler state: b_i, b_j, their (mu, sigma) start at 0 (gibbs_sbpmf2.cpp:276-318)
        const size_t nb = c->bias ? 1 : 0;
        for (DBuf* d : {&c->d_bu, &c->d_mbu, &c->d_sbu}) {
            d->alloc(nb * c->I * sizeof(double));
            HIPCHK(hipMemsetAsync(d->p, 0, d->bytes, st));
        }
        for (DBuf* d : {&c->d_bv, &c->d_mbv, &c->d_sbv}) {
            d->alloc(nb * c->J * sizeof(double));
            HIPCHK(hipMemsetAsync(d->p, 0, d->bytes, st));
        }
        const bool refm = cf.rng_mode == SBMF_RNG_REFERENCE;
        c->d_var3u.alloc((refm ? nb : 0) * 3 * c->I * sizeof(double));
        c->d_var3v.alloc((refm ? nb : 0) * 3 * c->J * sizeof(double));
        c->d_epart.alloc(nb * 2 * ((size_t)c->I + 1) * sizeof(double));  // per user row {sum e, sum e^2}
        c->empty_u.clear();
        c->empty_v.clear();
        for (uint32_t i = 0; c->bias && i < c->I; ++i)
            if (c->users.ptr[i + 1] == c->users.ptr[i]) c->empty_u.push_back(i);
        for (uint32_t j = 0; c->bias && j < c->J; ++j)
            if (c->items.ptr[j + 1] == c->items.ptr[j]) c->empty_v.push_back(j);
        c->shadow_u.assign(c->empty_u.size(), {0.0, 0.0, 0.0});
        c->shadow_v.assign(c->empty_v.size(), {0.0, 0.0, 0.0});
    }
    const std::vector<double> z(c->K, 0.0);
    c->hyp[0] = c->hyp[1] = Hyper{1.0, 0.0, 0.0, 0.0, z, z, z, z};  // tau 1, the global bias and its state 0
    c->reported = 0;

    // initial factors (gibbs_sbpmf_final.cpp:236-250)
    if (cf.rng_mode == SBMF_RNG_REFERENCE) {
        c->grand.seed_((unsigned)cf.seed);
        std::vector<double> U((size_t)c->I * c->K), V((size_t)c->J * c->K);
        for (uint32_t i = 0; i < c->I; ++i)
            for (uint32_t k = 0; k < c->K; ++k) U[(size_t)i * c->K + k] = 0.0 + c->init_sd * leva_normal(c->grand);
        for (uint32_t k = 0; k < c->K; ++k)  // V is k-major in the reference
            for (uint32_t j = 0; j < c->J; ++j) V[(size_t)j * c->K + k] = 0.0 + c->init_sd * leva_normal(c->grand);
        HIPCHK(hipStreamSynchronize(st));
        upload_table<T>(c, c->d_U, U.data(), c->I);
        upload_table<T>(c, c->d_V, V.data(), c->J);
    } else {
        HIPCHK(launch_init_philox<T>(c->d_U.as<T>(), c->K, c->Kp, 0, c->I, c->init_sd, cf.seed, TAG_INIT_U, st));
        HIPCHK(launch_init_philox<T>(c->d_V.as<T>(), c->K, c->Kp, 0, c->J, c->init_sd, cf.seed, TAG_INIT_V, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    c->kprof = std::getenv("SBMF_KPROF") && std::atoi(std::getenv("SBMF_KPROF")) > 0;
    if (c->kprof) {
        if (const char* e = std::getenv("SBMF_KPROF_SET")) c->kprof_set = std::atoi(e) ? 1 : 0;
        c->d_kprof.alloc(128 * sizeof(unsigned long long));
        HIPCHK(hipMemset(c->d_kprof.p, 0, 128 * sizeof(unsigned long long)));
    }
    for (hipEvent_t& e : c->kevs) event_destroy(e);
    for (hipEvent_t& e : c->sev) event_destroy(e);
    c->kevs.assign((size_t)c->nstages * 2 * SBMF_NKIND * 2, nullptr);
    c->kprev.assign((size_t)c->nstages * 2 * SBMF_NKIND, (int8_t)-1);
    c->kbegin.assign((size_t)c->nstages * 2 * SBMF_NKIND, nullptr);
    c->sev.assign((size_t)2 * c->nstages, nullptr);
    for (hipEvent_t& e : c->kevs) event_create(&e);
    for (hipEvent_t& e : c->sev) event_create(&e, hipEventDisableTiming);
    for (hipEvent_t& e : c->tsev) event_destroy(e);
    c->tsev.assign(c->virt ? (size_t)2 * (c->nstages + 1) : 0, nullptr);
    for (hipEvent_t& e : c->tsev) event_create(&e);
    c->sweep = 0;
    c->collected = 0;
    fill_kernel_bytes(c);
    c->prepared = true;
}
template void prepare_T<float>(sbmf_ctx*);
template void prepare_T<double>(sbmf_ctx*);

// Streaming-kernel tasks (at most `cmax` ratings each: a whole row, or the
// equal chunks of a longer row) in one list, largest rows first, claimed in
// order by the running workgroups of a launch of `gres` workgroups (k_gres'
// queue); a split row's chunks are consecutive.
static void build_stream_tasks(const Side& s, Side::StreamSet& S, const std::vector<uint32_t>& rows, uint32_t gres,
                               uint32_t nblk) {
    const uint32_t cmax = S.cmax;
    S.stasks.clear();
    S.xrows.clear();
    S.nxchunk = 0;
    S.sgrid = 0;
    for (uint32_t r : rows) {  // rows: degree-descending
        const uint32_t n = s.ptr[r + 1] - s.ptr[r];
        const uint32_t nch = (n + cmax - 1) / cmax;
        if (nch > gres)
            fail(SBMF_E_ARG, "row %u has %u ratings: more than %u co-resident chunks of %u", r, n, gres, cmax);
        if (nch == 1) {
            S.stasks.push_back(SplitTask{r, s.ptr[r], n, 1, 0, 0, 0, 0, 0, {0, 0, 0}});
        } else {
            const uint32_t slab0 = S.nxchunk;
            const uint32_t per = (n + nch - 1) / nch;
            // byte offsets of the row's slabs in the set's area (set_data checks the area < 2^32 bytes)
            const uint64_t xstr = (uint64_t)nblk * SLAB_DOUBLES * sizeof(double), xrow = (uint64_t)slab0 * xstr;
            if (xrow + (uint64_t)nch * xstr >= 0xffffffffull)
                fail(SBMF_E_ARG, "split-row exchange area exceeds 2^32 bytes at row %u", r);
            for (uint32_t c = 0; c < nch; ++c) {
                const uint32_t b = c * per, e = std::min(n, b + per);
                S.stasks.push_back(SplitTask{r, s.ptr[r] + b, e - b, nch, c, slab0, (uint32_t)xrow,
                                             (uint32_t)(xrow + c * xstr), (uint32_t)xstr, {0, 0, 0}});
            }
            S.xrows.push_back(SplitRow{r, slab0, nch, 0});
            S.nxchunk += nch;
        }
    }
    S.sgrid = std::min<uint32_t>(gres, (uint32_t)S.stasks.size());
}

// SURVEY.md §8(d) algorithmic bytes of one launch over `rows`.
static uint64_t alg_bytes(const Side& s, const std::vector<uint32_t>& rows, uint32_t K, uint64_t tsz) {
    uint64_t b = 0;
    for (uint32_t r : rows) b += (uint64_t)(s.ptr[r + 1] - s.ptr[r]) * (tsz * K + 4 + tsz) + 2 * tsz * K;
    return b;
}
static void fill_kernel_bytes(sbmf_ctx* c) {
    const uint64_t tsz = tsize(c);
    for (int sd = 0; sd < 2; ++sd) {
        const Side& s = sd == 0 ? c->users : c->items;
        for (int k = 0; k < SBMF_NKIND; ++k) {
            c->timing.kern_bytes[sd][k] = 0;
            c->timing.kern_rows[sd][k] = 0;
        }
        for (const auto& g : s.stg) {  // a kind's launches summed over the stages
            for (int k = 0; k < NBIN; ++k) {
                c->timing.kern_bytes[sd][k] += alg_bytes(s, g->bin_rows[k], c->K, tsz);
                c->timing.kern_rows[sd][k] += (uint32_t)g->bin_rows[k].size();
            }
        }
    }
}

}  // namespace sbmf
