// fm_dev.h -- the device code the two libFM learners' kernels share (fmm.hip: one user and one
// item per case; fmg.hip: cases with any number of features): everything that does not depend on
// how the cases are stored.  The fixed-order reductions, the decode of a launch index into a row
// or a chunk, the row's draw with the reference's rules for non-finite values, the chunk draw of
// long rows, the residual sums and shift, the staged column chains of the hyperparameter draws,
// the train / test prediction frames of regression and of classification (fm_target.h) -- all
// device code -- and one host helper, the threads-per-row launch switch (fm_launch_rows), which
// sits here because it names the kernels' NT instantiations.
//
// Included by those two files only, which define FM_DEV_CONTRACT first: the state of `#pragma
// clang fp contract` in the row's draw.  fmg.hip restates libFM's expressions without fused
// multiply-adds (off); fmm.hip keeps the compiler's default for HIP (fast), which its pinned bits
// were recorded with.  Everything here has internal linkage, so each file gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "fm_target.h"
#include "rng.h"

#ifndef FM_DEV_CONTRACT
#error "define FM_DEV_CONTRACT (off or fast) before including fm_dev.h"
#endif
#define FM_PRAGMA_(x) _Pragma(#x)
#define FM_PRAGMA(x) FM_PRAGMA_(x)

namespace sbmf {
namespace {

// ---- reductions and small helpers
__device__ __forceinline__ double wsum(double x) {  // xor butterfly: bit-identical in every lane
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

__device__ __forceinline__ double block_sum(double s, double* red) {  // 256 threads, fixed order
    s = wsum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ double clampd(double p, double lo, double hi) {
    p = p < hi ? p : hi;     // std::min(max_target, p)
    return p > lo ? p : lo;  // std::max(min_target, p)
}

// A row's {m, s2} from its threads' shares (thread lt of the row): the butterfly within a wave,
// then the row's NWR waves meet in LDS and are summed in wave order.
template <int NWR>
__device__ __forceinline__ double2 row_sum(int lt, double m, double s2) {
    m = wsum(m);
    s2 = wsum(s2);
    if constexpr (NWR > 1) {
        __shared__ double red[2][NWR];
        const int w = lt >> 6;
        if ((lt & 63) == 0) {
            red[0][w] = m;
            red[1][w] = s2;
        }
        __syncthreads();
        m = 0.0;
        s2 = 0.0;
#pragma unroll
        for (int k = 0; k < NWR; ++k) {
            m += red[0][k];
            s2 += red[1][k];
        }
    }
    return make_double2(m, s2);
}

// Launch index ri of a pass: a chunk of a long row {row, first entry, entries, long-row index}, or
// row rows[ri] with the entries [ptr[row], ptr[row + 1]); di is the slot in delta (DI_ROW: the
// row's own where the launch has no chunks -- fmm's several ranks).  The row pointer is named by
// member (&FMPassArgs::ptr / &FGPassArgs::aptr), not passed as a value: every field of `a` is then
// read in the branch that uses it.  Passed as values, the pointers are loaded ahead of the branch
// and the 256- and 1024-thread pass kernels compile to other instructions.
struct FMRow {
    uint32_t row, beg, n, di;
};
template <bool DI_ROW, class A>
__device__ __forceinline__ FMRow fm_row(const A& a, const uint32_t* A::*ptr, uint32_t ri) {
    if (a.chunks) {
        const uint4 ck = a.chunks[ri];
        return {ck.x, ck.y, ck.z, ck.w};
    }
    const uint32_t row = a.rows[ri], beg = (a.*ptr)[row];
    return {row, beg, (a.*ptr)[row + 1] - beg, DI_ROW ? row : 0u};
}

// ---- the draw
// The row's draw from its sums m = sum h e, s2 = sum h^2 under the prior {lambda, mu}: MODE 0
// draw_w (fm_learn_mcmc.h:680-719), MODE 1 draw_v (:793-835).  a: the pass's alpha, do_sample
// and normals z[at * zs + zoff] (read by a sampling draw with a spread only).  keep: a non-finite
// draw restores the old value (the reference returns before the update).
template <int MODE, class A>
__device__ __forceinline__ double fm_draw(const A& a, double lambda, double mu, uint32_t at, double old, double m,
                                          double s2, bool& keep) {
    FM_PRAGMA(clang fp contract(FM_DEV_CONTRACT))
    if constexpr (MODE == 1) m -= old * s2;
    s2 = 1.0 / (lambda + a.alpha * s2);
    m = -s2 * (a.alpha * m - mu * lambda);
    double nv;
    if (isnan(s2) || isinf(s2)) {
        nv = 0.0;
    } else if (a.do_sample) {  // ran_gaussian(mean, stdev), random.h:166-172
        const double sd = sqrt(s2);
        nv = (sd == 0.0 || isnan(sd)) ? m : m + sd * a.z[(size_t)at * a.zs + a.zoff];
    } else {
        nv = m;
    }
    keep = isnan(nv) || isinf(nv);
    return keep ? old : nv;
}

// Long rows in chunks: one thread per long row i (attribute a0 + rows[i], chunks [cfirst[i],
// cfirst[i + 1])), the chunk sums added in chunk order, then draw(at, old, m, s2, keep); own and
// delta[i] = {old, new, keep} written.  rec (fmm's in-place passes; else null): the attribute's
// record {old, value kept} is replaced, the one it held kept in qq[i].
template <class Draw>
__device__ __forceinline__ void fm_chunk_draw_body(double* own, uint32_t a0, const uint32_t* __restrict__ rows,
                                                   const uint32_t* __restrict__ cfirst, uint32_t nlong,
                                                   const double2* __restrict__ csums, double4* __restrict__ delta,
                                                   double2* rec, double2* __restrict__ qq, Draw draw) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nlong) return;
    double m = 0.0, s2 = 0.0;
    for (uint32_t c = cfirst[i]; c < cfirst[i + 1]; ++c) {
        m += csums[c].x;
        s2 += csums[c].y;
    }
    const uint32_t at = a0 + rows[i];
    const double old = own[at];
    bool keep;
    const double nv = draw(at, old, m, s2, keep);
    own[at] = nv;
    if (rec) {
        qq[i] = rec[at];
        rec[at] = make_double2(old, nv);  // nv == old when kept
    }
    delta[i] = make_double4(old, nv, keep ? 1.0 : 0.0, 0.0);
}

// ---- the residuals: e[q] of an array of doubles, or eq[q].x of the {e, q} records
template <class T>
__device__ __forceinline__ auto& fm_residual(T& r) {
    if constexpr (std::is_same_v<std::remove_const_t<T>, double>)
        return r;
    else
        return r.x;
}

// part[b] = {sum e^2, sum (e - w0)} over 1024-case blocks
template <class T>
__device__ __forceinline__ void fm_esums_body(const T* __restrict__ e, uint64_t n, double w0, double* __restrict__ part) {
    const uint64_t b0 = (uint64_t)blockIdx.x * 1024;
    double s = 0.0, d = 0.0;
    for (int k = 0; k < 4; ++k) {
        const uint64_t q = b0 + k * 256 + threadIdx.x;
        if (q < n) {
            const double v = fm_residual(e[q]);
            s += v * v;
            d += v - w0;
        }
    }
    s = wsum(s);
    d = wsum(d);
    __shared__ double red[2][4];
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = s;
        red[1][threadIdx.x >> 6] = d;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        part[2 * blockIdx.x + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

template <class T>
__device__ __forceinline__ void fm_shift_body(T* __restrict__ e, uint64_t n, double d) {
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (q < n) fm_residual(e[q]) -= d;
}

// ---- the column chains of the hyperparameter draws (fm_learn_mcmc.h:951-1089)
// Two sequential chains over the cnt members of a column (or of one group of it), in the host
// loop's order: with *in = {mu, gm0}, gm from gm0 adding (x_q - mu)^2 for q = 0..cnt-1, and m from
// 0 adding x_q -- the host loop's result bit for bit (no contraction); out[oi] = {gm, m}.
// value(q) is member q's x (Q: the width the member index is computed in).  The whole 256-thread
// workgroup stages CH-value chunks of the members and their squared deviations in LDS
// (double-buffered, 32 CH bytes); lane 0 runs the gm chain and lane 1 the m chain, side by side in
// one instruction stream.  gm0 is read by lane 0 alone, through `in`.
template <uint32_t CH, class Q, class Value>
__device__ __forceinline__ void fm_chains_body(uint32_t cnt, const double2* in, double2* out, size_t oi,
                                               Value value) {
#pragma clang fp contract(off)
    __shared__ __align__(16) double xs[2][CH];
    __shared__ __align__(16) double ds[2][CH];
    const double mu = in->x;
    double acc = threadIdx.x == 0 ? in->y : 0.0;  // lane 0: gm, lane 1: m
    const uint32_t nch = (cnt + CH - 1) / CH;
    auto stage = [&](uint32_t ch, int b) {
        for (uint32_t i = threadIdx.x; i < CH; i += 256) {
            const Q q = (Q)ch * CH + i;
            const double t = q < cnt ? value(q) : 0.0;
            const double d = t - mu;
            xs[b][i] = t;
            ds[b][i] = d * d;
        }
    };
    stage(0, 0);
    __syncthreads();
    for (uint32_t ch = 0; ch < nch; ++ch) {
        const int b = ch & 1;
        if (ch + 1 < nch) stage(ch + 1, b ^ 1);
        if (threadIdx.x < 2) {
            const double* __restrict__ src = threadIdx.x == 0 ? ds[b] : xs[b];
            const uint32_t n = min(CH, cnt - ch * CH);
            uint32_t j = 0;
            for (; j + 32 <= n; j += 32) {
                double2 t[16];  // 16-byte LDS reads, all issued before the first add
#pragma unroll
                for (int u = 0; u < 16; ++u) t[u] = reinterpret_cast<const double2*>(src + j)[u];
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    acc = acc + t[u].x;
                    acc = acc + t[u].y;
                }
            }
            for (; j < n; ++j) acc = acc + src[j];
        }
        __syncthreads();
    }
    __shared__ double res[2];
    if (threadIdx.x < 2) res[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[oi] = make_double2(res[0], res[1]);
}

// ---- the prediction frames (predict_data_and_write_to_eterms and _evaluate around it), one case
// per thread of 256-thread blocks; pred(c) is the layout's prediction of case c, a.lo / a.hi the
// target range
// Train: store(c, pred - y) keeps the residual; part[b] = the block's sum of (clamp(pred) - y)^2.
template <class A, class Pred, class Store>
__device__ __forceinline__ void fm_train_frame(const A& a, uint64_t n, const float* y,
                                               double* part, Pred pred, Store store) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    double se = 0.0;
    if (c < n) {
        const double pr = pred(c);
        const double err = clampd(pr, a.lo, a.hi) - y[c];
        se = err * err;
        store(c, pr - y[c]);
    }
    __shared__ double red[4];
    se = block_sum(se, red);
    if (threadIdx.x == 0) part[blockIdx.x] = se;
}

// Test: pthis[t] = pred, sum_all[t] += clamp(pred); part[2b] = the block's sum of
// (clamp(sum_all / it1) - y)^2 (the running mean), part[2b + 1] of (clamp(pred) - y)^2.
template <class A, class Pred>
__device__ __forceinline__ void fm_test_frame(const A& a, uint64_t n, const float* y, double it1,
                                              double* pthis, double* sum_all,
                                              double* part, Pred pred) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    double sa = 0.0, st = 0.0;
    if (t < n) {
        const double pr = pred(t);
        pthis[t] = pr;
        const double s = sum_all[t] + clampd(pr, a.lo, a.hi);
        sum_all[t] = s;
        const double ea = clampd(s * (1.0 / it1), a.lo, a.hi) - y[t];  // _evaluate: pred * normalizer
        const double et = clampd(pr * 1.0, a.lo, a.hi) - y[t];
        sa = ea * ea;
        st = et * et;
    }
    __shared__ double red[2][4];
    sa = block_sum(sa, red[0]);
    st = block_sum(st, red[1]);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = sa;
        part[2 * blockIdx.x + 1] = st;
    }
}

// ---- the classification frames (-task c, fm_target.h): the same one pass per case, the targets
// y in {-1, +1}.  Counts are integers, summed exactly (fm_count_sums_body).
__device__ __forceinline__ uint32_t block_count(bool hit, uint32_t* red) {  // 256 threads
    const uint32_t w = (uint32_t)__popcll(__ballot(hit));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// the reference's vote (fm_learn_mcmc_simultaneous.h:193, :333, :389)
__device__ __forceinline__ bool fm_vote(double p, float y) { return (p >= 0.5 && y > 0.0f) || (p < 0.5 && y < 0.0f); }

// ran_left_tgaussian(left) (random.h:72-102) from the counter-based stream of (seed, it, row).
// Both loops are bounded: 64 tries, then the truncation point (fm_target.h has the odds).
__device__ __forceinline__ double fm_left_tgauss(uint64_t seed, uint32_t it, uint32_t row, double left) {
#pragma clang fp contract(off)
    if (left <= 0.0) {  // naive rejection, two normals per Philox block
        for (uint32_t t = 0; t < 32; ++t) {
            double z0, z1;
            philox_normal_pair(seed, row, it, TAG_FMC_TARGET, t, z0, z1);
            if (!(z0 < left)) return z0;
            if (!(z1 < left)) return z1;
        }
        return left;
    }
    // Robert's translated exponential: ran_exp and ran_uniform of one Philox block per try
    const double alpha_star = 0.5 * (left + sqrt(left * left + 4.0));
    for (uint32_t t = 0; t < 64; ++t) {
        double u0, u1;
        philox_uniform_pair(seed, row, it, TAG_FMC_TARGET, t, u0, u1);
        const double z = -log(u0) / alpha_star + left;  // u0 in (0, 1]: the reference's 1 - ran_uniform()
        double d = z - alpha_star;
        d = exp(-(d * d) / 2);
        if (u1 < d) return z;
    }
    return left;
}

// the latent target of a case with prediction mu and label y (fm_learn_mcmc_simultaneous.h:197-218)
template <int TM>
__device__ __forceinline__ double fm_target(const FMTargetArgs& ta, uint64_t c, double mu, float y) {
#pragma clang fp contract(off)
    if constexpr (TM == FM_TGT_ALS) {
        const double phi_minus_mu = exp(-mu * mu / 2.0) / sqrt(3.141 * 2);
        const double Phi_minus_mu = ref_cdf_gaussian(-mu);
        return y >= 0.0f ? mu + phi_minus_mu / (1 - Phi_minus_mu) : mu - phi_minus_mu / Phi_minus_mu;
    } else {
        const uint32_t row = ta.fidx ? ta.fidx[c] : (uint32_t)c;
        const double lim = (0.0 - mu) / 1.0;  // (left - mean) / stdev, (right - mean) / stdev
        return y >= 0.0f ? mu + 1.0 * fm_left_tgauss(ta.seed, ta.it, row, lim)
                         : mu + 1.0 * -fm_left_tgauss(ta.seed, ta.it, row, -lim);
    }
}

// Train: p = cdf_gaussian(pred) votes, store(c, pred - latent target); ta.cnt[b] = the block's
// correct votes.  FM_TGT_HOST: store(c, pred) and ta.yhat[c] = pred, the targets follow from the host.
template <int TM, class Pred, class Store>
__device__ __forceinline__ void fm_class_train_frame(const FMTargetArgs& ta, uint64_t n, const float* y, Pred pred,
                                                     Store store) {
#pragma clang fp contract(off)
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool hit = false;
    if (c < n) {
        const double pr = pred(c);
        const float yc = y[c];
        hit = fm_vote(ref_cdf_gaussian(pr), yc);
        if constexpr (TM == FM_TGT_HOST) {
            ta.yhat[c] = pr;
            store(c, pr);
        } else {
            store(c, pr - fm_target<TM>(ta, c, pr, yc));
        }
    }
    __shared__ uint32_t red[4];
    const uint32_t k = block_count(hit, red);
    if (threadIdx.x == 0) ta.cnt[blockIdx.x] = k;
}

// Test: pthis[t] = p = cdf_gaussian(pred), sum_all[t] += p (no clamp); cnt[2b] = the block's
// correct votes of the running mean sum_all / it1, cnt[2b + 1] of p; ll[b] = the block's sum of
// -(m log10 q + (1 - m) log10(1 - q)), q = p clipped to [0.01, 0.99], m = (y + 1) / 2
// (_evaluate_class_map's first loop and _evaluate_class, :327-338, :383-401)
template <class Pred>
__device__ __forceinline__ void fm_class_test_frame(uint64_t n, const float* y, double it1, double* pthis,
                                                    double* sum_all, uint32_t* cnt, double* ll, Pred pred) {
#pragma clang fp contract(off)
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool ha = false, ht = false;
    double l = 0.0;
    if (t < n) {
        const double p = ref_cdf_gaussian(pred(t));
        pthis[t] = p;
        const double s = sum_all[t] + p;
        sum_all[t] = s;
        const float yt = y[t];
        ha = fm_vote(s * (1.0 / it1), yt);
        ht = fm_vote(p * 1.0, yt);
        const double m = (yt + 1.0) * 0.5;
        double pll = p;
        if (pll > 0.99) pll = 0.99;
        if (pll < 0.01) pll = 0.01;
        l = -(m * log10(pll) + (1 - m) * log10(1 - pll));
    }
    __shared__ uint32_t red[2][4];
    __shared__ double redl[4];
    const uint32_t ka = block_count(ha, red[0]), kt = block_count(ht, red[1]);
    l = block_sum(l, redl);
    if (threadIdx.x == 0) {
        cnt[2 * blockIdx.x] = ka;
        cnt[2 * blockIdx.x + 1] = kt;
        ll[blockIdx.x] = l;
    }
}

// out[w] = sum_b part[b * width + w], exact (64-bit integers); one 256-thread block per column w
__device__ __forceinline__ void fm_count_sums_body(const uint32_t* __restrict__ part, uint32_t nb, uint32_t width,
                                                   unsigned long long* __restrict__ out) {
    const uint32_t w = blockIdx.x;
    unsigned long long s = 0;
    for (uint32_t b = threadIdx.x; b < nb; b += 256) s += part[(size_t)b * width + w];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    __shared__ unsigned long long red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[w] = red[0] + red[1] + red[2] + red[3];
}

// e[q] -= t[q]: the host's targets (FM_TGT_HOST)
template <class T>
__device__ __forceinline__ void fm_sub_body(T* __restrict__ e, uint64_t n, const double* __restrict__ t) {
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (q < n) fm_residual(e[q]) -= t[q];
}

// ---- host: a pass over nrows rows with tpr threads each.  launch(NT, grid, block) starts the
// NT-threads-per-row instantiation (NT a std::integral_constant): a 256-thread block holds four
// 64-thread rows, or one row of 256 or 1024 threads.
template <class Launch>
hipError_t fm_launch_rows(int tpr, uint32_t nrows, Launch launch) {
    switch (tpr) {
        case 64:
            launch(std::integral_constant<int, 64>{}, dim3((nrows + 3) / 4), dim3(256));
            break;
        case 256:
            launch(std::integral_constant<int, 256>{}, dim3(nrows), dim3(256));
            break;
        case 1024:
            launch(std::integral_constant<int, 1024>{}, dim3(nrows), dim3(1024));
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace
}  // namespace sbmf
