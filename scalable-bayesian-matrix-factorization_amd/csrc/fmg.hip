// fmg.hip -- gfx950 kernels of the general libFM MCMC / ALS learner (fmg.h).
//
// A pass is one launch over the attribute rows of one (range, row-length bin).  A row walks
// its CSC entries {case, x} (sequential, 8 bytes each), gathers each case's {e, q} record
// (one 16-byte load), reduces sum h e and sum h^2 in a fixed order (lane-strided partial
// sums, xor butterfly, waves in wave order), draws its value, and scatters the updated
// record back (one 16-byte store; the w pass stores e alone).  No two rows of a launch share
// a case (sbmf_fm_ranges), so the scatter has no collisions and needs no atomics; every sum
// has a fixed order, so a rerun is bit-identical.  Contraction is off in the arithmetic that
// restates libFM's expressions: the reference is compiled without fused multiply-adds.
// What does not depend on how the cases are stored is fm_dev.h, shared with fmm.hip (listed
// there); this file keeps the {e, q} cache walk, the group lookup of the draw's prior, k_fmg_q
// and fg_pred.  Block-structure relations (k_fmr_*, fmg.h) add, per relation, the per-block-row
// gather of the cases' terms, the passes over the relation's attributes with the block rows'
// records in the place of the cases', the sync back to the cases, q^B and the block predictions.
#include <hip/hip_runtime.h>

#include "fmg.h"

#define FM_DEV_CONTRACT off  // the draw without fused multiply-adds, as the rest of this file
#include "fm_dev.h"

namespace sbmf {
namespace {

// The row's draw (fm_draw) under its prior.  GR: the row's group's (lm[grp[at]], one small load
// per row); else the launch's scalars.
template <int MODE, bool GR>
__device__ __forceinline__ double fmg_draw(const FGPassArgs& a, uint32_t at, double old, double m, double s2,
                                           bool& keep) {
    double lambda = a.lambda, mu = a.mu;
    if constexpr (GR) {
        const uint32_t g = a.grp_bytes == 1   ? static_cast<const uint8_t*>(a.grp)[at]
                           : a.grp_bytes == 2 ? static_cast<const uint16_t*>(a.grp)[at]
                                              : static_cast<const uint32_t*>(a.grp)[at];
        const double2 t = a.lm[g];
        lambda = t.x;
        mu = t.y;
    }
    return fm_draw<MODE>(a, lambda, mu, at, old, m, s2, keep);
}

// MODE 0: draw_w (fm_learn_mcmc.h:670-719); MODE 1: draw_v (:780-835).  NT threads per row; a
// 256-thread block holds 256 / NT rows (NT <= 256) or one row (NT = 1024).
template <int MODE, int NT, bool GR>
__device__ __forceinline__ void fmg_pass_body(const FGPassArgs& a) {
#pragma clang fp contract(off)
    constexpr int RPB = NT >= 256 ? 1 : 256 / NT;
    constexpr int NWR = NT >= 64 ? NT / 64 : 1;  // waves per row
    const int sub = threadIdx.x / NT, lt = threadIdx.x % NT;
    const uint32_t ri = blockIdx.x * RPB + sub;
    if (NT == 64 && ri >= a.nrows) return;  // a whole wave: no block barriers on this path
    const auto [row, beg, n, di] = fm_row<false>(a, &FGPassArgs::aptr, ri);
    const int xm = a.xmode;
    const double4 dl = xm == 2 ? a.delta[di] : make_double4(0.0, 0.0, 0.0, 0.0);
    const double old = xm == 2 ? dl.x : a.own[row];
    // a lane's first MCF entries stay in registers (case, x, e, q) from the sums to the update
    constexpr int MCF = 4;
    uint32_t cc[MCF];
    float cx[MCF];
    double2 cr[MCF];
    double m = 0.0, s2 = 0.0;
    const uint32_t nsum = xm == 2 ? 0u : n;
#pragma unroll
    for (int j = 0; j < MCF; ++j) {
        const uint32_t k = lt + j * NT;
        cc[j] = 0;
        cx[j] = 0.f;
        cr[j] = make_double2(0.0, 0.0);
        if (k < nsum) {
            const uint2 en = a.ent[beg + k];
            const float x = __uint_as_float(en.y);
            const double2 r = a.eq[en.x];
            cc[j] = en.x;
            cx[j] = x;
            cr[j] = r;
            if constexpr (MODE == 0) {
                m += x * (r.x - old * x);
                s2 += x * x;
            } else {
                const double h = x * (r.y - x * old);
                m += h * r.x;
                s2 += h * h;
            }
        }
    }
    for (uint32_t k = lt + MCF * NT; k < nsum; k += NT) {
        const uint2 en = a.ent[beg + k];
        const float x = __uint_as_float(en.y);
        const double2 r = a.eq[en.x];
        if constexpr (MODE == 0) {
            m += x * (r.x - old * x);
            s2 += x * x;
        } else {
            const double h = x * (r.y - x * old);
            m += h * r.x;
            s2 += h * h;
        }
    }
    if (xm != 2) {
        const double2 ms = row_sum<NWR>(lt, m, s2);
        m = ms.x;
        s2 = ms.y;
    }
    if (xm == 1) {  // the chunk's share of its row's sums
        if (lt == 0) a.sums[ri] = make_double2(m, s2);
        return;
    }
    double nv;
    bool keep;
    if (xm == 2) {
        nv = dl.y;
        keep = dl.z != 0.0;
    } else {
        nv = fmg_draw<MODE, GR>(a, row, old, m, s2, keep);
        if (lt == 0) a.own[row] = nv;
    }
    if (keep) return;  // the reference returns before the update (:697-710, :811-824)
    const double d = old - nv;
    auto update = [&](uint32_t c, float x, double2 r) {
        if constexpr (MODE == 0) {
            const double h = x;
            a.eq[c].x = r.x - h * d;
        } else {
            const double h = x * (r.y - x * old);
            a.eq[c] = make_double2(r.x - h * d, r.y - x * d);
        }
    };
#pragma unroll
    for (int j = 0; j < MCF; ++j) {
        const uint32_t k = lt + j * NT;
        if (k < n) {
            if (xm != 2) {
                update(cc[j], cx[j], cr[j]);
            } else {
                const uint2 en = a.ent[beg + k];
                update(en.x, __uint_as_float(en.y), a.eq[en.x]);
            }
        }
    }
    for (uint32_t k = lt + MCF * NT; k < n; k += NT) {
        const uint2 en = a.ent[beg + k];
        update(en.x, __uint_as_float(en.y), a.eq[en.x]);
    }
}

// k_fmg_pass: the launch's one prior; k_fmg_gpass: every row its group's (attribute groups)
template <int MODE, int NT>
__global__ __launch_bounds__(NT > 256 ? NT : 256) void k_fmg_pass(FGPassArgs a) {
    fmg_pass_body<MODE, NT, false>(a);
}
template <int MODE, int NT>
__global__ __launch_bounds__(NT > 256 ? NT : 256) void k_fmg_gpass(FGPassArgs a) {
    fmg_pass_body<MODE, NT, true>(a);
}

// long rows in chunks: the draw per long row
template <int MODE, bool GR>
__device__ __forceinline__ void fmg_chunk_draw_body(const FGPassArgs& a, const uint32_t* __restrict__ rows,
                                                    const uint32_t* __restrict__ cfirst, uint32_t nlong,
                                                    const double2* __restrict__ csums, double4* __restrict__ delta) {
    fm_chunk_draw_body(a.own, 0, rows, cfirst, nlong, csums, delta, nullptr, nullptr,
                       [&](uint32_t at, double old, double m, double s2, bool& keep) {
                           return fmg_draw<MODE, GR>(a, at, old, m, s2, keep);
                       });
}
template <int MODE>
__global__ __launch_bounds__(256) void k_fmg_chunk_draw(FGPassArgs a, const uint32_t* __restrict__ rows,
                                                        const uint32_t* __restrict__ cfirst, uint32_t nlong,
                                                        const double2* __restrict__ csums, double4* __restrict__ delta) {
    fmg_chunk_draw_body<MODE, false>(a, rows, cfirst, nlong, csums, delta);
}
template <int MODE>
__global__ __launch_bounds__(256) void k_fmg_gchunk_draw(FGPassArgs a, const uint32_t* __restrict__ rows,
                                                         const uint32_t* __restrict__ cfirst, uint32_t nlong,
                                                         const double2* __restrict__ csums, double4* __restrict__ delta) {
    fmg_chunk_draw_body<MODE, true>(a, rows, cfirst, nlong, csums, delta);
}

// ---- relations (fmg.h): a relation's pass.  The frame is fmg_pass_body's -- row decode, chunk
// modes, fixed-order sums, the draw, the early return of a kept value --; the record is block row
// j's {we, y, wnum, q | weq, wc, wc_sqr} and the sums and updates are draw_w_rel's (MODE 0,
// fm_learn_mcmc.h:727-736, :770-776) and draw_v_rel's (MODE 1, :845-855, :889-898), written as
// their lines are written: x is a float, so x * x is a float product.  Both draws subtract old *
// s2 from m after the sums (:736, :855), which is fm_draw's MODE 1.  A block row is a few entries
// of a short table: the update re-reads its record rather than keep it in registers.
template <int MODE, int NT, bool GR>
__device__ __forceinline__ void fmr_pass_body(const FGPassArgs& a) {
#pragma clang fp contract(off)
    constexpr int RPB = NT >= 256 ? 1 : 256 / NT;
    constexpr int NWR = NT >= 64 ? NT / 64 : 1;
    const int sub = threadIdx.x / NT, lt = threadIdx.x % NT;
    const uint32_t ri = blockIdx.x * RPB + sub;
    if (NT == 64 && ri >= a.nrows) return;
    const auto [row, beg, n, di] = fm_row<false>(a, &FGPassArgs::aptr, ri);
    const int xm = a.xmode;
    const double4 dl = xm == 2 ? a.delta[di] : make_double4(0.0, 0.0, 0.0, 0.0);
    const double old = xm == 2 ? dl.x : a.own[row];
    double m = 0.0, s2 = 0.0;
    const uint32_t nsum = xm == 2 ? 0u : n;
    for (uint32_t k = lt; k < nsum; k += NT) {
        const uint2 en = a.ent[beg + k];
        const float x = __uint_as_float(en.y);
        const double4 r0 = a.rb[2 * (size_t)en.x];
        if constexpr (MODE == 0) {
            m += x * r0.x;
            s2 += x * x * r0.z;
        } else {
            const double4 r1 = a.rb[2 * (size_t)en.x + 1];
            const double h = x * (r0.w - x * old);
            m += (h * r0.x + x * r1.x);
            s2 += (h * h * r0.z + 2 * r1.y * x * h + x * x * r1.z);
        }
    }
    if (xm != 2) {
        const double2 ms = row_sum<NWR>(lt, m, s2);
        m = ms.x;
        s2 = ms.y;
    }
    if (xm == 1) {
        if (lt == 0) a.sums[ri] = make_double2(m, s2);
        return;
    }
    double nv;
    bool keep;
    if (xm == 2) {
        nv = dl.y;
        keep = dl.z != 0.0;
    } else {
        nv = fmg_draw<1, GR>(a, row, old, m, s2, keep);
        if (lt == 0) a.own[row] = nv;
    }
    if (keep) return;
    const double d = old - nv, dn = nv - old;
    for (uint32_t k = lt; k < n; k += NT) {
        const uint2 en = a.ent[beg + k];
        const float x = __uint_as_float(en.y);
        double4 r0 = a.rb[2 * (size_t)en.x];
        if constexpr (MODE == 0) {
            const double h = x;
            r0.x -= h * d * r0.z;
            r0.y += dn * h;
        } else {
            double4 r1 = a.rb[2 * (size_t)en.x + 1];
            const double h = x * (r0.w - x * old);
            r0.x -= d * (h * r0.z + x * r1.y);
            r0.w -= d * x;
            r1.x -= d * (h * r1.y + x * r1.z);
            r0.y += dn * h;
            a.rb[2 * (size_t)en.x + 1] = r1;
        }
        a.rb[2 * (size_t)en.x] = r0;
    }
}

template <int MODE, int NT>
__global__ __launch_bounds__(NT > 256 ? NT : 256) void k_fmr_pass(FGPassArgs a) {
    fmr_pass_body<MODE, NT, false>(a);
}
template <int MODE, int NT>
__global__ __launch_bounds__(NT > 256 ? NT : 256) void k_fmr_gpass(FGPassArgs a) {
    fmr_pass_body<MODE, NT, true>(a);
}

// a row's four sums: row_sum's order for each
template <int NWR>
__device__ __forceinline__ double4 row_sum4(int lt, double4 s) {
    s.x = wsum(s.x);
    s.y = wsum(s.y);
    s.z = wsum(s.z);
    s.w = wsum(s.w);
    if constexpr (NWR > 1) {
        __shared__ double4 red[NWR];
        if ((lt & 63) == 0) red[lt >> 6] = s;
        __syncthreads();
        s = make_double4(0.0, 0.0, 0.0, 0.0);
#pragma unroll
        for (int k = 0; k < NWR; ++k) {
            s.x += red[k].x;
            s.y += red[k].y;
            s.z += red[k].z;
            s.w += red[k].w;
        }
    }
    return s;
}

// the gather with its un-sync (fmg.h); V: the v step's four sums, else we alone
template <int V, int NT>
__global__ __launch_bounds__(NT > 256 ? NT : 256) void k_fmr_gather(FGRelArgs a) {
#pragma clang fp contract(off)
    constexpr int RPB = NT >= 256 ? 1 : 256 / NT;
    constexpr int NWR = NT >= 64 ? NT / 64 : 1;
    const int sub = threadIdx.x / NT, lt = threadIdx.x % NT;
    const uint32_t ri = blockIdx.x * RPB + sub;
    if (NT == 64 && ri >= a.nrows) return;
    uint32_t j, beg, n;
    if (a.chunks) {
        const uint4 ck = a.chunks[ri];
        j = ck.x, beg = ck.y, n = ck.z;
    } else {
        j = a.rows[ri], beg = a.bptr[j], n = a.bptr[j + 1] - beg;
    }
    const double4 r0 = a.rb[2 * (size_t)j];
    const double y = r0.y, qb = r0.w;
    double4 s = make_double4(0.0, 0.0, 0.0, 0.0);  // we, weq, wc, wc_sqr
    for (uint32_t k = lt; k < n; k += NT) {
        const uint32_t c = a.bcase[beg + k];
        const double2 r = a.eq[c];
        s.x += r.x;
        if constexpr (V) {
            const double q = r.y - qb;
            s.y += (r.x * q);
            s.z += q;
            s.w += (q * q);
            a.eq[c] = make_double2(r.x - (y + q * qb), q);
        } else {
            a.eq[c].x = r.x - y;
        }
    }
    s = row_sum4<NWR>(lt, s);
    if (a.chunks) {  // the chunk's share of its block row's sums
        if (lt == 0) a.sums[ri] = s;
        return;
    }
    if (lt == 0) {
        a.rb[2 * (size_t)j] = make_double4(s.x, y, r0.z, qb);
        if constexpr (V) a.rb[2 * (size_t)j + 1] = make_double4(s.y, s.z, s.w, 0.0);
    }
}

// one thread per long block row: its chunks' sums in chunk order, then its record
template <int V>
__global__ __launch_bounds__(256) void k_fmr_gather_combine(const uint32_t* __restrict__ rows,
                                                            const uint32_t* __restrict__ cfirst, uint32_t nlong,
                                                            const double4* __restrict__ sums, double4* __restrict__ rb) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nlong) return;
    double4 s = make_double4(0.0, 0.0, 0.0, 0.0);
    for (uint32_t c = cfirst[i]; c < cfirst[i + 1]; ++c) {
        const double4 t = sums[c];
        s.x += t.x;
        s.y += t.y;
        s.z += t.z;
        s.w += t.w;
    }
    const size_t j = rows[i];
    rb[2 * j].x = s.x;
    if constexpr (V) rb[2 * j + 1] = make_double4(s.y, s.z, s.w, 0.0);
}

template <int V>
__global__ __launch_bounds__(256) void k_fmr_sync(const uint32_t* __restrict__ map, uint64_t n,
                                                  const double4* __restrict__ rb, double2* __restrict__ eq) {
#pragma clang fp contract(off)
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const double4 r0 = rb[2 * (size_t)map[c]];
    if constexpr (V) {
        const double2 r = eq[c];
        eq[c] = make_double2(r.x + (r0.y + r.y * r0.w), r.y + r0.w);
    } else {
        eq[c].x += r0.y;
    }
}

__global__ __launch_bounds__(256) void k_fmr_q(const uint32_t* __restrict__ rptr, const uint32_t* __restrict__ rattr,
                                               const float* __restrict__ rx, uint32_t nb, const double* __restrict__ vf,
                                               double4* __restrict__ rb) {
#pragma clang fp contract(off)
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nb) return;
    double q = 0.0;
    for (uint32_t k = rptr[j], e = rptr[j + 1]; k < e; ++k) q += vf[rattr[k]] * rx[k];
    rb[2 * (size_t)j].w = q;
}

__global__ __launch_bounds__(256) void k_fmr_addq(const uint32_t* __restrict__ map, uint64_t n,
                                                  const double4* __restrict__ rb, double2* __restrict__ eq) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < n) eq[c].y += rb[2 * (size_t)map[c]].w;
}

// one block row per thread, in the reference's accumulation order (fmg.h)
__global__ __launch_bounds__(256) void k_fmr_block_predict(const uint32_t* __restrict__ rptr,
                                                           const uint32_t* __restrict__ rattr,
                                                           const float* __restrict__ rx, uint32_t nb,
                                                           const double* __restrict__ vT, const double* __restrict__ w,
                                                           uint32_t K, uint32_t Kp, int k1, double* __restrict__ qbf,
                                                           double* __restrict__ qs, double4* __restrict__ rb) {
#pragma clang fp contract(off)
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nb) return;
    const uint32_t k0 = rptr[j], ke = rptr[j + 1];
    double y = 0.0, q2 = 0.0;
    for (uint32_t f = 0; f < K; ++f) {
        double q = 0.0;
        for (uint32_t k = k0; k < ke; ++k) {
            const double v = vT[(size_t)rattr[k] * Kp + f];
            const float x = rx[k];
            q += v * x;
            q2 -= 0.5 * v * v * x * x;
        }
        qbf[(size_t)j * K + f] = q;
        y += 0.5 * q * q;
    }
    if (k1)
        for (uint32_t k = k0; k < ke; ++k) q2 += w[rattr[k]] * rx[k];
    qs[j] = q2;
    double4 r0 = rb[2 * (size_t)j];
    r0.y = y + q2;
    r0.w = 0.0;
    rb[2 * (size_t)j] = r0;
}

__global__ __launch_bounds__(256) void k_fmg_q(const uint32_t* __restrict__ cptr, const uint32_t* __restrict__ cattr,
                                               const float* __restrict__ cx, uint64_t n,
                                               const double* __restrict__ vf, double2* __restrict__ eq) {
#pragma clang fp contract(off)
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    double q = 0.0;
    for (uint32_t j = cptr[c], e = cptr[c + 1]; j < e; ++j) q += vf[cattr[j]] * cx[j];
    eq[c].y = q;
}

__global__ __launch_bounds__(256) void k_fmg_esums(const double2* __restrict__ eq, uint64_t n, double w0,
                                                   double* __restrict__ part) {
    fm_esums_body(eq, n, w0, part);
}

__global__ __launch_bounds__(256) void k_fmg_shift(double2* __restrict__ eq, uint64_t n, double d) {
    fm_shift_body(eq, n, d);
}

// prediction of case c: e = sum_f 1/2 q_f^2 with q_f over the case's entries in ascending
// attribute order, q2 = - sum_f sum_j 1/2 v^2 x^2 (f outer, as the reference's second loop)
// + sum_j w x, then e + q2 (+ w0).  The two f loops share their loads: e and q2 are
// separate accumulators, each still added to in the reference's order.
template <bool REL = false>
__device__ __forceinline__ double fg_pred(const FGPredictArgs& a, uint64_t c) {
#pragma clang fp contract(off)
    const uint32_t j0 = a.cptr[c], j1 = a.cptr[c + 1];
    uint32_t br[FG_MAX_REL];  // REL: the case's block rows
    if constexpr (REL) {
#pragma unroll
        for (uint32_t r = 0; r < FG_MAX_REL; ++r) br[r] = r < a.nrel ? a.rel[r].map[c] : 0u;
    }
    double e = 0.0, q2 = 0.0;
    for (uint32_t f = 0; f < a.K; ++f) {
        double q = 0.0;
        for (uint32_t j = j0; j < j1; ++j) {
            const double v = a.vT[(size_t)a.cattr[j] * a.Kp + f];
            const float x = a.cx[j];
            q += v * x;
            q2 -= 0.5 * v * v * x * x;
        }
        if constexpr (REL) {  // q_all = q^M_f + sum_r q^B_f (:202-206)
#pragma unroll
            for (uint32_t r = 0; r < FG_MAX_REL; ++r)
                if (r < a.nrel) q += a.rel[r].qbf[(size_t)br[r] * a.K + f];
        }
        e += 0.5 * q * q;
    }
    if (a.k1)
        for (uint32_t j = j0; j < j1; ++j) q2 += a.w[a.cattr[j]] * a.cx[j];
    if constexpr (REL) {  // the blocks' q-terms (:327-330)
#pragma unroll
        for (uint32_t r = 0; r < FG_MAX_REL; ++r)
            if (r < a.nrel) q2 += a.rel[r].qs[br[r]];
    }
    e = e + q2;
    if (a.k0) e += a.w0;
    return e;
}

__global__ __launch_bounds__(256) void k_fmg_predict_train(FGPredictArgs a, double2* __restrict__ eq,
                                                           double* __restrict__ part) {
    fm_train_frame(a, a.n, a.y, part, [&](uint64_t c) { return fg_pred(a, c); },
                   [&](uint64_t c, double r) { eq[c] = make_double2(r, 0.0); });
}

__global__ __launch_bounds__(256) void k_fmg_predict_test(FGPredictArgs a, double it1, double* __restrict__ pthis,
                                                          double* __restrict__ sum_all, double* __restrict__ part) {
    fm_test_frame(a, a.n, a.y, it1, pthis, sum_all, part, [&](uint64_t t) { return fg_pred(a, t); });
}

// the classification frames (fm_dev.h) on this layout; TM: how the latent target is formed
template <int TM>
__global__ __launch_bounds__(256) void k_fmg_class_train(FGPredictArgs a, FMTargetArgs ta, double2* __restrict__ eq) {
    fm_class_train_frame<TM>(ta, a.n, a.y, [&](uint64_t c) { return fg_pred(a, c); },
                             [&](uint64_t c, double r) { eq[c] = make_double2(r, 0.0); });
}

__global__ __launch_bounds__(256) void k_fmg_class_test(FGPredictArgs a, double it1, double* __restrict__ pthis,
                                                        double* __restrict__ sum_all, uint32_t* __restrict__ cnt,
                                                        double* __restrict__ ll) {
    fm_class_test_frame(a.n, a.y, it1, pthis, sum_all, cnt, ll, [&](uint64_t t) { return fg_pred(a, t); });
}

// the four frames of a context with relations: the cases' terms plus their block rows' (fg_pred<true>)
__global__ __launch_bounds__(256) void k_fmr_predict_train(FGPredictArgs a, double2* __restrict__ eq,
                                                           double* __restrict__ part) {
    fm_train_frame(a, a.n, a.y, part, [&](uint64_t c) { return fg_pred<true>(a, c); },
                   [&](uint64_t c, double r) { eq[c] = make_double2(r, 0.0); });
}

__global__ __launch_bounds__(256) void k_fmr_predict_test(FGPredictArgs a, double it1, double* __restrict__ pthis,
                                                          double* __restrict__ sum_all, double* __restrict__ part) {
    fm_test_frame(a, a.n, a.y, it1, pthis, sum_all, part, [&](uint64_t t) { return fg_pred<true>(a, t); });
}

template <int TM>
__global__ __launch_bounds__(256) void k_fmr_class_train(FGPredictArgs a, FMTargetArgs ta, double2* __restrict__ eq) {
    fm_class_train_frame<TM>(ta, a.n, a.y, [&](uint64_t c) { return fg_pred<true>(a, c); },
                             [&](uint64_t c, double r) { eq[c] = make_double2(r, 0.0); });
}

__global__ __launch_bounds__(256) void k_fmr_class_test(FGPredictArgs a, double it1, double* __restrict__ pthis,
                                                        double* __restrict__ sum_all, uint32_t* __restrict__ cnt,
                                                        double* __restrict__ ll) {
    fm_class_test_frame(a.n, a.y, it1, pthis, sum_all, cnt, ll, [&](uint64_t t) { return fg_pred<true>(a, t); });
}

__global__ __launch_bounds__(256) void k_fmg_sub(double2* __restrict__ eq, uint64_t n, const double* __restrict__ t) {
    fm_sub_body(eq, n, t);
}

template <int MODE, bool GR>
hipError_t launch_pass(const FGPassArgs& a, int tpr, hipStream_t st) {
    if (a.nrows == 0) return hipSuccess;
    if (a.xmode != 0 && !a.chunks) return hipErrorInvalidValue;
    if (GR && (!a.lm || (a.grp_bytes != 1 && a.grp_bytes != 2 && a.grp_bytes != 4))) return hipErrorInvalidValue;
    return fm_launch_rows(tpr, a.nrows, [&](auto nt, dim3 grid, dim3 block) {
        constexpr int NT = decltype(nt)::value;
        if (GR)
            k_fmg_gpass<MODE, NT><<<grid, block, 0, st>>>(a);
        else
            k_fmg_pass<MODE, NT><<<grid, block, 0, st>>>(a);
    });
}

template <int MODE, bool GR>
hipError_t launch_rel_pass(const FGPassArgs& a, int tpr, hipStream_t st) {
    if (a.nrows == 0) return hipSuccess;
    if (!a.rb || (a.xmode != 0 && !a.chunks)) return hipErrorInvalidValue;
    if (GR && (!a.lm || (a.grp_bytes != 1 && a.grp_bytes != 2 && a.grp_bytes != 4))) return hipErrorInvalidValue;
    return fm_launch_rows(tpr, a.nrows, [&](auto nt, dim3 grid, dim3 block) {
        constexpr int NT = decltype(nt)::value;
        if (GR)
            k_fmr_gpass<MODE, NT><<<grid, block, 0, st>>>(a);
        else
            k_fmr_pass<MODE, NT><<<grid, block, 0, st>>>(a);
    });
}

// The grouped form of k_fmm_hsums (fmm.hip): block (c, g) runs the two chains (fm_chains_body) of
// group g of column c in 1024-value chunks (32 KiB of LDS: four groups' workgroups share a CU's
// 160 KiB where k_fmm_hsums' 64 KiB admit two).  A contiguous group reads its range, any other
// gathers through its ascending member list.
__global__ __launch_bounds__(256) void k_fmg_gsums(const double* __restrict__ v, const double* __restrict__ w,
                                                   uint32_t p, uint32_t K, uint32_t G,
                                                   const uint32_t* __restrict__ gptr, const uint32_t* __restrict__ gidx,
                                                   const uint32_t* __restrict__ gfirst, const double2* __restrict__ mg,
                                                   double2* __restrict__ out) {
    const uint32_t c = blockIdx.x, g = blockIdx.y;
    const double* __restrict__ x = c < K ? v + (size_t)c * p : w;
    const uint32_t b0 = gptr[g], cnt = gptr[g + 1] - b0, first = gfirst[g];
    const size_t cg = (size_t)c * G + g;
    const double2 in = mg[cg];
    fm_chains_body<1024, uint32_t>(cnt, &in, out, cg, [&](uint32_t q) {
        const uint32_t at = first != 0xffffffffu ? first + q : gidx[b0 + q];
        double t = 0.0;
        if (at < p) t = x[at];
        return t;
    });
}

}  // namespace

hipError_t fmg_wpass(const FGPassArgs& a, int tpr, hipStream_t st) {
    return a.grp ? launch_pass<0, true>(a, tpr, st) : launch_pass<0, false>(a, tpr, st);
}
hipError_t fmg_vpass(const FGPassArgs& a, int tpr, hipStream_t st) {
    return a.grp ? launch_pass<1, true>(a, tpr, st) : launch_pass<1, false>(a, tpr, st);
}

hipError_t fmg_group_sums(const double* v, const double* w, uint32_t p, uint32_t K, uint32_t G, const uint32_t* gptr,
                          const uint32_t* gidx, const uint32_t* gfirst, const double2* mg, double2* out, hipStream_t st) {
    if (G == 0 || G > 65535u) return hipErrorInvalidValue;  // the grid's y extent
    k_fmg_gsums<<<dim3(K + 1, G), 256, 0, st>>>(v, w, p, K, G, gptr, gidx, gfirst, mg, out);
    return hipGetLastError();
}

hipError_t fmg_chunk_draw(const FGPassArgs& a, const uint32_t* rows, const uint32_t* cfirst, uint32_t nlong,
                          const double2* csums, int vpass, double4* delta, hipStream_t st) {
    if (nlong == 0) return hipSuccess;
    if (a.grp && (!a.lm || (a.grp_bytes != 1 && a.grp_bytes != 2 && a.grp_bytes != 4))) return hipErrorInvalidValue;
    const dim3 grid((nlong + 255) / 256);
    if (vpass && a.grp)
        k_fmg_gchunk_draw<1><<<grid, 256, 0, st>>>(a, rows, cfirst, nlong, csums, delta);
    else if (vpass)
        k_fmg_chunk_draw<1><<<grid, 256, 0, st>>>(a, rows, cfirst, nlong, csums, delta);
    else if (a.grp)
        k_fmg_gchunk_draw<0><<<grid, 256, 0, st>>>(a, rows, cfirst, nlong, csums, delta);
    else
        k_fmg_chunk_draw<0><<<grid, 256, 0, st>>>(a, rows, cfirst, nlong, csums, delta);
    return hipGetLastError();
}

hipError_t fmg_rel_wpass(const FGPassArgs& a, int tpr, hipStream_t st) {
    return a.grp ? launch_rel_pass<0, true>(a, tpr, st) : launch_rel_pass<0, false>(a, tpr, st);
}
hipError_t fmg_rel_vpass(const FGPassArgs& a, int tpr, hipStream_t st) {
    return a.grp ? launch_rel_pass<1, true>(a, tpr, st) : launch_rel_pass<1, false>(a, tpr, st);
}

hipError_t fmg_rel_gather(const FGRelArgs& a, int vstep, int tpr, hipStream_t st) {
    if (a.nrows == 0) return hipSuccess;
    if (a.chunks && !a.sums) return hipErrorInvalidValue;
    return fm_launch_rows(tpr, a.nrows, [&](auto nt, dim3 grid, dim3 block) {
        constexpr int NT = decltype(nt)::value;
        if (vstep)
            k_fmr_gather<1, NT><<<grid, block, 0, st>>>(a);
        else
            k_fmr_gather<0, NT><<<grid, block, 0, st>>>(a);
    });
}

hipError_t fmg_rel_gather_combine(const uint32_t* rows, const uint32_t* cfirst, uint32_t nlong, const double4* sums,
                                  int vstep, double4* rb, hipStream_t st) {
    if (nlong == 0) return hipSuccess;
    if (vstep)
        k_fmr_gather_combine<1><<<(nlong + 255) / 256, 256, 0, st>>>(rows, cfirst, nlong, sums, rb);
    else
        k_fmr_gather_combine<0><<<(nlong + 255) / 256, 256, 0, st>>>(rows, cfirst, nlong, sums, rb);
    return hipGetLastError();
}

hipError_t fmg_rel_sync(const uint32_t* map, uint64_t n, const double4* rb, double2* eq, int vstep, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (vstep)
        k_fmr_sync<1><<<grid, 256, 0, st>>>(map, n, rb, eq);
    else
        k_fmr_sync<0><<<grid, 256, 0, st>>>(map, n, rb, eq);
    return hipGetLastError();
}

hipError_t fmg_rel_q(const uint32_t* rptr, const uint32_t* rattr, const float* rx, uint32_t nb, const double* vf,
                     double4* rb, hipStream_t st) {
    if (nb == 0) return hipSuccess;
    k_fmr_q<<<(nb + 255) / 256, 256, 0, st>>>(rptr, rattr, rx, nb, vf, rb);
    return hipGetLastError();
}

hipError_t fmg_rel_addq(const uint32_t* map, uint64_t n, const double4* rb, double2* eq, hipStream_t st) {
    if (n == 0) return hipSuccess;
    k_fmr_addq<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(map, n, rb, eq);
    return hipGetLastError();
}

hipError_t fmg_rel_block_predict(const uint32_t* rptr, const uint32_t* rattr, const float* rx, uint32_t nb,
                                 const double* vT, const double* w, uint32_t K, uint32_t Kp, int k1, double* qbf,
                                 double* qs, double4* rb, hipStream_t st) {
    if (nb == 0) return hipSuccess;
    k_fmr_block_predict<<<(nb + 255) / 256, 256, 0, st>>>(rptr, rattr, rx, nb, vT, w, K, Kp, k1, qbf, qs, rb);
    return hipGetLastError();
}

hipError_t fmg_q(const uint32_t* cptr, const uint32_t* cattr, const float* cx, uint64_t n, const double* vf,
                 double2* eq, hipStream_t st) {
    if (n == 0) return hipSuccess;
    k_fmg_q<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(cptr, cattr, cx, n, vf, eq);
    return hipGetLastError();
}

hipError_t fmg_esums(const double2* eq, uint64_t n, double w0, double* part, hipStream_t st) {
    if (n == 0) return hipSuccess;
    k_fmg_esums<<<(unsigned)((n + 1023) / 1024), 256, 0, st>>>(eq, n, w0, part);
    return hipGetLastError();
}

hipError_t fmg_shift(double2* eq, uint64_t n, double d, hipStream_t st) {
    if (n == 0) return hipSuccess;
    k_fmg_shift<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(eq, n, d);
    return hipGetLastError();
}

hipError_t fmg_predict_train(const FGPredictArgs& a, double2* eq, double* part, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    if (a.nrel > FG_MAX_REL) return hipErrorInvalidValue;
    if (a.nrel)
        k_fmr_predict_train<<<(unsigned)((a.n + 255) / 256), 256, 0, st>>>(a, eq, part);
    else
        k_fmg_predict_train<<<(unsigned)((a.n + 255) / 256), 256, 0, st>>>(a, eq, part);
    return hipGetLastError();
}

hipError_t fmg_class_train(const FGPredictArgs& a, const FMTargetArgs& ta, double2* eq, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    const unsigned grid = (unsigned)((a.n + 255) / 256);
    if (a.nrel > FG_MAX_REL || (ta.mode == FM_TGT_HOST && !ta.yhat)) return hipErrorInvalidValue;
    if (ta.mode != FM_TGT_ALS && ta.mode != FM_TGT_PHILOX && ta.mode != FM_TGT_HOST) return hipErrorInvalidValue;
    if (a.nrel) {
        if (ta.mode == FM_TGT_ALS)
            k_fmr_class_train<FM_TGT_ALS><<<grid, 256, 0, st>>>(a, ta, eq);
        else if (ta.mode == FM_TGT_PHILOX)
            k_fmr_class_train<FM_TGT_PHILOX><<<grid, 256, 0, st>>>(a, ta, eq);
        else
            k_fmr_class_train<FM_TGT_HOST><<<grid, 256, 0, st>>>(a, ta, eq);
    } else if (ta.mode == FM_TGT_ALS) {
        k_fmg_class_train<FM_TGT_ALS><<<grid, 256, 0, st>>>(a, ta, eq);
    } else if (ta.mode == FM_TGT_PHILOX) {
        k_fmg_class_train<FM_TGT_PHILOX><<<grid, 256, 0, st>>>(a, ta, eq);
    } else {
        k_fmg_class_train<FM_TGT_HOST><<<grid, 256, 0, st>>>(a, ta, eq);
    }
    return hipGetLastError();
}

hipError_t fmg_class_test(const FGPredictArgs& a, double it1, double* pthis, double* sum_all, uint32_t* cnt, double* ll,
                          hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    if (a.nrel > FG_MAX_REL) return hipErrorInvalidValue;
    if (a.nrel)
        k_fmr_class_test<<<(unsigned)((a.n + 255) / 256), 256, 0, st>>>(a, it1, pthis, sum_all, cnt, ll);
    else
        k_fmg_class_test<<<(unsigned)((a.n + 255) / 256), 256, 0, st>>>(a, it1, pthis, sum_all, cnt, ll);
    return hipGetLastError();
}

hipError_t fmg_sub_targets(double2* eq, uint64_t n, const double* t, hipStream_t st) {
    if (n == 0) return hipSuccess;
    k_fmg_sub<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(eq, n, t);
    return hipGetLastError();
}

hipError_t fmg_predict_test(const FGPredictArgs& a, double it1, double* pthis, double* sum_all, double* part,
                            hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    if (a.nrel > FG_MAX_REL) return hipErrorInvalidValue;
    if (a.nrel)
        k_fmr_predict_test<<<(unsigned)((a.n + 255) / 256), 256, 0, st>>>(a, it1, pthis, sum_all, part);
    else
        k_fmg_predict_test<<<(unsigned)((a.n + 255) / 256), 256, 0, st>>>(a, it1, pthis, sum_all, part);
    return hipGetLastError();
}

}  // namespace sbmf
