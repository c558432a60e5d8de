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
#include <hip/hip_runtime.h>

#include "fmg.h"

namespace sbmf {
namespace {

__device__ __forceinline__ double wsum(double x) {  // xor butterfly: bit-identical in every lane
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

// The row's draw from its sums m = sum h e, s2 = sum h^2 (fm_learn_mcmc.h:680-710, :793-824);
// keep: a non-finite draw restores the old value (the reference returns before the update).
// GR: the prior is the row's group's (lm[grp[at]], one small load per row); else the launch's scalars.
template <int MODE, bool GR>
__device__ __forceinline__ double fmg_draw(const FGPassArgs& a, uint32_t at, double old, double m, double s2,
                                           bool& keep) {
#pragma clang fp contract(off)
    double lambda = a.lambda, mu = a.mu;
    if constexpr (GR) {
        const uint32_t g = a.grp_bytes == 1   ? static_cast<const uint8_t*>(a.grp)[at]
                           : a.grp_bytes == 2 ? static_cast<const uint16_t*>(a.grp)[at]
                                              : static_cast<const uint32_t*>(a.grp)[at];
        const double2 t = a.lm[g];
        lambda = t.x;
        mu = t.y;
    }
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
    uint32_t row, beg, n, di;
    if (a.chunks) {
        const uint4 ck = a.chunks[ri];
        row = ck.x;
        beg = ck.y;
        n = ck.z;
        di = ck.w;
    } else {
        row = a.rows[ri];
        beg = a.aptr[row];
        n = a.aptr[row + 1] - beg;
        di = 0;
    }
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
        m = wsum(m);
        s2 = wsum(s2);
        if constexpr (NWR > 1) {  // waves of the row meet in LDS, summed in wave order
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

// long rows in chunks: one thread per long row, chunk sums in chunk order, then the draw
template <int MODE, bool GR>
__device__ __forceinline__ void fmg_chunk_draw_body(const FGPassArgs& a, const uint32_t* __restrict__ rows,
                                                    const uint32_t* __restrict__ cfirst, uint32_t nlong,
                                                    const double2* __restrict__ csums, double4* __restrict__ delta) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nlong) return;
    double m = 0.0, s2 = 0.0;
    for (uint32_t c = cfirst[i]; c < cfirst[i + 1]; ++c) {
        m += csums[c].x;
        s2 += csums[c].y;
    }
    const uint32_t at = rows[i];
    const double old = a.own[at];
    bool keep;
    const double nv = fmg_draw<MODE, GR>(a, at, old, m, s2, keep);
    a.own[at] = nv;
    delta[i] = make_double4(old, nv, keep ? 1.0 : 0.0, 0.0);
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
    const uint64_t b0 = (uint64_t)blockIdx.x * 1024;
    double s = 0.0, d = 0.0;
    for (int k = 0; k < 4; ++k) {
        const uint64_t q = b0 + k * 256 + threadIdx.x;
        if (q < n) {
            const double v = eq[q].x;
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

__global__ __launch_bounds__(256) void k_fmg_shift(double2* __restrict__ eq, uint64_t n, double d) {
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (q < n) eq[q].x -= d;
}

// prediction of case c: e = sum_f 1/2 q_f^2 with q_f over the case's entries in ascending
// attribute order, q2 = - sum_f sum_j 1/2 v^2 x^2 (f outer, as the reference's second loop)
// + sum_j w x, then e + q2 (+ w0).  The two f loops share their loads: e and q2 are
// separate accumulators, each still added to in the reference's order.
__device__ __forceinline__ double fg_pred(const FGPredictArgs& a, uint64_t c) {
#pragma clang fp contract(off)
    const uint32_t j0 = a.cptr[c], j1 = a.cptr[c + 1];
    double e = 0.0, q2 = 0.0;
    for (uint32_t f = 0; f < a.K; ++f) {
        double q = 0.0;
        for (uint32_t j = j0; j < j1; ++j) {
            const double v = a.vT[(size_t)a.cattr[j] * a.Kp + f];
            const float x = a.cx[j];
            q += v * x;
            q2 -= 0.5 * v * v * x * x;
        }
        e += 0.5 * q * q;
    }
    if (a.k1)
        for (uint32_t j = j0; j < j1; ++j) q2 += a.w[a.cattr[j]] * a.cx[j];
    e = e + q2;
    if (a.k0) e += a.w0;
    return e;
}

__device__ __forceinline__ double clampd(double p, double lo, double hi) {
    p = p < hi ? p : hi;     // std::min(max_target, p)
    return p > lo ? p : lo;  // std::max(min_target, p)
}

__device__ __forceinline__ double block_sum(double s, double* red) {  // 256 threads, fixed order
    s = wsum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void k_fmg_predict_train(FGPredictArgs a, double2* __restrict__ eq,
                                                           double* __restrict__ part) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    double se = 0.0;
    if (c < a.n) {
        const double pr = fg_pred(a, c);
        const double err = clampd(pr, a.lo, a.hi) - a.y[c];
        se = err * err;
        eq[c] = make_double2(pr - a.y[c], 0.0);
    }
    __shared__ double red[4];
    se = block_sum(se, red);
    if (threadIdx.x == 0) part[blockIdx.x] = se;
}

__global__ __launch_bounds__(256) void k_fmg_predict_test(FGPredictArgs a, double it1, double* __restrict__ pthis,
                                                          double* __restrict__ sum_all, double* __restrict__ part) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    double sa = 0.0, st = 0.0;
    if (t < a.n) {
        const double pr = fg_pred(a, t);
        pthis[t] = pr;
        const double s = sum_all[t] + clampd(pr, a.lo, a.hi);
        sum_all[t] = s;
        const double ea = clampd(s * (1.0 / it1), a.lo, a.hi) - a.y[t];  // _evaluate: pred * normalizer
        const double et = clampd(pr * 1.0, a.lo, a.hi) - a.y[t];
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

template <int MODE, bool GR>
hipError_t launch_pass(const FGPassArgs& a, int tpr, hipStream_t st) {
    if (a.nrows == 0) return hipSuccess;
    if (a.xmode != 0 && !a.chunks) return hipErrorInvalidValue;
    if (GR && (!a.lm || (a.grp_bytes != 1 && a.grp_bytes != 2 && a.grp_bytes != 4))) return hipErrorInvalidValue;
    switch (tpr) {
        case 64:
            if (GR)
                k_fmg_gpass<MODE, 64><<<(a.nrows + 3) / 4, 256, 0, st>>>(a);
            else
                k_fmg_pass<MODE, 64><<<(a.nrows + 3) / 4, 256, 0, st>>>(a);
            break;
        case 256:
            if (GR)
                k_fmg_gpass<MODE, 256><<<a.nrows, 256, 0, st>>>(a);
            else
                k_fmg_pass<MODE, 256><<<a.nrows, 256, 0, st>>>(a);
            break;
        case 1024:
            if (GR)
                k_fmg_gpass<MODE, 1024><<<a.nrows, 1024, 0, st>>>(a);
            else
                k_fmg_pass<MODE, 1024><<<a.nrows, 1024, 0, st>>>(a);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// The grouped form of k_fmm_hsums (fmm.hip): block (c, g) runs the two chains of group g of
// column c.  The workgroup stages 1024-value chunks of the group's values and their squared
// deviations in LDS (double-buffered, 32 KiB: four groups' workgroups share a CU's 160 KiB where
// k_fmm_hsums' 64 KiB admit two); lane 0 runs the gm chain and lane 1 the m chain.  A contiguous
// group reads its range, any other gathers through its ascending member list.
__global__ __launch_bounds__(256) void k_fmg_gsums(const double* __restrict__ v, const double* __restrict__ w,
                                                   uint32_t p, uint32_t K, uint32_t G,
                                                   const uint32_t* __restrict__ gptr, const uint32_t* __restrict__ gidx,
                                                   const uint32_t* __restrict__ gfirst, const double2* __restrict__ mg,
                                                   double2* __restrict__ out) {
#pragma clang fp contract(off)
    constexpr uint32_t CH = 1024;
    __shared__ __align__(16) double xs[2][CH];
    __shared__ __align__(16) double ds[2][CH];
    const uint32_t c = blockIdx.x, g = blockIdx.y;
    const double* __restrict__ x = c < K ? v + (size_t)c * p : w;
    const uint32_t b0 = gptr[g], cnt = gptr[g + 1] - b0, first = gfirst[g];
    const double2 in = mg[(size_t)c * G + g];
    const double mu = in.x;
    double acc = threadIdx.x == 0 ? in.y : 0.0;  // lane 0: gm, lane 1: m
    const uint32_t nch = (cnt + CH - 1) / CH;
    auto stage = [&](uint32_t ch, int b) {
        for (uint32_t i = threadIdx.x; i < CH; i += 256) {
            const uint32_t q = ch * CH + i;
            double t = 0.0;
            if (q < cnt) {
                const uint32_t at = first != 0xffffffffu ? first + q : gidx[b0 + q];
                if (at < p) t = x[at];
            }
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
    if (threadIdx.x == 0) out[(size_t)c * G + g] = make_double2(res[0], res[1]);
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
    k_fmg_predict_train<<<(unsigned)((a.n + 255) / 256), 256, 0, st>>>(a, eq, part);
    return hipGetLastError();
}

hipError_t fmg_predict_test(const FGPredictArgs& a, double it1, double* pthis, double* sum_all, double* part,
                            hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    k_fmg_predict_test<<<(unsigned)((a.n + 255) / 256), 256, 0, st>>>(a, it1, pthis, sum_all, part);
    return hipGetLastError();
}

}  // namespace sbmf
