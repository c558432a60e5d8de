// vb_lists.hip -- gfx950 kernels of the online VB learner's lists (vb_lists.h):
//   k_vb_score  rows x all items, mean and variance from one pass over the item tables
//               (MFMA f64 16x16x4, three chains per k step into two accumulators)
//   k_vb_pairs  (user, item) pairs, 16 lanes per pair in k_predict's order
//   k_vb_sd     a row of variances to standard deviations
//   k_vb_guest  a guest's posterior from its ratings, one workgroup per guest
// The selection is recommend.hip's (launch_watch_select_given).
#include "vb_lists.h"

#include <cmath>
#include <cstdlib>

#include "recommend.h"
#include "recommend_dev.h"

namespace sbmf {
namespace {

// ------------------------------------------------------------------ scoring
// The watch list's scoring kernel (k_watch_accum, recommend.hip) with two accumulators per row
// group: a workgroup of four waves takes 16 MU rows and VB_TILES item tiles of 16; it stages the
// rows' mu, mu^2 + s and s in LDS (rows of Kp + 2 doubles: the 16 rows a quarter wave reads 16
// bytes of fall on different banks); a wave takes every fourth item tile.  watch_tile_products'
// operand layout: A[m][k] from lane m + 16 k (the rows, from LDS), B[k][n] from lane n + 16 k (the
// items, from memory), D[(l >> 4) + 4 j][l & 15] in acc[j]; a lane loads four consecutive k at
// once, step s multiplies column 4 (l >> 4) + s of both operands.  Per k step, from one load of the
// item's mu and s:
//   accM += mu_u . mu_j            accV += (mu_u^2 + s_u) . s_j           accV += s_u . mu_j^2
// (mu_j^2 formed in registers), so accV = sum_f (s_u s_j + mu_u^2 s_j + s_u mu_j^2).  The padding
// columns of every table are zero.  The epilogue adds the biases and the global bias in
// k_predict's association and writes: no old value is read.
constexpr uint32_t VB_TILES = 16;

template <int MU>
__global__ __launch_bounds__(256) void k_vb_score(VBRows rows, uint32_t n, VBItems it, uint32_t Jp,
                                                  double* __restrict__ M, double* __restrict__ Vr) {
    extern __shared__ double lds[];  // um, uq, us: [16 MU][Kp + 2] each, then the rows' ids
    const uint32_t Kp = it.Kp, J = it.J, ld = Kp + 2;
    double* um = lds;
    double* uq = um + (size_t)16 * MU * ld;
    double* us = uq + (size_t)16 * MU * ld;
    uint32_t* uid = reinterpret_cast<uint32_t*>(us + (size_t)16 * MU * ld);
    const uint32_t w0 = blockIdx.x * 16 * MU;
    if (threadIdx.x < 16 * MU)
        uid[threadIdx.x] = w0 + threadIdx.x < n ? (rows.ids ? rows.ids[w0 + threadIdx.x] : w0 + threadIdx.x) : 0u;
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < 16 * MU * Kp; x += 256) {
        const uint32_t r = x / Kp, k = x - r * Kp;
        const bool ok = w0 + r < n;
        const double m = ok ? rows.mu[(size_t)uid[r] * Kp + k] : 0.0, s = ok ? rows.sg[(size_t)uid[r] * Kp + k] : 0.0;
        um[r * ld + k] = m;
        uq[r * ld + k] = m * m + s;
        us[r * ld + k] = s;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n16 = lane & 15, kq = lane >> 4;
    const uint32_t ntile = Jp / 16;
    const uint32_t tend = min(ntile, (blockIdx.y + 1) * VB_TILES);
    const double mu0 = it.scal->mu0, sg0 = it.scal->sg0;
    for (uint32_t tile = blockIdx.y * VB_TILES + wave; tile < tend; tile += 4) {
        const uint32_t item = tile * 16 + n16;
        const size_t vo = (size_t)min(item, J - 1) * Kp + 4 * kq;  // a padding item reads the last row (not stored)
        const double *vm = it.mu + vo, *vs = it.sg + vo;
        wd4 accM[MU], accV[MU];
#pragma unroll
        for (int t = 0; t < MU; ++t) accM[t] = accV[t] = wd4{0, 0, 0, 0};
        for (uint32_t k0 = 0; k0 < Kp; k0 += 16) {
            double bm[4], bs[4], bq[4];
            load4<double>(vm + k0, bm);
            load4<double>(vs + k0, bs);
#pragma unroll
            for (int s = 0; s < 4; ++s) bq[s] = bm[s] * bm[s];
#pragma unroll
            for (int t = 0; t < MU; ++t) {
                if (w0 + t * 16 >= n) continue;  // a row group past the list (uniform)
                const size_t ao = (size_t)(t * 16 + n16) * ld + k0 + 4 * kq;
                double am[4], aq[4], as[4];
                load4<double>(um + ao, am);
                load4<double>(uq + ao, aq);
                load4<double>(us + ao, as);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    accM[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(am[s], bm[s], accM[t], 0, 0, 0);
                    accV[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(aq[s], bs[s], accV[t], 0, 0, 0);
                    accV[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[s], bq[s], accV[t], 0, 0, 0);
                }
            }
        }
        if (item >= J) continue;
        const double wj = it.w_mu[item], sj = it.w_sg[item];
#pragma unroll
        for (int t = 0; t < MU; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t r = t * 16 + kq + 4 * j, w = w0 + r;
                if (w >= n) continue;
                const size_t o = (size_t)w * Jp + item;
                M[o] = ((accM[t][j] + rows.w_mu[uid[r]]) + wj) + mu0;
                Vr[o] = ((accV[t][j] + rows.w_sg[uid[r]]) + sj) + sg0;
            }
    }
}

template <int MU>
hipError_t vb_score_mu(const VBRows& rows, uint32_t n, const VBItems& it, double* M, double* Vr, hipStream_t st) {
    const uint32_t Jp = watch_jp(it.J);
    const dim3 grid((n + 16 * MU - 1) / (16 * MU), (Jp / 16 + VB_TILES - 1) / VB_TILES);
    const size_t lds = vb_score_lds_bytes(MU, it.Kp);
    if (lds > 64 * 1024) {  // MU = 1, Kp > 160: past the default limit of a launch's dynamic LDS
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_vb_score<MU>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    k_vb_score<MU><<<grid, 256, lds, st>>>(rows, n, it, Jp, M, Vr);
    return hipGetLastError();
}

// ------------------------------------------------------------------ pairs
// sum over the 16 lanes of a pair's group, lane 0's value broadcast (k_predict's sum16)
__device__ __forceinline__ double sum16(double x) {
    x += __shfl_xor(x, 8, 16);
    x += __shfl_xor(x, 4, 16);
    x += __shfl_xor(x, 2, 16);
    x += __shfl_xor(x, 1, 16);
    return __shfl(x, 0, 16);
}

// k_predict (vbo.hip) for any (user, item) pair: lane ci of the pair's 16 adds columns ci, 16 + ci,
// ... in order, then the butterfly; the mean is k_predict's r - e.
__global__ __launch_bounds__(256) void k_vb_pairs(const uint32_t* __restrict__ users, const uint32_t* __restrict__ items,
                                                  uint64_t n, const double* __restrict__ muT,
                                                  const double* __restrict__ sgT, VBTables tb, uint32_t Kp,
                                                  double* __restrict__ mean, double* __restrict__ sd,
                                                  double* __restrict__ var) {
    const uint64_t q = (uint64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int ci = threadIdx.x & 15;
    if (q >= n) return;  // whole 16-lane groups
    const uint32_t u = users[q], pa = tb.I + items[q];
    const uint32_t nb = Kp / 16;
    double d = 0.0, tv = 0.0;
    for (uint32_t b = 0; b < nb; ++b) {
        const double vu = muT[(size_t)u * Kp + 16 * b + ci], su = sgT[(size_t)u * Kp + 16 * b + ci];
        const double vi = muT[(size_t)pa * Kp + 16 * b + ci], si = sgT[(size_t)pa * Kp + 16 * b + ci];
        d += vu * vi;
        tv += su * si + su * (vi * vi) + si * (vu * vu);
    }
    d = sum16(d);
    tv = sum16(tv);
    if (ci == 0) {
        const double m = ((d + tb.mu_w[u]) + tb.mu_w[pa]) + tb.scal->mu0;
        const double v = ((tv + tb.sg_w[u]) + tb.sg_w[pa]) + tb.scal->sg0;
        double mo, so;
        watch_given_moments(m, v, mo, so);
        mean[q] = mo;
        if (sd) sd[q] = so;
        if (var) var[q] = v;
    }
}

__global__ __launch_bounds__(256) void k_vb_sd(const double* __restrict__ var, uint32_t n, double* __restrict__ sd) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double m, s;
    watch_given_moments(0.0, var[j], m, s);
    sd[j] = s;
}

// ------------------------------------------------------------------ guests
// One workgroup of 16 waves per guest, the longest guests first; the block structure of the
// fold-in scan (foldin_dev.h) without normals.  The residuals e_j sit in the guest's slice of the
// device scratch.  First, once (they do not depend on the scans), the precisions P_f = sigma_v[f]
// + alpha sum_j (mu_jf^2 + s_jf): every lane's and then every column's sum is kept as an unevaluated
// pair hi + lo (error-free additions, the square's error by an FMA), so P_f is the correctly rounded
// sum to within an ulp in whatever order the partials meet, and 1 / P_f a second rounding away.
// Per scan: the bias step (the residuals' sum: a lane's strided sum, the wave's butterfly, the
// waves in order), then per block of 16 columns k0 .. k0 + 15, with S the [n][16] slice of the
// rated items' means:
//   1. a wave takes every 16th vector of 4 ratings, four per trip (256 ratings a trip of the
//      workgroup): lane l holds S[4 vec + (l >> 4)][l & 15]; one MFMA with A = B = that value adds
//      the vector's part of S^T S; c = S^T e by one FMA per lane
//   2. the waves' partial G and c are added in wave (then quarter-wave) order
//   3. wave 0 makes the 16 updates in order: lane m holds c_m, which after update j < m loses
//      G[m][j] d_j: g_m <- alpha (c_m + G_mm g_m) / P_m
//   4. e_j -= S[j] . d, one thread per rating
// Step 4 is skipped after a scan's last block: the next scan takes its residuals afresh.
constexpr uint32_t VG_NW = 16, VG_NT = 64 * VG_NW, VG_UNROLL = 4;

struct VbGuestLds {
    double g[VB_GUEST_KP_MAX], P[VB_GUEST_KP_MAX];
    double Gw[VG_NW][256], Gs[16 * 17], cw[VG_NW][4][16], sw[VG_NW][4][16], cs[16], D[16], red[VG_NW];
};

// s + e = a + b exactly (Knuth's two-sum: no ordering of |a|, |b| needed)
__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

__global__ __launch_bounds__(1024) void k_vb_guest(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ items,
                                                   const double* __restrict__ ratings,
                                                   const uint32_t* __restrict__ order, double* __restrict__ E,
                                                   uint32_t scans, VBItems it, const double* __restrict__ sigma_v,
                                                   uint32_t K, double* __restrict__ GM, double* __restrict__ GS,
                                                   double* __restrict__ gb, double* __restrict__ gs) {
    __shared__ VbGuestLds L;
    const uint32_t g = order[blockIdx.x];
    const uint32_t p0 = ptr[g], ng = ptr[g + 1] - p0;
    const uint32_t* itj = items + p0;
    const double* r = ratings + p0;
    double* e = E + p0;
    const uint32_t Kp = it.Kp, tid = threadIdx.x;
    const uint32_t lane = tid & 63, wave = tid >> 6, col = lane & 15, q = lane >> 4;
    const double alpha = it.scal->alpha, mu0 = it.scal->mu0;
    const double Pb = it.scal->sigma_w + alpha * (double)ng;
    for (uint32_t k = tid; k < Kp; k += VG_NT) L.g[k] = 0.0;
    for (uint32_t j = tid; j < ng; j += VG_NT) e[j] = (r[j] - mu0) - it.w_mu[itj[j]];
    // 0. the precisions
    for (uint32_t k0 = 0; k0 < Kp; k0 += 16) {
        double hi = 0.0, lo = 0.0;
        for (uint32_t j = 4 * wave + q; j < ng; j += 4 * VG_NW) {
            const size_t o = (size_t)itj[j] * Kp + k0 + col;
            const double m = it.mu[o], sj = it.sg[o], mm = m * m;
            double t;
            two_sum(hi, mm, hi, t);
            lo += t + fma(m, m, -mm);
            two_sum(hi, sj, hi, t);
            lo += t;
        }
        L.cw[wave][q][col] = hi;
        L.sw[wave][q][col] = lo;
        __syncthreads();
        if (tid < 16) {
            const uint32_t k = k0 + tid;
            double H = 0.0, Lo = 0.0, t;
#pragma unroll 1
            for (uint32_t w = 0; w < VG_NW; ++w)
#pragma unroll
                for (int y = 0; y < 4; ++y) {
                    two_sum(H, L.cw[w][y][tid], H, t);
                    Lo += t + L.sw[w][y][tid];
                }
            // sigma_v + alpha (H + Lo), the product's and the sum's errors carried to the last addition
            const double pa = alpha * H, pe = fma(alpha, H, -pa) + alpha * Lo;
            double ps;
            two_sum(k < K ? sigma_v[k] : 1.0, pa, ps, t);
            L.P[k] = ps + (t + pe);
        }
        __syncthreads();
    }
    double b = 0.0;
    for (uint32_t scan = 0; scan < scans; ++scan) {
        // The residuals of b and g afresh, as foldin_scan takes them at a scan's start (the first
        // scan's are set above).  Carried over by increments alone they stop following an update
        // smaller than half their ulp while b keeps creeping towards (alpha / sigma_w) sum_j e_j:
        // 4.6 ulps of b after 64 scans at n = 256, against 1.6 this way.
        if (scan > 0) {
            for (uint32_t j = tid; j < ng; j += VG_NT) {
                const double* vp = it.mu + (size_t)itj[j] * Kp;
                double s = 0.0;
                for (uint32_t k = 0; k < Kp; k += 4) {
                    double bb[4];
                    load4<double>(vp + k, bb);
#pragma unroll
                    for (int y = 0; y < 4; ++y) s = fma(L.g[k + y], bb[y], s);
                }
                e[j] = (((r[j] - mu0) - it.w_mu[itj[j]]) - b) - s;
            }
            __syncthreads();
        }
        // the bias: b <- alpha sum_j (e_j + b) / P_b
        double x = 0.0;
        for (uint32_t j = tid; j < ng; j += VG_NT) x += e[j] + b;
        for (int m = 32; m > 0; m >>= 1) x += __shfl_xor(x, m, 64);
        if (lane == 0) L.red[wave] = x;
        __syncthreads();
        double tot = 0.0;
#pragma unroll
        for (uint32_t w = 0; w < VG_NW; ++w) tot += L.red[w];
        const double bn = alpha * tot / Pb, db = bn - b;
        for (uint32_t j = tid; j < ng; j += VG_NT) e[j] -= db;
        b = bn;
        __syncthreads();
        for (uint32_t k0 = 0; k0 < Kp; k0 += 16) {
            // 1. this wave's part of G and c
            wd4 acc = wd4{0, 0, 0, 0};
            double cp = 0.0;
            for (uint32_t v0 = 4 * wave; v0 < ng; v0 += 4 * VG_NW * VG_UNROLL) {
                uint32_t row[VG_UNROLL];
                double v[VG_UNROLL], ej[VG_UNROLL];
#pragma unroll
                for (uint32_t u = 0; u < VG_UNROLL; ++u) {
                    const uint32_t j = v0 + u * 4 * VG_NW + q;
                    row[u] = j < ng ? itj[j] : 0u;
                }
#pragma unroll
                for (uint32_t u = 0; u < VG_UNROLL; ++u) {
                    const uint32_t j = v0 + u * 4 * VG_NW + q;
                    v[u] = ej[u] = 0.0;
                    if (j < ng) {  // a slot past the row adds zeros
                        v[u] = it.mu[(size_t)row[u] * Kp + k0 + col];
                        ej[u] = e[j];
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < VG_UNROLL; ++u) {
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u], v[u], acc, 0, 0, 0);
                    cp = fma(v[u], ej[u], cp);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) L.Gw[wave][(q + 4 * i) * 16 + col] = acc[i];
            L.cw[wave][q][col] = cp;
            __syncthreads();
            // 2. the waves' sums, in wave order
            if (tid < 256) {
                double s = 0.0;
#pragma unroll
                for (uint32_t w = 0; w < VG_NW; ++w) s += L.Gw[w][tid];
                L.Gs[(tid >> 4) * 17 + (tid & 15)] = s;
            } else if (tid < 256 + 16) {
                const uint32_t c = tid & 15;
                double s = 0.0;
#pragma unroll
                for (uint32_t w = 0; w < VG_NW; ++w)
#pragma unroll
                    for (int y = 0; y < 4; ++y) s += L.cw[w][y][c];
                L.cs[c] = s;
            }
            __syncthreads();
            // 3. the block's 16 updates (every quarter of wave 0 computes them; the first one stores)
            if (wave == 0) {
                const uint32_t k = k0 + col;
                const bool kin = k < K;
                const double Gd = L.Gs[col * 17 + col], uo = L.g[k];
                const double P = L.P[k];
                double cm = L.cs[col], un = 0.0;
                for (uint32_t j = 0; j < 16; ++j) {
                    // lane j's c is final here: c_j = sum mu_jk e_j with the earlier updates applied
                    const double Q = cm + Gd * uo;
                    const double cand = kin ? alpha * Q / P : 0.0;
                    const double dj = __shfl(cand - uo, (int)j, 16);
                    if (col == j) un = cand;
                    if (col > j) cm -= L.Gs[col * 17 + j] * dj;
                }
                if (q == 0) {
                    L.g[k] = un;
                    L.D[col] = un - uo;
                }
            }
            __syncthreads();
            // 4. the residuals
            if (k0 + 16 < Kp) {
                for (uint32_t j = tid; j < ng; j += VG_NT) {
                    const double* vp = it.mu + (size_t)itj[j] * Kp + k0;
                    double s = 0.0;
#pragma unroll
                    for (int x4 = 0; x4 < 16; x4 += 4) {
                        double bb[4];
                        load4<double>(vp + x4, bb);
#pragma unroll
                        for (int y = 0; y < 4; ++y) s = fma(bb[y], L.D[x4 + y], s);
                    }
                    e[j] -= s;
                }
                __syncthreads();
            }
        }
    }
    for (uint32_t k = tid; k < Kp; k += VG_NT) {
        GM[(size_t)g * Kp + k] = L.g[k];
        GS[(size_t)g * Kp + k] = k < K ? 1.0 / L.P[k] : 0.0;
    }
    if (tid == 0) {
        gb[g] = b;
        gs[g] = 1.0 / Pb;
    }
}

}  // namespace

hipError_t launch_vb_score(const VBRows& rows, uint32_t n, const VBItems& it, double* M, double* Vr, hipStream_t st) {
    if (n == 0 || it.J == 0) return hipSuccess;
    int mu = vb_score_mu(it.Kp);
    // SBMF_VB_SCORE_MU=1|2|4 (measurements: profiles/vb_lists_bench.py): another row count, where the CU's LDS holds it
    if (const char* f = std::getenv("SBMF_VB_SCORE_MU")) {
        const int m = std::atoi(f);
        if ((m == 1 || m == 2 || m == 4) && vb_score_lds_bytes(m, it.Kp) <= 160 * 1024) mu = m;
    }
    switch (mu) {
        case 4:
            return vb_score_mu<4>(rows, n, it, M, Vr, st);
        case 2:
            return vb_score_mu<2>(rows, n, it, M, Vr, st);
    }
    return vb_score_mu<1>(rows, n, it, M, Vr, st);
}

hipError_t launch_vb_pairs(const uint32_t* users, const uint32_t* items, uint64_t n, const double* muT, const double* sgT,
                           const VBTables& tb, uint32_t Kp, double* mean, double* sd, double* var, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if ((n + 15) / 16 > 0x7fffffffull) return hipErrorInvalidValue;
    k_vb_pairs<<<(uint32_t)((n + 15) / 16), 256, 0, st>>>(users, items, n, muT, sgT, tb, Kp, mean, sd, var);
    return hipGetLastError();
}

hipError_t launch_vb_sd(const double* var, uint32_t n, double* sd, hipStream_t st) {
    if (n == 0) return hipSuccess;
    k_vb_sd<<<(n + 255) / 256, 256, 0, st>>>(var, n, sd);
    return hipGetLastError();
}

hipError_t launch_vb_guest(const uint32_t* ptr, const uint32_t* items, const double* ratings, const uint32_t* order,
                           double* E, uint32_t n, uint32_t scans, const VBItems& it, const double* sigma_v, uint32_t K,
                           double* GM, double* GS, double* gb, double* gs, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (it.Kp > VB_GUEST_KP_MAX || scans == 0) return hipErrorInvalidValue;
    k_vb_guest<<<n, VG_NT, 0, st>>>(ptr, items, ratings, order, E, scans, it, sigma_v, K, GM, GS, gb, gs);
    return hipGetLastError();
}

}  // namespace sbmf
