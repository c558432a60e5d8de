// foldin_dev.h -- device code shared by the fold-in row kernel (k_foldin, foldin.hip) and the
// sample store's guest kernels (k_samples_foldin, k_samples_foldin_step, samples_foldin.hip): one
// coordinate scan of a guest's factor row against one V, the row, its normals and [sg | mu] in LDS.
// Both files run the same operations in the same order, so a stored sample's guest row is the
// in-chain draw of that sweep bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "foldin.h"
#include "rng.h"

namespace sbmf {

typedef double fd4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ void fload4(const T* p, double (&b)[4]);
template <>
__device__ __forceinline__ void fload4<double>(const double* p, double (&b)[4]) {
    const double2 x = *reinterpret_cast<const double2*>(p), y = *reinterpret_cast<const double2*>(p + 2);
    b[0] = x.x, b[1] = x.y, b[2] = y.x, b[3] = y.y;
}
template <>
__device__ __forceinline__ void fload4<float>(const float* p, double (&b)[4]) {
    const float4 x = *reinterpret_cast<const float4*>(p);
    b[0] = (double)x.x, b[1] = (double)x.y, b[2] = (double)x.z, b[3] = (double)x.w;
}

// One workgroup of FOLDIN_NW = 16 waves per guest, the longest guests first (order[]): a guest
// is one chain of dependent steps, so the launch takes as long as its longest row, and the
// waves and the eight gathers a wave keeps in flight are what shorten that.
constexpr uint32_t FOLDIN_NW = 16, FOLDIN_NT = 64 * FOLDIN_NW, FOLDIN_UNROLL = 8;

// The workgroup's LDS (51,584 bytes): the row u, its normals and the [sg | mu] of the sweep, then
// the Gram block's per-wave parts and sums.
struct FoldinLds {
    double urow[FOLDIN_KP_MAX], zs[FOLDIN_KP_MAX], hyp[2 * FOLDIN_KP_MAX];
    double Gw[FOLDIN_NW][256], Gs[16 * 17], cw[FOLDIN_NW][4][16], cs[16], D[16];
};

// The scan's normals: z_k = Philox normal 256 scan + k of (seed, row g, sweep, TAG_GUEST); scan 0's
// are the in-chain list's.
__device__ __forceinline__ void foldin_normals(FoldinLds& L, uint64_t seed, uint32_t g, uint32_t sweep, uint32_t scan,
                                               uint32_t Kp, uint32_t tid) {
    for (uint32_t p = tid; p < Kp / 2; p += FOLDIN_NT)
        philox_normal_pair(seed, g, sweep, TAG_GUEST, 128 * scan + p, L.zs[2 * p], L.zs[2 * p + 1]);
}

// One scan of the row in L.urow over the guest's ng ratings (it, r; residual scratch e) against V;
// tid is threadIdx.x.
// On entry L.urow, L.zs and L.hyp are written and a barrier has passed; on exit L.urow holds the
// drawn row, visible to every thread, and nothing of L is read any more.  The residuals e_j sit
// in the guest's slice of the device scratch (a row may be longer than any LDS: the scan loops
// over it and holds none of it in registers).
// Per block of 16 columns k0..k0+15, with S the [n_g][16] slice of the rated items' V rows:
//   1. a wave takes every 16th vector of 4 ratings, eight of them per trip: lane l holds
//      S[4 vec + (l >> 4)][l & 15] -- 16 lanes read 128 contiguous bytes of a V row (f32: 64) -- and one MFMA f64 16x16x4
//      with A = B = that value adds the vector's part of S^T S: A[m][k] from lane m + 16 k,
//      B[k][n] from lane n + 16 k, D[(l >> 4) + 4 i][l & 15] in acc[i]
//      (tests/hip/mfma_layout.hip); c = S^T e by one FMA per lane
//   2. the waves' partial G and c are added in wave (then quarter-wave) order in LDS
//   3. wave 0 makes the 16 draws in order: lane m holds c_m, which after draw j < m loses
//      G[m][j] d_j -- the coordinate loop's residual update, seen through S^T
//   4. e_j -= S[j] . d, one thread per rating (its 128 bytes of the row again)
// Step 4 is skipped after the last block: nothing reads the residuals then.
template <typename T>
__device__ __forceinline__ void foldin_scan(FoldinLds& L, const uint32_t* __restrict__ it, const double* __restrict__ r,
                                            double* e, uint32_t ng, const T* __restrict__ V, uint32_t K, uint32_t Kp,
                                            double tau, int sd_is_var, uint32_t tid) {
    const uint32_t lane = tid & 63, wave = tid >> 6, col = lane & 15, q = lane >> 4;
    // e_j = r_j - u . v_j
    for (uint32_t j = tid; j < ng; j += FOLDIN_NT) {
        const T* vp = V + (size_t)it[j] * Kp;
        double s = 0.0;
        for (uint32_t k = 0; k < Kp; k += 4) {
            double b[4];
            fload4<T>(vp + k, b);
#pragma unroll
            for (int x = 0; x < 4; ++x) s = fma(L.urow[k + x], b[x], s);
        }
        e[j] = r[j] - s;
    }
    __syncthreads();
    for (uint32_t k0 = 0; k0 < Kp; k0 += 16) {
        // 1. this wave's part of G_B and c
        fd4 acc = fd4{0, 0, 0, 0};
        double cp = 0.0;
        for (uint32_t v0 = 4 * wave; v0 < ng; v0 += 4 * FOLDIN_NW * FOLDIN_UNROLL) {
            uint32_t row[FOLDIN_UNROLL];
            double v[FOLDIN_UNROLL], ej[FOLDIN_UNROLL];
#pragma unroll
            for (uint32_t x = 0; x < FOLDIN_UNROLL; ++x) {
                const uint32_t j = v0 + x * 4 * FOLDIN_NW + q;
                row[x] = j < ng ? it[j] : 0u;
            }
#pragma unroll
            for (uint32_t x = 0; x < FOLDIN_UNROLL; ++x) {
                const uint32_t j = v0 + x * 4 * FOLDIN_NW + q;
                v[x] = ej[x] = 0.0;
                if (j < ng) {  // a slot past the row adds zeros
                    v[x] = (double)V[(size_t)row[x] * Kp + k0 + col];
                    ej[x] = e[j];
                }
            }
#pragma unroll
            for (uint32_t x = 0; x < FOLDIN_UNROLL; ++x) {
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v[x], v[x], acc, 0, 0, 0);
                cp = fma(v[x], ej[x], cp);
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
            for (uint32_t w = 0; w < FOLDIN_NW; ++w) s += L.Gw[w][tid];
            L.Gs[(tid >> 4) * 17 + (tid & 15)] = s;
        }
        if (tid < 16) {
            double s = 0.0;
#pragma unroll
            for (uint32_t w = 0; w < FOLDIN_NW; ++w)
#pragma unroll
                for (int x = 0; x < 4; ++x) s += L.cw[w][x][tid];
            L.cs[tid] = s;
        }
        __syncthreads();
        // 3. the block's 16 draws (every quarter of wave 0 computes them; the first one stores)
        if (wave == 0) {
            const uint32_t k = k0 + col;
            const bool kin = k < K;
            const double P = L.Gs[col * 17 + col], uo = L.urow[k];
            const double sg = L.hyp[k], mu = L.hyp[FOLDIN_KP_MAX + k], z = L.zs[k];
            const double var = kin ? 1.0 / (sg + tau * P) : 0.0;
            const double sd = sd_is_var ? var : sqrt(var);
            double cm = L.cs[col], un = 0.0;
            for (uint32_t j = 0; j < 16; ++j) {
                // lane j's c is final here: c_j = sum v_jk e_j with the earlier draws applied
                const double Q = cm + P * uo;
                const double mean = var * (tau * Q + sg * mu);
                const double cand = kin ? mean + sd * z : 0.0;
                const double dj = __shfl(cand - uo, (int)j, 16);
                if (col == j) un = cand;
                if (col > j) cm -= L.Gs[col * 17 + j] * dj;
            }
            if (q == 0) {
                L.urow[k] = un;
                L.D[col] = un - uo;
            }
        }
        __syncthreads();
        // 4. the residuals
        if (k0 + 16 < Kp) {
            for (uint32_t j = tid; j < ng; j += FOLDIN_NT) {
                const T* vp = V + (size_t)it[j] * Kp + k0;
                double s = 0.0;
#pragma unroll
                for (int x4 = 0; x4 < 16; x4 += 4) {
                    double b[4];
                    fload4<T>(vp + x4, b);
#pragma unroll
                    for (int x = 0; x < 4; ++x) s = fma(b[x], L.D[x4 + x], s);
                }
                e[j] -= s;
            }
            __syncthreads();
        }
    }
}

}  // namespace sbmf
