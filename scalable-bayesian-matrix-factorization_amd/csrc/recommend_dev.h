// recommend_dev.h -- device code the scoring kernels share (recommend.hip: k_watch_accum, one
// sample added to sums in memory; samples.hip: k_samples_score, every stored sample added to sums
// in registers): the MFMA tile product, a score's biases and clamp, the sums' update and the
// moments read from them.  One copy of each expression: the same product order and the same
// contraction give the same bits per sample in both kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace sbmf {

typedef double wd4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ void load4(const T* p, double (&b)[4]);
template <>
__device__ __forceinline__ void load4<double>(const double* p, double (&b)[4]) {
    const double2 x = *reinterpret_cast<const double2*>(p), y = *reinterpret_cast<const double2*>(p + 2);
    b[0] = x.x, b[1] = x.y, b[2] = y.x, b[3] = y.y;
}
template <>
__device__ __forceinline__ void load4<float>(const float* p, double (&b)[4]) {
    const float4 x = *reinterpret_cast<const float4*>(p);
    b[0] = (double)x.x, b[1] = (double)x.y, b[2] = (double)x.z, b[3] = (double)x.w;
}

// One item tile's products against the 16 MU rows a workgroup holds in LDS (`us`: rows of ld =
// Kp + 2 doubles), added to acc[MU].  MFMA f64 16x16x4, per step: A[m][k] from lane m + 16 k (the
// rows, from LDS), B[k][n] from lane n + 16 k (the items: vp is this lane's V row at column 4 kq,
// n16 = lane & 15, kq = lane >> 4), D[(l >> 4) + 4 j][l & 15] in acc[t][j].  A lane loads four
// consecutive k of its row at once: within a block of 16 k, step s multiplies column 4 kq + s of
// both operands, a fixed permutation of the k order.  Row group t is skipped when it lies past
// the list (w0 + 16 t >= n, uniform).  (acc as a pointer: taken by reference to the array, the
// compiler moved all MU accumulators of k_watch_accum into AGPRs and used more registers.)
template <typename T, int MU>
__device__ __forceinline__ void watch_tile_products(const double* us, uint32_t ld, const T* vp, uint32_t Kp, uint32_t w0,
                                                    uint32_t n, uint32_t n16, uint32_t kq, wd4* __restrict__ acc) {
    for (uint32_t k0 = 0; k0 < Kp; k0 += 16) {
        double b[4];
        load4<T>(vp + k0, b);
#pragma unroll
        for (int t = 0; t < MU; ++t) {
            if (w0 + t * 16 >= n) continue;  // a tile past the list (uniform)
            double a[4];
            load4<double>(us + (size_t)(t * 16 + n16) * ld + k0 + 4 * kq, a);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[s], acc[t], 0, 0, 0);
        }
    }
}

// a product with its biases (as k_test adds them), when there are any
__device__ __forceinline__ double watch_biased(double dot, bool biased, double b0, double bi, double bj) {
    return biased ? ((b0 + bi) + bj) + dot : dot;
}
__device__ __forceinline__ double watch_clamped(double s, int clamp, double lo, double hi) {
    if (clamp) {
        s = (s < hi) ? s : hi;
        s = (lo < s) ? s : lo;
    }
    return s;
}
// a sample's score joins the sums
__device__ __forceinline__ void watch_sums_add(double o1, double o2, double s, double& s1, double& s2) {
    s1 = o1 + s;
    s2 = o2 + s * s;
}

// One place for the expressions, without contraction: sbmf_watch_scores returns exactly the
// mean and stdev the selection ranks by, and a caller forming mean - risk * stdev from them in
// IEEE double arithmetic gets the selection's key bit for bit.
__device__ __forceinline__ void watch_moments(double s1, double s2, double nw, double& mean, double& sd) {
#pragma clang fp contract(off)
    mean = s1 / nw;
    const double mm = mean * mean;
    const double v = s2 / nw - mm;
    sd = sqrt(v > 0.0 ? v : 0.0);
}
// The same pair when the two rows ARE a mean and a variance (the online VB lists, vb_lists.hip:
// closed-form moments, no sums): s2 / nw - mean^2 of var + mean^2 would cancel to 0 wherever
// var << mean^2, the normal case of a converged posterior.
__device__ __forceinline__ void watch_given_moments(double m, double var, double& mean, double& sd) {
#pragma clang fp contract(off)
    mean = m;
    sd = sqrt(var > 0.0 ? var : 0.0);
}

}  // namespace sbmf
