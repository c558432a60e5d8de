// samples.hip -- gfx950 kernels of the posterior sample store (include/sbmf.h, sbmf_keep_samples):
//   k_samples_score  the scores of a list of users against every item, summed (and their squares)
//                    over every stored sample in one launch (MFMA f64 16x16x4)
//   k_samples_pairs  mean / stdev of (user, item) pairs over the stored samples
#include "samples.h"

#include "recommend_dev.h"

namespace sbmf {

__device__ __forceinline__ uint32_t ring_slot(uint32_t head, uint32_t s, uint32_t cap) {
    const uint32_t p = head + s;  // head < cap, s < cap <= 65535
    return p >= cap ? p - cap : p;
}

// ------------------------------------------------------------------ scores of users x items
// A workgroup of four waves takes 16 MU users and 4 SAMPLES_TW item tiles of 16; wave w owns
// tiles w, w + 4, ... of them and keeps their S1 / S2 -- 8 MU SAMPLES_TW doubles per lane -- in
// registers over the whole sample loop.  Per sample the workgroup stages its users' rows of that
// sample's U into LDS (as k_watch_accum does once per launch: the same layout, so the same tile
// function reads it), then each wave runs its tiles' K loops against that sample's V.  The sums
// are written once, after the last sample; nothing of size [n][Jp] is read.  Samples are added
// oldest first, the order in which a watch list registered before the first kept sweep adds them.
template <typename T, int MU>
__global__ __launch_bounds__(256) void k_samples_score(SampleView sv, const uint32_t* __restrict__ users, uint32_t n,
                                                       uint32_t J, uint32_t Jp, uint32_t Kp, int clamp, double lo,
                                                       double hi, double* __restrict__ S1, double* __restrict__ S2) {
    extern __shared__ double us[];  // [16 MU][Kp + 2], the rows' biases [16 MU], the rows' user ids [16 MU]
    constexpr int TW = (int)SAMPLES_TW;
    const uint32_t ld = Kp + 2;
    double* ub = us + (size_t)16 * MU * ld;
    uint32_t* uid = reinterpret_cast<uint32_t*>(ub + 16 * MU);
    const uint32_t w0 = blockIdx.x * 16 * MU;
    if (threadIdx.x < 16 * MU) uid[threadIdx.x] = w0 + threadIdx.x < n ? users[w0 + threadIdx.x] : 0u;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n16 = lane & 15, kq = lane >> 4;
    const uint32_t ntile = Jp / 16;
    const bool biased = sv.bu != nullptr;
    double s1[TW][MU][4], s2[TW][MU][4];
#pragma unroll
    for (int i = 0; i < TW; ++i)
#pragma unroll
        for (int t = 0; t < MU; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) s1[i][t][j] = s2[i][t][j] = 0.0;
    for (uint32_t s = 0; s < sv.count; ++s) {
        const uint32_t p = ring_slot(sv.head, s, sv.cap);
        const T* U = static_cast<const T*>(sv.U) + (size_t)p * sv.su;
        const T* V = static_cast<const T*>(sv.V) + (size_t)p * sv.sv;
        const double* bu = biased ? sv.bu + (size_t)p * sv.sbu : nullptr;
        const double* bv = biased ? sv.bv + (size_t)p * sv.sbv : nullptr;
        const double b0 = biased ? sv.b0[s] : 0.0;
        __syncthreads();  // the ids are staged; the previous sample's rows are read
        // 16 lanes per row, 16 rows per pass (Kp is a multiple of 16): no division, 128-byte runs of a row
        for (uint32_t r = threadIdx.x >> 4; r < 16 * MU; r += 16) {
            const bool live = w0 + r < n;
            const T* urow = U + (size_t)uid[r] * Kp;
            for (uint32_t k = threadIdx.x & 15; k < Kp; k += 16) us[r * ld + k] = live ? (double)urow[k] : 0.0;
        }
        if (threadIdx.x < 16 * MU) ub[threadIdx.x] = biased && w0 + threadIdx.x < n ? bu[uid[threadIdx.x]] : 0.0;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TW; ++i) {
            const uint32_t tile = (blockIdx.y * TW + i) * 4 + wave;
            if (tile >= ntile) continue;  // a tile past the items (uniform in the wave; no barrier below)
            const uint32_t item = tile * 16 + n16, irow = min(item, J - 1);  // a padding item reads the last row (not stored)
            wd4 acc[MU];
#pragma unroll
            for (int t = 0; t < MU; ++t) acc[t] = wd4{0, 0, 0, 0};
            watch_tile_products<T, MU>(us, ld, V + (size_t)irow * Kp + 4 * kq, Kp, w0, n, n16, kq, acc);
            const double bj = biased ? bv[irow] : 0.0;
#pragma unroll
            for (int t = 0; t < MU; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t r = t * 16 + kq + 4 * j;
                    double sc = watch_biased(acc[t][j], biased, b0, ub[r], bj);
                    sc = watch_clamped(sc, clamp, lo, hi);
                    watch_sums_add(s1[i][t][j], s2[i][t][j], sc, s1[i][t][j], s2[i][t][j]);
                }
        }
    }
#pragma unroll
    for (int i = 0; i < TW; ++i) {
        const uint32_t item = ((blockIdx.y * TW + i) * 4 + wave) * 16 + n16;
        if (item >= J) continue;
#pragma unroll
        for (int t = 0; t < MU; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t w = w0 + t * 16 + kq + 4 * j;
                if (w >= n) continue;
                const size_t o = (size_t)w * Jp + item;
                S1[o] = s1[i][t][j];
                S2[o] = s2[i][t][j];
            }
    }
}

template <typename T, int MU>
static hipError_t samples_score_mu(const SampleView& sv, const uint32_t* users, uint32_t n, uint32_t J, uint32_t Kp,
                                   int clamp, double lo, double hi, double* S1, double* S2, hipStream_t st) {
    const uint32_t Jp = watch_jp(J), per = 4 * SAMPLES_TW;
    // the user groups along x: workgroups launched together read the same V rows
    const dim3 grid((n + 16 * MU - 1) / (16 * MU), (Jp / 16 + per - 1) / per);
    k_samples_score<T, MU><<<grid, 256, samples_lds_bytes(MU, Kp), st>>>(sv, users, n, J, Jp, Kp, clamp, lo, hi, S1, S2);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_samples_score(const SampleView& sv, const uint32_t* users, uint32_t n, uint32_t J, uint32_t Kp, int clamp,
                                double lo, double hi, double* S1, double* S2, hipStream_t st) {
    if (n == 0 || J == 0) return hipSuccess;
    if (sv.count == 0 || sv.count > sv.cap || sv.head >= sv.cap || Kp % 16) return hipErrorInvalidValue;
    switch (watch_mu(Kp)) {
        case 4:
            return samples_score_mu<T, 4>(sv, users, n, J, Kp, clamp, lo, hi, S1, S2, st);
        case 2:
            return samples_score_mu<T, 2>(sv, users, n, J, Kp, clamp, lo, hi, S1, S2, st);
    }
    return samples_score_mu<T, 1>(sv, users, n, J, Kp, clamp, lo, hi, S1, S2, st);
}
template hipError_t launch_samples_score<double>(const SampleView&, const uint32_t*, uint32_t, uint32_t, uint32_t, int,
                                                 double, double, double*, double*, hipStream_t);
template hipError_t launch_samples_score<float>(const SampleView&, const uint32_t*, uint32_t, uint32_t, uint32_t, int,
                                                double, double, double*, double*, hipStream_t);

// ------------------------------------------------------------------ scores of pairs
// 16 lanes per pair, 16 pairs per workgroup.  Every lane of a group ends with the same dot
// product (the butterfly adds the same two values in every lane) and runs the same sums; lane 0
// writes.  No lane leaves early: the shuffles need them all.
template <typename T>
__global__ __launch_bounds__(256) void k_samples_pairs(SampleView sv, const uint32_t* __restrict__ users,
                                                       const uint32_t* __restrict__ items, uint32_t n, uint32_t Kp,
                                                       int clamp, double lo, double hi, double* __restrict__ mean,
                                                       double* __restrict__ sd) {
    const uint32_t pair = blockIdx.x * 16 + (threadIdx.x >> 4), l = threadIdx.x & 15;
    const bool live = pair < n;
    const uint32_t u = live ? users[pair] : 0u, it = live ? items[pair] : 0u;
    const bool biased = sv.bu != nullptr;
    double s1 = 0.0, s2 = 0.0;
    for (uint32_t s = 0; s < sv.count; ++s) {
        const uint32_t p = ring_slot(sv.head, s, sv.cap);
        const T* ur = static_cast<const T*>(sv.U) + (size_t)p * sv.su + (size_t)u * Kp;
        const T* vr = static_cast<const T*>(sv.V) + (size_t)p * sv.sv + (size_t)it * Kp;
        double d = 0.0;
        for (uint32_t k = l; k < Kp; k += 16) d = fma((double)ur[k], (double)vr[k], d);
#pragma unroll
        for (int m = 8; m > 0; m >>= 1) d += __shfl_xor(d, m, 16);
        double sc = watch_biased(d, biased, biased ? sv.b0[s] : 0.0, biased ? sv.bu[(size_t)p * sv.sbu + u] : 0.0,
                                 biased ? sv.bv[(size_t)p * sv.sbv + it] : 0.0);
        sc = watch_clamped(sc, clamp, lo, hi);
        watch_sums_add(s1, s2, sc, s1, s2);
    }
    if (live && l == 0) {
        double m, d;
        watch_moments(s1, s2, (double)sv.count, m, d);
        mean[pair] = m;
        if (sd) sd[pair] = d;
    }
}

template <typename T>
hipError_t launch_samples_pairs(const SampleView& sv, const uint32_t* users, const uint32_t* items, uint32_t n, uint32_t Kp,
                                int clamp, double lo, double hi, double* mean, double* sd, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (sv.count == 0 || sv.count > sv.cap || sv.head >= sv.cap) return hipErrorInvalidValue;
    k_samples_pairs<T><<<(n + 15) / 16, 256, 0, st>>>(sv, users, items, n, Kp, clamp, lo, hi, mean, sd);
    return hipGetLastError();
}
template hipError_t launch_samples_pairs<double>(const SampleView&, const uint32_t*, const uint32_t*, uint32_t, uint32_t,
                                                 int, double, double, double*, double*, hipStream_t);
template hipError_t launch_samples_pairs<float>(const SampleView&, const uint32_t*, const uint32_t*, uint32_t, uint32_t, int,
                                                double, double, double*, double*, hipStream_t);

}  // namespace sbmf
