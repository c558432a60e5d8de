// recommend.h -- host-callable launchers for the watch-list kernels in recommend.hip:
// posterior score moments of a caller-chosen list of users against every item,
// accumulated once per collected sweep, and the exact top-N selection over them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sbmf {

// Items per accumulator row: J rounded up to the 16-item MFMA tile.
inline uint32_t watch_jp(uint32_t J) { return (J + 15) / 16 * 16; }
// 32-bit words per row of the rated-item mask.
inline uint32_t watch_jw(uint32_t J) { return (J + 31) / 32; }

// One sweep's scores of the n watched users against all J items, added to the running sums:
// s = U[users[w]] . V[j] (+ (b0 + bu[user]) + bv[j] when bu is non-null: the biased sampler),
// clamped to [lo, hi] when clamp is set; S1[w][j] += s, S2[w][j] += s*s (rows of Jp doubles).
// T is the tables' type; the products and the sums are f64 either way.  Every element is
// read, added to and written by one lane, in a fixed order: a rerun is bit-identical.
template <typename T>
hipError_t launch_watch_accum(const uint32_t* users, uint32_t n, const T* U, const T* V, uint32_t J, uint32_t Kp,
                              const double* bu, const double* bv, double b0, int clamp, double lo, double hi,
                              double* S1, double* S2, hipStream_t st);

// mean[j] = s1[j] / nw, sd[j] = sqrt(max(0, s2[j] / nw - mean[j]^2)) for j < J: one row's
// moments, computed by the expressions the selection ranks by (bit for bit).
hipError_t launch_watch_moments(const double* s1, const double* s2, uint32_t J, double nw, double* mean, double* sd,
                                hipStream_t st);

// mask[w] (Jw words, zero on entry): bit j set for every item j that users[w] rated in the
// training set (uptr / upart: the user-side CSR).
hipError_t launch_watch_mask(const uint32_t* users, uint32_t n, const uint32_t* uptr, const uint32_t* upart,
                             uint32_t* mask, uint32_t Jw, hipStream_t st);

// Per watched user the topn (1..1024) items with the largest key mean - risk * sd, ties by
// ascending item id; items whose mask bit is set are left out (mask null: none).  Outputs are
// [n][topn]; slots past the number of candidates hold item 0xffffffff and NaN.  sd may be null.
hipError_t launch_watch_select(uint32_t n, const double* S1, const double* S2, uint32_t J, double nw, double risk,
                               const uint32_t* mask, uint32_t topn, uint32_t* items, double* mean, double* sd,
                               hipStream_t st);

}  // namespace sbmf
