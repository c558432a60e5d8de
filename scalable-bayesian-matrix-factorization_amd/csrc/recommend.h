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

// The scoring launch's shape: a workgroup holds 16 MU rows in LDS, as many as 64 KB take (Kp <= 112:
// 64, <= 240: 32, else 16), as rows of Kp + 2 doubles with their ids behind them.
inline int watch_mu(uint32_t Kp) { return Kp <= 112 ? 4 : Kp <= 240 ? 2 : 1; }
inline size_t watch_lds_bytes(int MU, uint32_t Kp) {
    return (size_t)16 * MU * (Kp + 2) * sizeof(double) + 16 * MU * sizeof(uint32_t);
}

// One sweep's scores of the n watched users against all J items, added to the running sums:
// s = U[users[w]] . V[j] (+ (b0 + bu[user]) + bv[j] when bu is non-null: the biased sampler),
// clamped to [lo, hi] when clamp is set; S1[w][j] += s, S2[w][j] += s*s (rows of Jp doubles).
// T is the tables' type; the products and the sums are f64 either way.  Every element is
// read, added to and written by one lane, in a fixed order: a rerun is bit-identical.
template <typename T>
hipError_t launch_watch_accum(const uint32_t* users, uint32_t n, const T* U, const T* V, uint32_t J, uint32_t Kp,
                              const double* bu, const double* bv, double b0, int clamp, double lo, double hi,
                              double* S1, double* S2, hipStream_t st);

// The same launch with an epilogue chosen by the caller, for f64 tables with both bias vectors
// (the libFM query list, fmq.h: rows of A are the queries' s_q, rows of B the candidates' q^B, ba
// = a_q, bb = y_j, b0 = w0): s = ((b0 + ba[row]) + bb[j]) + A[row] . B[j]; WATCH_EPI_CDF then
// takes the probit probability ref_cdf_gaussian(s); WATCH_EPI_SET stores s and s * s in place of
// adding them (the old sums are not read).  epi = 0 is launch_watch_accum<double>'s own kernel.
enum : int { WATCH_EPI_CDF = 1, WATCH_EPI_SET = 2 };
hipError_t launch_watch_accum_epi(int epi, const uint32_t* rows, uint32_t n, const double* A, const double* B,
                                  uint32_t J, uint32_t Kp, const double* ba, const double* bb, double b0, int clamp,
                                  double lo, double hi, double* S1, double* S2, hipStream_t st);

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

// The same selection over rows that hold a mean and a variance themselves (M, Vr [n][Jp]): sd =
// sqrt(max(0, var)), no division and no difference of squares (the online VB lists, vb_lists.h).
hipError_t launch_watch_select_given(uint32_t n, const double* M, const double* Vr, uint32_t J, double risk,
                                     const uint32_t* mask, uint32_t topn, uint32_t* items, double* mean, double* sd,
                                     hipStream_t st);

}  // namespace sbmf
