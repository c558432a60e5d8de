// samples.h -- host-callable launchers for the posterior sample store's kernels in samples.hip:
// the scores of any users against every item, and of any (user, item) pairs, summed over all
// stored samples inside one launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "recommend.h"

namespace sbmf {

// The store as the kernels read it: a ring of `cap` slots, the oldest sample in slot `head`,
// `count` of them kept.  Slot p holds U at U + p su and V at V + p sv (elements of the tables'
// type: I Kp and J Kp), and with biases bu + p I, bv + p J (null without); b0 [count] is in
// the samples' order of age, oldest first.
struct SampleView {
    const void *U = nullptr, *V = nullptr;
    const double *bu = nullptr, *bv = nullptr, *b0 = nullptr;
    size_t su = 0, sv = 0, sbu = 0, sbv = 0;
    uint32_t head = 0, cap = 0, count = 0;
};

// The scoring launch's shape: a workgroup of four waves holds 16 MU user rows of one sample in
// LDS (watch_mu, recommend.h) with the rows' ids and biases behind them, and takes SAMPLES_TW
// item tiles of 16 per wave, whose sums stay in registers over the sample loop.
constexpr uint32_t SAMPLES_TW = 2;
inline size_t samples_lds_bytes(int MU, uint32_t Kp) { return watch_lds_bytes(MU, Kp) + (size_t)16 * MU * sizeof(double); }

// S1[w][j] = sum over the samples, oldest first, of s = U_s[users[w]] . V_s[j] (+ (b0_s +
// bu_s[user]) + bv_s[j] with biases), clamped to [lo, hi] when clamp is set; S2 the same of
// s * s; rows of Jp = watch_jp(J) doubles, the columns from J on not written.  Each sum is held
// by one lane and written once: a rerun is bit-identical.  Per sample the products are
// k_watch_accum's (recommend_dev.h).
template <typename T>
hipError_t launch_samples_score(const SampleView& sv, const uint32_t* users, uint32_t n, uint32_t J, uint32_t Kp, int clamp,
                                double lo, double hi, double* S1, double* S2, hipStream_t st);

// mean[p], sd[p] (watch_moments' expressions) of the pairs (users[p], items[p]) over the
// samples, in the same order: 16 lanes per pair, lane l sums k = l, l + 16, ... and the 16
// partial sums meet in a fixed butterfly.  sd may be null.
template <typename T>
hipError_t launch_samples_pairs(const SampleView& sv, const uint32_t* users, const uint32_t* items, uint32_t n, uint32_t Kp,
                                int clamp, double lo, double hi, double* mean, double* sd, hipStream_t st);

}  // namespace sbmf
