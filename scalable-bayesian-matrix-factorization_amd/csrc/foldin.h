// foldin.h -- host-callable launcher of the fold-in row kernel in foldin.hip: one draw of
// every guest's factor row from its conditional given the sweep's item factors (guests are
// users outside the training set, given by their ratings; include/sbmf.h, sbmf_foldin_users).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sbmf {

// Largest Kp (num_factor <= 256 rounded up to the 16-column block) the kernel's LDS is sized for.
constexpr uint32_t FOLDIN_KP_MAX = 256;

// Draws G[g] (rows of Kp, T = the tables' type) for g < n from V, in place, starting from the
// row's current value: e_j = r_j - G[g] . V[items[j]] over the guest's ratings
// ptr[g] <= j < ptr[g + 1], then for k = 0..K-1 in order P = sum v_jk^2,
// Q = sum v_jk (e_j + v_jk u_k), var = 1 / (sg_k + tau P), mean = var (tau Q + sg_k mu_k),
// u_k' = mean + (sd_is_var ? var : sqrt(var)) z_k, e_j += v_jk (u_k - u_k') -- in blocks of
// 16 columns (Gram block by MFMA f64 16x16x4, 16 serial draws, the residuals updated once
// per block).  hyper = [sg | mu], 2 Kp doubles with zero padding; z_k = Philox normal k of
// (seed, row g, sweep, TAG_GUEST).  E: scratch of ptr[n] doubles (the residuals; contents on
// exit are not meaningful).  order: a permutation of 0..n-1, workgroup b draws guest order[b]
// (the host lists the longest guests first: the launch ends with its longest row).  All
// arithmetic in f64: V is widened on load, the row rounded once on store.  Padding columns
// stay zero.  One workgroup per guest, every sum in a fixed order and no atomics: a rerun is
// bit-identical.
template <typename T>
hipError_t launch_foldin(uint32_t n, const uint32_t* order, const uint32_t* ptr, const uint32_t* items,
                         const double* ratings, T* G, const T* V, uint32_t K, uint32_t Kp, const double* hyper,
                         double tau, int sd_is_var, uint64_t seed, uint32_t sweep, double* E, hipStream_t st);

}  // namespace sbmf
