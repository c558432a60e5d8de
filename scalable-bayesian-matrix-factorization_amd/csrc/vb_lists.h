// vb_lists.h -- host-callable launchers of the online VB learner's lists (vb_lists.hip): the
// closed-form mean and variance of a score under the learner's factorised Gaussian posterior, for
// rows (training users, or guests' rows in a caller buffer) against every item and for single
// (user, item) pairs, and a guest's posterior from its ratings with the item side held fixed.
//
// With user u's and item j's means mu, variances s (biases: w), and the global bias (mu0, s0):
//   d    = sum_f mu_uf mu_jf
//   tv   = sum_f (s_uf s_jf + s_uf mu_jf^2 + s_jf mu_uf^2)
//   mean = ((d + mu^w_u) + mu^w_j) + mu0
//   var  = ((tv + s^w_u) + s^w_j) + s0
// the reference's e / t terms of a case (fm_learn_vb_online.h:80-310; k_predict, vbo.hip) without
// the target: no clamp and no 1 / alpha noise term -- the moments of the model's prediction.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vbo.h"

namespace sbmf {

// The scoring launch's shape: a workgroup holds 16 MU rows in LDS three times over -- mu_u,
// mu_u^2 + s_u and s_u, rows of Kp + 2 doubles -- with their ids behind them.  MU is the largest
// of 4, 2, 1 whose three arrays fit 64 KB (Kp <= 32: 4, <= 80: 2); MU = 1 takes what Kp asks for
// (Kp = 256: 99,136 bytes of the CU's 160 KB).
inline int vb_score_mu(uint32_t Kp) { return Kp <= 32 ? 4 : Kp <= 80 ? 2 : 1; }
inline size_t vb_score_lds_bytes(int MU, uint32_t Kp) {
    return (size_t)3 * 16 * MU * (Kp + 2) * sizeof(double) + 16 * MU * sizeof(uint32_t);
}

// The rows of a scoring launch: attribute-major tables [.][Kp] (zero padding) of means and
// variances, and the rows' bias means and variances.  ids != null: row w is entry ids[w] of the
// tables (the training users, of muT / sgT and mu_w / sg_w); ids == null: row w is entry w (the
// guests' buffer).
struct VBRows {
    const uint32_t* ids;
    const double *mu, *sg, *w_mu, *w_sg;
};
// The item side: rows I.. of muT / sgT and of mu_w / sg_w, and the scalars.
struct VBItems {
    const double *mu, *sg, *w_mu, *w_sg;
    const VBScal* scal;
    uint32_t J, Kp;
};

// M[w][j] = mean, Vr[w][j] = var of the n rows against all J items (rows of Jp = J rounded up to
// 16 doubles; the padding is not written).  Every element is written by one lane from a
// fixed-order sum, nothing is read back: a rerun is bit-identical.
hipError_t launch_vb_score(const VBRows& rows, uint32_t n, const VBItems& it, double* M, double* Vr, hipStream_t st);

// mean[q], sd[q] = sqrt(max(0, var)) of the pairs (users[q], items[q]), 16 lanes per pair in
// k_predict's order of sums; var (may be null) the variance itself
hipError_t launch_vb_pairs(const uint32_t* users, const uint32_t* items, uint64_t n, const double* muT, const double* sgT,
                           const VBTables& tb, uint32_t Kp, double* mean, double* sd, double* var, hipStream_t st);

// sd[j] = sqrt(max(0, var[j])), the selection's expression (recommend_dev.h)
hipError_t launch_vb_sd(const double* var, uint32_t n, double* sd, hipStream_t st);

// A guest's posterior from its n ratings (j, r_j), items, mu0 and alpha fixed: the reference's
// update_w, then update_v factor-outer (fm_learn_vb_online.h:635-800) at step size rho = 1 on a
// new attribute whose cases are the guest's ratings.  With P_b = sigma_w + alpha n and
// P_f = sigma_v[f] + alpha sum_j (mu_jf^2 + s_jf), from b = 0, g = 0, e_j = r_j - mu0 - mu^w_j,
// `scans` times:
//   b   <- alpha sum_j (e_j + b) / P_b;               e_j -= delta b
//   g_f <- alpha sum_j mu_jf (e_j + g_f mu_jf) / P_f;  e_j -= mu_jf delta g_f    f = 0 .. K-1 in order
// Variances 1 / P_b, 1 / P_f.  ptr / items / ratings / order / E: a GuestCSR (lists.h) on the
// device; one workgroup per guest, order[] the longest first.  GM, GS [n][Kp] (zero padding), gb,
// gs [n].  No random numbers; every sum in a fixed order.
constexpr uint32_t VB_GUEST_KP_MAX = 256;
hipError_t launch_vb_guest(const uint32_t* ptr, const uint32_t* items, const double* ratings, const uint32_t* order,
                           double* E, uint32_t n, uint32_t scans, const VBItems& it, const double* sigma_v, uint32_t K,
                           double* GM, double* GS, double* gb, double* gs, hipStream_t st);

}  // namespace sbmf
