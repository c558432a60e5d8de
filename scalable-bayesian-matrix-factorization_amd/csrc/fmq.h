// fmq.h -- the query list of libFM's MCMC / ALS learner (include/sbmf.h, sbmf_fm_query_cases):
// posterior scores of nq query cases against every block row of one relation, the candidates.
//
// With relations the learner keeps, per block row j of relation R after fmg_rel_block_predict,
// q^B_jf (qbf), the q-term qs[j] and y_j = sum_f 1/2 q^B_jf^2 + qs[j] (rb[2j].y).  libFM's
// prediction of query q joined to block row j is bilinear in those -- fg_pred<true> with the
// square 1/2 (s + q^B)^2 multiplied out:
//   score(q, j) = ((w0 + a_q) + y_j) + sum_f s_q[f] q^B_jf
//   s_q[f] = sum over q's main entries of v[attr][f] x + sum_{r != R} q^B_r[row_r(q)][f]
//   a_q    = sum_f 1/2 s_q[f]^2 - sum_f sum_entries 1/2 v^2 x^2 + sum_entries w x + sum_{r != R} qs_r[row_r(q)]
// so an iteration's scores are one [nq x K] . [K x n_B] product and two bias vectors: the shape
// of the watch list's scoring launch (recommend.hip), whose kernel runs it.  Per iteration:
//   k_fmq_terms     s_q (rows of Kp doubles, zero padding) and a_q of every query
//   k_fmq_operands  the candidates' q^B as rows of Kp doubles with zero padding, and their y_j
//   k_watch_accum   the scores, through the epilogue, into the [nq][nBp] sums
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "fmg.h"

namespace sbmf {

struct FMQTermsArgs {
    uint32_t nq;
    const uint32_t* ptr;   // [nq + 1] the queries' main entries, ascending attribute within a query
    const uint32_t* attr;
    const float* x;
    const double* vT;      // [p][Kp]
    const double* w;       // [p]
    uint32_t K, Kp;
    int k1;
    // the relations other than the candidates', in relation order: query q joins block row
    // rows[q] of a relation whose q^B and q-terms are qbf / qs
    uint32_t nrel;
    struct Rel {
        const uint32_t* rows;
        const double* qbf;
        const double* qs;
    } rel[FG_MAX_REL];
    double* s;  // [nq][Kp]
    double* a;  // [nq]
};
// One wave per query, lanes along f (the reads of vT[attr * Kp + f] and qbf[row * K + f] are
// contiguous), a loop over the entries; the sums over f are per-lane chains in ascending f and a
// butterfly: a fixed order, no atomics.
hipError_t fmq_terms(const FMQTermsArgs& a, hipStream_t st);
// B[j * Kp + f] = f < K ? qbf[j * K + f] : 0, y[j] = rb[2 j].y for the nb block rows; B holds
// fmq_operand_bytes.  Kp >= 16: sbmf_create refuses num_factor = 0, so no launch here sees K = 0.
inline size_t fmq_operand_bytes(uint32_t nb, uint32_t Kp) { return (size_t)nb * Kp * sizeof(double); }
hipError_t fmq_operands(const double* qbf, const double4* rb, uint32_t nb, uint32_t K, uint32_t Kp, double* B,
                        double* y, hipStream_t st);

// The list as the learner sees it (FMChain::query): the queries and operand tables are the list's
// own; the sums, the identity row list and the count are the context's ScoreList (ctx.h).
struct FMQueryList {
    uint32_t rel = 0, nq = 0, nb = 0;
    int clamp = 0;
    DBuf d_ptr, d_attr, d_x, d_rows, d_s, d_a, d_B, d_y;  // d_rows: [nrel][nq], the candidates' own slice unused
    DBuf d_eptr, d_erows;                                  // the exclusion CSR (null: none)
    const uint32_t* ids = nullptr;
    double *S1 = nullptr, *S2 = nullptr;
    uint32_t* count = nullptr;
    hipEvent_t ev[3] = {};  // the last iteration's [begin, terms and operands end, accumulate end]
    void drop() {
        for (DBuf* d : {&d_ptr, &d_attr, &d_x, &d_rows, &d_s, &d_a, &d_B, &d_y, &d_eptr, &d_erows}) d->release();
        for (hipEvent_t& e : ev) event_destroy(e);
        rel = nq = nb = 0;
        clamp = 0;
        ids = nullptr;
        S1 = S2 = nullptr;
        count = nullptr;
    }
};

}  // namespace sbmf
