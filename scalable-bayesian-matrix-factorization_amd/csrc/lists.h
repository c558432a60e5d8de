// lists.h -- the host steps the score lists (lists.cpp) and the sample store (samples.cpp) share:
// the contexts they cover, the top-N selection and the moments of one row from a pair of sums, and
// the guests' CSR on the device.  Defined in lists.cpp.
#pragma once
#include "common.h"

struct sbmf_ctx;

namespace sbmf {

// The learners and schedules a list (`what`: its noun in the messages) covers; everything else is
// SBMF_E_STATE.
void list_scope(const sbmf_ctx* c, const char* what, const char* fn, bool unbiased_only);
// a list's queued work is done (it runs on the evaluation's stream, which the compute stream
// waits for before the sweep's results are copied)
void list_sync(sbmf_ctx* c);

// One call's selection temporaries, for slices of at most `rows` rows: the top-N ids, their
// [mean | spread], and (excluding) the rows' bit masks over the columns.
struct TopnScratch {
    DBuf d_it, d_ms, d_mask;
    void alloc(uint32_t rows, uint32_t topn, uint32_t J, bool exclude);  // throws as DBuf::alloc
};
// Top-N of the m rows whose sums S1 / S2 [m][Jp] hold `count` samples: mask (the columns
// csr_items[csr_ptr[i] .. csr_ptr[i + 1]) of row d_ids[r] = i are left out; a null csr_ptr: none
// is), select, synchronise, download into items / mean / stdev [m][topn] (stdev may be null).
// given: S1 / S2 hold the rows' means and variances themselves (the online VB lists; count unused).
void select_topn(TopnScratch& t, const uint32_t* d_ids, uint32_t m, const double* S1, const double* S2, uint32_t J,
                 uint32_t count, const uint32_t* csr_ptr, const uint32_t* csr_items, uint32_t topn, double risk, Span& span,
                 hipStream_t st, uint32_t* items, double* mean, double* stdev, bool given = false);
// mean and (may be null) spread [J] of one row of sums S1 / S2 over `count` samples
void row_moments(const double* S1, const double* S2, uint32_t J, uint32_t count, hipStream_t st, double* mean, double* stdev);

// Guests given by their ratings, a CSR, as the fold-in kernels read them: ptr from 0, the guests'
// order of drawing (by falling length within each slice: a launch ends with its longest row, so
// those start first), the residuals' area E [nnz], and the identity list 0..n-1 (the scoring
// kernel's row list).
struct GuestCSR {
    uint32_t n = 0, nnz = 0;
    DBuf d_ptr, d_items, d_ratings, d_order, d_E, d_ids;
    // what the entry points that take guests refuse (SBMF_E_ARG); J: the items
    static void check(const char* fn, uint32_t n, const uint32_t* ptr, const uint32_t* items, const double* ratings, uint32_t J);
    // (n > 0) allocates and fills everything, and synchronises `st`.  ids: where the identity list
    // goes when the caller holds one already (d_ids then stays empty).
    void upload(uint32_t n_, const uint32_t* ptr, const uint32_t* items, const double* ratings, uint32_t rows_per_slice,
                hipStream_t st, uint32_t* ids = nullptr);
    void drop();
};

}  // namespace sbmf
