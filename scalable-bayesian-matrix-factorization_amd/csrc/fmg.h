// fmg.h -- libFM's MCMC / ALS learner (fm_learn_mcmc.h:411-623 draw_all, :627-835
// draw_w0 / draw_w / draw_v, :117-348 predict_data_and_write_to_eterms) for cases with any
// number of features and real-valued x, on the GPU.  The two-attribute learner (fmm.h)
// is built around "one user and one item per case"; this one keeps libFM's own cache:
// one {e, q} record per training case (e_q_term), and the training set twice -- a
// case-major CSR (q, predictions) and an attribute-major CSC of {case, x} entries
// (libFM's data_t), cases ascending within an attribute.
//
// draw_w / draw_v read and write the cache of the drawn attribute's cases only, so two
// attributes that share no case commute exactly.  sbmf_fm_ranges cuts [0, p) into
// contiguous ranges of mutually exclusive attributes; libFM's ascending loop over a range
// is one launch per row-length bin (each attribute with the normal libFM's order assigns
// it), and the ranges run in ascending order.  A one-hot field is one range; a multi-hot
// field degrades to ranges of one attribute, and the chain is still libFM's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/sbmf.h"
#include "fm_target.h"

namespace sbmf {

constexpr uint32_t FG_MAX_REL = 4;  // relations of one context (the prediction kernels' argument block)

// One pass over the attribute rows of one (range, bin).  Row `a` owns the CSC entries
// [aptr[a], aptr[a+1]); an entry is {case, bits of x (float)}.
struct FGPassArgs {
    const uint32_t* rows;   // [nrows] attributes of this launch
    uint32_t nrows;
    const uint32_t* aptr;   // [p+1]
    const uint2* ent;       // [nnz] {case, x}
    double2* eq;            // [n] {e, q} per training case (libFM's e_q_term)
    double* own;            // w, or column f of v, by attribute
    const double* z;        // normals, z[a * zs + zoff] (do_sample)
    uint32_t zs, zoff;
    double alpha, mu, lambda;
    int do_sample;
    // long rows in chunks (non-null: the launch runs over chunks {row, first entry, entries,
    // long-row index}): xmode 1 writes chunk ri's {sum h e, sum h^2} to sums[ri]; xmode 2
    // takes {old, new, keep} from delta[long-row index] and updates the chunk's cases;
    // xmode 0: sums, draw and update in one pass
    int xmode;
    const uint4* chunks;
    double2* sums;
    const double4* delta;
    // attribute groups (-meta), last so that the fields above keep their places: grp[a] the
    // group of attribute a, grp_bytes (1, 2 or 4) wide, and this pass's priors lm[g] = {lambda,
    // mu}; a row then takes lm[grp[row]] in place of the scalars mu / lambda.  grp null: one
    // group, the scalars.
    const void* grp;
    const double2* lm;
    int grp_bytes;
    // a relation's pass (fmg_rel_wpass / fmg_rel_vpass): the block rows' records (below); a row
    // is then an attribute of the relation, an entry {block row, x}, and own / z / grp point at
    // the relation's first attribute.  Null in the passes over the cases.
    double4* rb;
};
// draw_w (:670-719) / draw_v (:780-835) over the rows of a launch, 64 / 256 / 1024 threads per row
hipError_t fmg_wpass(const FGPassArgs& a, int threads_per_row, hipStream_t st);
hipError_t fmg_vpass(const FGPassArgs& a, int threads_per_row, hipStream_t st);
// long rows: row i of `rows` owns chunks [cfirst[i], cfirst[i+1]); chunk sums added in chunk
// order, the draw, own written, delta[i] = {old, new, keep}
hipError_t fmg_chunk_draw(const FGPassArgs& a, const uint32_t* rows, const uint32_t* cfirst, uint32_t nlong,
                          const double2* csums, int vpass, double4* delta, hipStream_t st);
// The sums the hyperparameter draws (fm_learn_mcmc.h:931-1089) take over the attributes of one
// group of one model column (v column c < K, w for c = K): out[c * G + g] = {gm, m}, gm from
// mg[c * G + g].y adding (x_a - mg[c * G + g].x)^2, m from 0 adding x_a, over the group's
// attributes in ascending id -- each one sequential chain without contraction, so the host loop's
// bits.  Group g's members: gidx[gptr[g] .. gptr[g+1]) ascending, or the range from gfirst[g]
// when gfirst[g] != 0xffffffff (a contiguous group).  One workgroup per (column, group).
hipError_t fmg_group_sums(const double* v, const double* w, uint32_t p, uint32_t K, uint32_t G, const uint32_t* gptr,
                          const uint32_t* gidx, const uint32_t* gfirst, const double2* mg, double2* out, hipStream_t st);
// eq[c].q = sum over the case's entries (ascending attribute) of v_f[attr] * x  (add_main_q, :513-517)
hipError_t fmg_q(const uint32_t* cptr, const uint32_t* cattr, const float* cx, uint64_t n, const double* vf,
                 double2* eq, hipStream_t st);
// part[b] = {sum e^2, sum (e - w0)} over 1024-case blocks of eq[].e; eq[c].e -= d
hipError_t fmg_esums(const double2* eq, uint64_t n, double w0, double* part, hipStream_t st);
hipError_t fmg_shift(double2* eq, uint64_t n, double d, hipStream_t st);
// predict_data_and_write_to_eterms (:117-348) per case in its accumulation order.  Train
// (eq non-null): eq[c] = {pred - y, 0}, part[b] = sum (clamp(pred) - y)^2.  Test: pthis[t] =
// pred, sum_all[t] += clamp(pred), part[2b] = (clamp(sum_all / it1) - y)^2, part[2b+1] =
// (clamp(pred) - y)^2.
struct FGPredictArgs {
    const uint32_t* cptr;
    const uint32_t* cattr;
    const float* cx;
    const float* y;
    uint64_t n;
    const double* vT;  // [p][Kp]
    const double* w;   // [p]
    double w0;
    uint32_t K, Kp;
    int k0, k1;
    double lo, hi;
    // relations (last, so that the fields above keep their places): case c joins block row
    // map[c] of relation r, whose q^B_f is qbf[row * K + f] and whose q-term is qs[row]
    // (fmg_rel_block_predict).  nrel = 0: the cases alone.
    uint32_t nrel;
    struct Rel {
        const uint32_t* map;
        const double* qbf;
        const double* qs;
    } rel[FG_MAX_REL];
};
hipError_t fmg_predict_train(const FGPredictArgs& a, double2* eq, double* part, hipStream_t st);
hipError_t fmg_predict_test(const FGPredictArgs& a, double it1, double* pthis, double* sum_all, double* part,
                            hipStream_t st);
// The classification frames (fm_target.h; y in {-1, +1}).  Train: eq[c] = {pred - latent target, 0}
// (FM_TGT_HOST: {pred, 0} and ta.yhat[c] = pred), ta.cnt[b] the block's correct votes.  Test:
// pthis[t] = p = cdf_gaussian(pred), sum_all[t] += p, cnt[2b] / cnt[2b+1] the correct votes of
// sum_all / it1 and of p, ll[b] the block's -log10 likelihood of p clipped to [0.01, 0.99].
hipError_t fmg_class_train(const FGPredictArgs& a, const FMTargetArgs& ta, double2* eq, hipStream_t st);
hipError_t fmg_class_test(const FGPredictArgs& a, double it1, double* pthis, double* sum_all, uint32_t* cnt, double* ll,
                          hipStream_t st);
// eq[c].e -= t[c] (FM_TGT_HOST: the host's targets)
hipError_t fmg_sub_targets(double2* eq, uint64_t n, const double* t, hipStream_t st);

// ---- block-structure relations (libFM's -relation; fm_learn_mcmc.h:57-65, :458-491, :521-620,
// draw_w_rel :721-777, draw_v_rel :839-899).  A relation holds its features once per block row;
// every case joins one block row (map[c]).  Block row j's state is relation_cache's seven doubles
// as two 32-byte halves: rb[2j] = {we, y, wnum, q}, rb[2j + 1] = {weq, wc, wc_sqr, 0} -- the w
// step reads and writes the first half alone.
//
// Gather (:463-468, :585-598): per block row the sums over its train cases (bcase[bptr[j] ..
// bptr[j+1]), ascending) with the un-sync fused in.  vstep 0: we = sum e, then e -= y.  vstep 1:
// q_c = q - q^B, we = sum e, weq = sum e q_c, wc = sum q_c, wc_sqr = sum q_c^2, then e -= y +
// q_c q^B and q = q_c.  A case belongs to one block row, so nothing collides; the sums have a
// fixed order (lane-strided shares, butterfly, waves in wave order).
struct FGRelArgs {
    const uint32_t* rows;  // [nrows] block rows of this launch
    uint32_t nrows;
    const uint32_t* bptr;
    const uint32_t* bcase;
    double4* rb;
    double2* eq;
    // block rows with more cases than SBMF_FMM_LONG in chunks, as the passes' long rows (non-null:
    // the launch runs over chunks {block row, first case, cases, long-row index}): chunk ri's four
    // sums go to sums[ri] -- the un-sync of its cases is done, it needs y and q^B alone -- and
    // fmg_rel_gather_combine adds a block row's chunk sums in chunk order into its record
    const uint4* chunks;
    double4* sums;
};
hipError_t fmg_rel_gather(const FGRelArgs& a, int vstep, int threads_per_row, hipStream_t st);
// long block row i of `rows` owns chunks [cfirst[i], cfirst[i+1]) of sums
hipError_t fmg_rel_gather_combine(const uint32_t* rows, const uint32_t* cfirst, uint32_t nlong, const double4* sums,
                                  int vstep, double4* rb, hipStream_t st);
// Sync (:487-489, :616-619) per train case: e += y[j] (vstep 1: + q q^B[j], then q += q^B[j])
hipError_t fmg_rel_sync(const uint32_t* map, uint64_t n, const double4* rb, double2* eq, int vstep, hipStream_t st);
// draw_w_rel / draw_v_rel over the rows of a launch: FGPassArgs with rb set (eq unused)
hipError_t fmg_rel_wpass(const FGPassArgs& a, int threads_per_row, hipStream_t st);
hipError_t fmg_rel_vpass(const FGPassArgs& a, int threads_per_row, hipStream_t st);
// q^B of factor f per block row (:524-545): rb[2j].q = sum over the block row's entries
// (ascending attribute) of vf[attr] x, vf pointing at the relation's first attribute ...
hipError_t fmg_rel_q(const uint32_t* rptr, const uint32_t* rattr, const float* rx, uint32_t nb, const double* vf,
                     double4* rb, hipStream_t st);
// ... and eq[c].q += q^B[map[c]] (:548-552)
hipError_t fmg_rel_addq(const uint32_t* map, uint64_t n, const double4* rb, double2* eq, hipStream_t st);
// The block rows' part of predict_data_and_write_to_eterms (:172-220, :252-273, :299-346): qbf[j *
// K + f] = q^B_jf, qs[j] = -sum_f sum_i 1/2 v^2 x^2 + sum_i w x, rb[2j].y = sum_f 1/2 q^B_jf^2 + qs[j],
// rb[2j].q = 0.  vT / w point at the relation's first attribute.
hipError_t fmg_rel_block_predict(const uint32_t* rptr, const uint32_t* rattr, const float* rx, uint32_t nb,
                                 const double* vT, const double* w, uint32_t K, uint32_t Kp, int k1, double* qbf,
                                 double* qs, double4* rb, hipStream_t st);

// ---- host learner (fmg.cpp): libFM's chain (FMChain, fmc.h) on this layout, driven by the C ABI in sbmf.cpp
struct FMChain;
// a relation as sbmf_add_relation collects it: the block table as a CSR by block row (entries
// sorted by attribute), the block row of every train / test case, its own groups (empty: one)
struct FMRelation {
    std::vector<uint64_t> ptr;
    std::vector<uint32_t> attr;
    std::vector<float> x;
    uint32_t num_attr = 0;
    std::vector<uint32_t> train_row, test_row, group;
    uint32_t G = 1;
};
// libFM's attribute groups as the C ABI collects them: group[a] for every attribute (empty: one
// group), the groups' -regular precisions (empty: cfg.regw / cfg.regv for every group)
struct FMGroups {
    std::vector<uint32_t> group;
    std::vector<double> regw, regv;
};
FMChain* fmg_create(const sbmf_config& c, const sbmf_cases& train, const sbmf_cases& test, hipStream_t st,
                    const FMGroups* groups = nullptr, const std::vector<FMRelation>* relations = nullptr);
// the ranges of sbmf_fm_ranges over [0, p) (train cases; ids >= train.num_attr have no case)
void fm_ranges(const sbmf_cases& train, uint32_t p, std::vector<uint32_t>& bounds);

}  // namespace sbmf
