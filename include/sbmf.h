/*
 * sbmf.h -- C ABI of the MI355X-native Scalable-BPMF (SBPMF) Gibbs sampler.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * has no library interface: its sampler is the body of main() in
 * src/libfm/gibbs_sbpmf_final.cpp:23-595 (and the libFM learner behind
 * `bin/libFM -method mcmc`, src/libfm/libfm.cpp:72-644 ->
 * fm_learn_mcmc::learn, fm_learn_mcmc.h:1154).  Each entry point below names
 * the reference code it replaces.  Plain C types only: no torch, no HIP types.
 * The CLI (`sbmf`, libFM flag grammar) and the Python mirror (package
 * sbmf/) are built on exactly these calls; INTEGRATION.md shows the ctypes
 * binding a maintainer would add.
 *
 * Ownership: the caller owns every host array it passes (they are copied in);
 * the library owns all device memory, streams and RCCL communicators.
 * Errors: every call returns SBMF_OK (0) or a negative SBMF_E_* code and
 * records a message readable with sbmf_last_error(ctx) (or
 * sbmf_last_global_error() when no context exists).  The reference instead
 * throws std::string / const char* and still exits 0 (libfm.cpp:636-640).
 * Threading: a context is used by one host thread at a time.
 * Device: every compute entry point requires a gfx950 GPU; there is no CPU
 * fallback (sbmf_create fails with SBMF_E_DEVICE without one).
 */
#ifndef SBMF_H_
#define SBMF_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBMF_ABI_VERSION 2
#define SBMF_NKIND 11 /* kernel kinds reported by sbmf_get_timing */

enum sbmf_status {
    SBMF_OK = 0,
    SBMF_E_ARG = -1,      /* invalid argument / configuration                    */
    SBMF_E_STATE = -2,    /* call out of order (e.g. run before set_train)       */
    SBMF_E_DEVICE = -3,   /* HIP runtime error or no usable GPU                  */
    SBMF_E_IO = -4,       /* file open / parse error                             */
    SBMF_E_COMM = -5,     /* RCCL error                                          */
    SBMF_E_NOMEM = -6     /* host or device allocation failed                    */
};

/* RNG mode. REFERENCE replays the reference's exact variate stream (glibc
 * rand(), Leva normals, Marsaglia-Tsang gammas; src/util/random.h:118-176),
 * generated on the host and consumed by the GPU; PHILOX draws counter-based
 * normals inside the kernels (throughput mode, rank-count independent). */
enum sbmf_rng_mode { SBMF_RNG_REFERENCE = 0, SBMF_RNG_PHILOX = 1 };

/* Quirk set. FINAL = gibbs_sbpmf_final.cpp semantics (posterior VARIANCE
 * passed as the stdev of ran_gaussian, :393,413,485,529; init N(0,1); clamp
 * [1,5]).  SBPMF2 = src/libfm/gibbs_sbpmf2.cpp (:240,248,386,406,412,557:
 * init N(0,0.1), nu0 without 1/2, mu_v uses sigma_u*, clamp [0.5,5]).
 * NONE = the statistically correct sampler (stdev = sqrt(variance)).
 * BIAS2 = the biased sampler at the top level of the reference,
 * gibbs_sbpmf2.cpp:335-637 (the paper's Algorithm 1, libFM -dim '1,1,K'):
 * global bias b0 and per-user / per-item biases with Normal-Gamma priors,
 * alpha ~ G(a0 + N, b0 + sum E^2), factor precisions with shape alpha0 + I,
 * posterior variance as stdev, init N(0,0.1), clamp [0.5,5].  BIAS22 = the
 * same sampler as src/libfm/gibbs_sbpmf22.cpp (init N(0,1), clamp [1,5]). */
enum sbmf_quirks { SBMF_QUIRKS_FINAL = 0, SBMF_QUIRKS_SBPMF2 = 1, SBMF_QUIRKS_NONE = 2, SBMF_QUIRKS_BIAS2 = 3,
                   SBMF_QUIRKS_BIAS22 = 4 };

/* Learner (libFM -method, libfm.cpp:394-445).  MCMC = the SBPMF Gibbs sampler.
 * VB = online variational Bayes, the reference's fm_learn_vb_online
 * (src/libfm/src/fm_learn_vb_online.h, -method vb_online; its batch -method vb
 * is a no-op as shipped): per epoch a shuffle into
 * mini-batches and natural-gradient steps (t0 + t)^-0.5 on the per-attribute
 * Gaussian posteriors of w0, w and V.  With VB a "sweep" of sbmf_run is an
 * epoch, rmse_avg is the test RMSE of the posterior-mean prediction, tau is
 * alpha, factors / biases are the posterior means, and only F64 is offered. */
/* LIBFM_MCMC = libFM's own MCMC chain (bin/libFM -method mcmc,
 * src/libfm/src/fm_learn_mcmc.h:411-623 draw_all, fm_learn_mcmc_simultaneous.h):
 * a factorization machine over the users-first one-hot attributes (user u,
 * item I + i) with global bias w0, attribute biases w and factors v, one
 * attribute group with Normal-Gamma hyperpriors, noise precision alpha, the
 * factors drawn f-outer (per factor: every user, then every item) with the
 * posterior standard deviation; a sweep re-predicts train and test.  ALS =
 * the same learner without sampling or hyperparameter inference (bin/libFM
 * -method als, libfm.cpp:132-136): deterministic.  Both use libfm_dim and
 * reg0 / regw / regv, f64 only; rmse_train / rmse_avg are libFM's "Train=" /
 * "Test=", tau is alpha.  On several GPUs (sbmf_comm_init) each rank owns a
 * sbmf_partition_rows user range and every case of those users; the item sums
 * are all-gathered and added in rank order, so every rank draws the same items
 * and the chain equals one rank's up to the rounding of that sum. */
enum sbmf_method { SBMF_METHOD_MCMC = 0, SBMF_METHOD_VB = 1, SBMF_METHOD_LIBFM_MCMC = 2, SBMF_METHOD_ALS = 3 };
/* libFM's -task (sbmf_config::task) */
enum sbmf_task { SBMF_TASK_REGRESSION = 0, SBMF_TASK_CLASSIFICATION = 1 };

/* Arithmetic type of factors, residuals and reductions on the GPU.  F64 is
 * the reference's (all-double) arithmetic. */
enum sbmf_precision { SBMF_F64 = 0, SBMF_F32 = 1 };

typedef struct sbmf_config {
    uint32_t num_factor;   /* K: -dim 'k0,k1,K' (libfm.cpp:93); reference D=20 (:218)          */
    uint32_t num_iter;     /* collection sweeps: -iter (libfm.cpp:97); reference 100 (:299)     */
    uint32_t burnin;       /* burn-in sweeps before collection; reference 0 (:300)              */
    uint64_t seed;         /* -seed (honoured; the reference ignores it, libfm.cpp:124)         */
    int32_t rng_mode;      /* enum sbmf_rng_mode                                               */
    int32_t quirks;        /* enum sbmf_quirks                                                 */
    int32_t precision;     /* enum sbmf_precision                                              */
    int32_t device;        /* HIP device ordinal for this context                              */
    double init_stdev;     /* <0: quirk-set default (1.0 final / 0.1 sbpmf2); -init_stdev      */
    double clamp_lo;       /* prediction clamp; <0: quirk-set default (1.0 / 0.5)              */
    double clamp_hi;       /* default 5.0 (gibbs_sbpmf_final.cpp:556)                          */
    /* hyperpriors (gibbs_sbpmf_final.cpp:256-269) */
    double a0, b0, alpha0, beta0, nu0, mu0;
    uint32_t recompute_every; /* recompute E=r-UV from scratch every n sweeps (reference: every
                                 sweep, :317-334); 0 = only at start                            */
    uint32_t eval_train;      /* 1: compute train RMSE of the current sample each sweep          */
    uint32_t eval_test;       /* 1: test prediction + running-mean RMSE each sweep (:539-563)    */
    uint32_t gram_threshold;  /* reserved, must be 0 (the full-Gram row route was removed)       */
    uint32_t row_kernel;      /* reserved, must be 0 (the per-coordinate row kernels were removed:
                                 the MFMA Gram-block kernels are the only row kernels)          */
    uint32_t stream_threshold;/* rows with more ratings use the streaming Gram-block kernel
                                 k_gres (0 = default: 256 f64 / 512 f32)                        */
    uint32_t split_chunk;     /* streaming-kernel task size: rows longer than this are split
                                 into chunks on co-resident workgroups (0 = the register
                                 capacity of the workgroup shape; larger values are capped to it) */
    uint32_t tune;            /* kernel-variant bits for experiments (0 = tuned defaults):
                                 bit 1 = residuals from r - own.partner as on several GPUs,
                                 bit 2 = power-of-two waves per Gram-block row (2/4/8) instead
                                         of ceil(ratings / ratings-per-wave),
                                 bit 3 = f64 rows of 33..64 ratings on two 8-vector waves instead
                                         of one 16-vector wave,
                                 bit 7 = k_gres on 4-wave workgroups (both sides),
                                 bit 8 = f64 rows of 65..128 ratings as 3-4-wave Gram-block rows
                                         (default: one-wave k_grow workgroups),
                                 bit 9 = f64 rows of 129..256 ratings as 3-4-wave Gram-block rows
                                         (default: two-wave k_grow workgroups),
                                 bit 10 = f64 rows of 9..64 ratings on the one-wave Gram-block
                                          kind (default: one-wave k_grow workgroups),
                                 bit 11 = f32 rows of 17..512 ratings on the Gram-block kinds
                                          (default: one- / two-wave k_grow workgroups),
                                 bit 12 = k_grow reads sigma and mu from memory at every K
                                          (default: from LDS when Kp <= 128),
                                 bit 13 = f64 user streaming rows all on one 4-wave k_gres set
                                          (default: rows above 512 ratings on a second, 8-wave set),
                                 bit 14 = (experiment) that second user set on 16-wave workgroups,
                                 bit 17 = k_gres on 16-wave workgroups (both sides),
                                 bit 23 = f64 user streaming rows all on 8-wave k_gres workgroups
                                          (default: up to 512 ratings on 4-wave ones, 512-rating
                                          tasks, longer rows on a second, 8-wave set),
                                 bit 24 = k_gres as a cooperative launch (experiments only; the
                                          default is an ordinary launch in every schedule: tasks are
                                          claimed in queue order, no co-residency needed),
                                 bit 25 = a half's Gram-block kinds all on one side stream
                                          (default since round 5: alternating between two side
                                          streams, beside each other and the streaming launch),
                                 bit 26 = no overlap of the next sweep's prologue (sums, column
                                          statistics, host draws) with the test evaluation
                                          (Philox mode; the chain is the same either way),
                                 bit 27 = f64 item rows on 8-wave k_gres workgroups (default:
                                          rows > 1024 ratings on 16-wave ones, the rest 8-wave),
                                 bit 29 = a half's Gram-block launches after its streaming launch
                                          on one stream (default: on a second stream beside it),
                                 bit 30 = a half's two streaming sets (items: rows > 1024 and the
                                          rest) one after the other (default: side by side),
                                 bit 28 = (one rank) the test evaluation after the next sweep's
                                          prologue kernels on the compute stream (default: on the
                                          second stream beside them; the results are the same).
                                 Every other bit is refused (SBMF_E_ARG): bits 0, 4-6, 15, 16,
                                 18-22 and 31 selected variants removed in rounds 1-6 (measured
                                 slower or neutral, kept in git history).  Bits whose meaning
                                 changed between rounds: 24 (round 4: ordinary
                                 launch; since round 5 the cooperative one), 25 (round-4 LDS-DMA
                                 prefetch; since round 5 one side stream).  */
    uint32_t method;          /* enum sbmf_method: -method mcmc (default) | vb                   */
    uint32_t vb_batches;      /* online VB: mini-batches per epoch (0 = the reference's 30,
                                 fm_learn_vb_online_simultaneous.h:62)                           */
    uint32_t average;         /* running mean of the test prediction: 0 = quirk-set default
                                 (sum / (sweep + 1), gibbs_sbpmf_final.cpp:559, which counts
                                 burn-in sweeps; quirks none: collected sweeps), 1 = sum over
                                 the collected sweeps / their number, 2 = sum / (sweep + 1)       */
    uint32_t libfm_dim;       /* LIBFM_MCMC / ALS: the k0,k1 of -dim 'k0,k1,K' as bits: bit 0 =
                                 global bias w0, bit 1 = attribute biases w (default 3)          */
    double reg0, regw, regv;  /* LIBFM_MCMC / ALS: -regular 'r0,r1,r2' (libfm.cpp:484-513): ALS's
                                 fixed precisions, MCMC's starting w / v precisions (default 0) */
    uint32_t pipeline;        /* SBPMF sampler, throughput mode (Philox, prologue overlap on): 1 =
                                 sweep s+1's start (its hyperparameter upload and user half) is
                                 queued before sweep s is reported to the run callback, so the
                                 device does not idle through the host's per-sweep work.  The
                                 chain and the reports are the same.  In sweep s's callback
                                 sbmf_predict and the hyperparameter getters (sbmf_get_hyper,
                                 sbmf_get_biases' b0) are valid and describe sweep s; the factors
                                 (sbmf_get_factors) are not, because sweep s+1's user half may be
                                 running.  A stop the callback asks for takes effect after sweep
                                 s+1.  0 (default): each sweep is reported with the device idle
                                 after it                                                         */
    uint32_t task;            /* enum sbmf_task: SBMF_TASK_REGRESSION (default) | SBMF_TASK_CLASSIFICATION
                                 (libFM's -task c, a probit model: targets <= 0 become -1, the others
                                 +1, libfm.cpp:454-455; min / max target play no part).  LIBFM_MCMC and
                                 ALS only; any other method with it is SBMF_E_ARG                  */
} sbmf_config;

/* Per-sweep report passed to the run callback. */
typedef struct sbmf_sweep_info {
    uint32_t sweep;            /* 0-based sweep index (burn-in included)                     */
    uint32_t collected;        /* 1 if this sweep entered the running mean                   */
    double rmse_avg;           /* test RMSE of the running-mean prediction (the reference's
                                  "rmse is", gibbs_sbpmf_final.cpp:562); NaN if no test set  */
    double rmse_this;          /* test RMSE of this sweep's sample alone                      */
    double rmse_train;         /* train RMSE of this sample (clamped), NaN if not evaluated   */
    double tau;                /* noise precision drawn this sweep                           */
    double ms_sweep;           /* device time of the sweep from its start to the end of the item
                                  half, ms.  Throughput mode (overlapped start): the sweep's start
                                  work -- residual sum, column statistics, both normal fills and
                                  the hyperparameter upload -- was queued at the end of the
                                  previous sweep, beside its test evaluation, and is not in here
                                  (sbmf_timing.ms_hyper of the previous sweep holds it)        */
    double ms_eval;            /* device time of the test evaluation, ms                      */
    /* SBMF_TASK_CLASSIFICATION (the rmse_* above are then NaN; these are NaN in regression; tau
       stays alpha): */
    double acc_train;          /* share of the train cases this sweep's model classifies right  */
    double acc_avg;            /* test accuracy of the running-mean probability (libFM's "Test=",
                                  fm_learn_mcmc_simultaneous.h:327-338); NaN if no test set      */
    double acc_this;           /* test accuracy of this sweep's probabilities alone (:383-401)   */
    double ll_this;            /* their mean -log10 likelihood, clipped to [0.01, 0.99]          */
} sbmf_sweep_info;

/* Return non-zero to stop the run early. */
typedef int (*sbmf_sweep_cb)(const sbmf_sweep_info* info, void* user);

typedef struct sbmf_ctx sbmf_ctx;

/* --- configuration / lifetime -------------------------------------------------------------- */
/* Fill reference defaults (gibbs_sbpmf_final.cpp:218,256-269,299-300). */
int sbmf_config_default(sbmf_config* cfg);
/* Create a context on cfg->device.  Replaces the reference's setup in main()
 * (gibbs_sbpmf_final.cpp:252-306).  Fails with SBMF_E_DEVICE without a GPU. */
int sbmf_create(const sbmf_config* cfg, sbmf_ctx** out);
void sbmf_destroy(sbmf_ctx* ctx);
const char* sbmf_last_error(const sbmf_ctx* ctx);
const char* sbmf_last_global_error(void);
int sbmf_abi_version(void);

/* --- data ---------------------------------------------------------------------------------- */
/* Training triples (0-based ids, any order; file order is preserved as the
 * reference's R / R_t entry order, gibbs_sbpmf_final.cpp:192-215). */
int sbmf_set_train(sbmf_ctx* ctx, uint64_t n, const uint32_t* user, const uint32_t* item, const double* rating);
int sbmf_set_test(sbmf_ctx* ctx, uint64_t n, const uint32_t* user, const uint32_t* item, const double* rating);
/* Optional: row counts.  Default (0,0) = max id + 1 over train and test
 * (gibbs_sbpmf_final.cpp:146-148); empty ids are kept and sampled. */
int sbmf_set_dims(sbmf_ctx* ctx, uint32_t num_users, uint32_t num_items);

/* Build the device layout (CSR / CSC, degree bins), upload, and initialise
 * U, V (draws the init variates, :236-250).  Implicitly called by sbmf_run. */
int sbmf_prepare(sbmf_ctx* ctx);

/* Run `sweeps` Gibbs sweeps (continuing the chain across calls).  One sweep =
 * the reference loop body gibbs_sbpmf_final.cpp:309-564: tau, per-factor
 * hyperparameters, user half-sweep, item half-sweep, test evaluation. */
int sbmf_run(sbmf_ctx* ctx, uint32_t sweeps, sbmf_sweep_cb cb, void* user);

/* --- results ------------------------------------------------------------------------------- */
/* Averaged clamped test prediction (sum / collected sweeps; libfm -out,
 * libfm.cpp:629-634).  out: [n_test].  SBMF_TASK_CLASSIFICATION: the probability of the
 * positive class (MCMC: the mean over the iterations; ALS: the last iteration's), clipped to
 * [0, 1] (fm_learn_mcmc.h:355-379). */
int sbmf_predict(sbmf_ctx* ctx, double* out);
/* Factors as row-major doubles: U [num_users][K], V [num_items][K]. Either may be NULL. */
int sbmf_get_factors(sbmf_ctx* ctx, double* U, double* V);
/* Overwrite the factors (row-major doubles).  For checkpoints and tests. */
int sbmf_set_factors(sbmf_ctx* ctx, const double* U, const double* V);
/* Hyperparameters [sigma_u | mu_u | sigma_v | mu_v] (4K doubles) and tau.  On a
 * libFM MCMC / ALS context with more than one attribute group (sbmf_set_attr_groups)
 * hyper4k is SBMF_E_STATE -- read sbmf_get_fm_groups --; with hyper4k NULL tau is
 * still returned. */
int sbmf_get_hyper(sbmf_ctx* ctx, double* hyper4k, double* tau);
int sbmf_get_dims(sbmf_ctx* ctx, uint32_t* num_users, uint32_t* num_items, uint64_t* n_train, uint64_t* n_test);
/* Biased sampler only: b_i [num_users], b_j [num_items] and the global b_0
 * (gibbs_sbpmf2.cpp:276-318 state).  Any pointer may be NULL. */
int sbmf_get_biases(sbmf_ctx* ctx, double* bu, double* bv, double* b0);

/* --- measurement --------------------------------------------------------------------------- */
/* Device times of the last sweep (HIP events on the context's stream).
 * kern_*[side][kind]: side 0 = user half, 1 = item half; kind =
 *   0..4  MFMA Gram-block row kernels: 1 wave/row (two sizes), then 2..8
 *         waves/row (ceil(ratings/32) f64, /64 f32) timed in three groups; up to
 *         8/64/64/128/256 ratings (f64), 16/64/128/256/512 (f32),
 *   5     streaming MFMA Gram-block kernel k_gres: one persistent launch per
 *         stream set over tasks of <= 512 / 1024 / 2048 (f64, 4- / 8- / 16-wave
 *         workgroups) ratings held in VGPRs -- whole rows, or chunks of longer
 *         rows on co-resident workgroups -- plus the publish of split rows,
 *   6..10 reserved (the removed per-coordinate and full-Gram row kernels: 0).
 * kern_ms of the streaming kind is the last sweep's; those of kinds 0..4 are timed on
 * the first sweep of each sbmf_run call and kept (an event between two launches on a
 * stream leaves the device idle for microseconds).  kern_bytes is the
 * algorithmic traffic of that launch per SURVEY.md §8(d): per rating
 * s*K (partner row) + 4 (partner id) + s (residual), per row 2*s*K (own row
 * read + write), s = 4 (f32) or 8 (f64). */
typedef struct sbmf_timing {
    double ms_user_half, ms_item_half, ms_hyper, ms_eval, ms_comm;
    double kern_ms[2][SBMF_NKIND];
    uint64_t kern_bytes[2][SBMF_NKIND];
    uint32_t kern_rows[2][SBMF_NKIND];
    uint64_t bytes_algorithmic;  /* whole sweep, both halves                                    */
    uint32_t n_launch;           /* kernel launches in the last sweep                           */
    double ms_vb_factor;         /* online VB: device time of an epoch's factor passes (the 2K
                                    vbo_user_v / vbo_item_v launches of every mini-batch, HIP
                                    events around each batch's factor loop), mean over the last
                                    run's epochs (round 6); 0 for the other learners              */
} sbmf_timing;
int sbmf_get_timing(sbmf_ctx* ctx, sbmf_timing* t);

/* --- posterior top-N for a watch list of users ----------------------------------------------- */
/* Not a reference interface: the reference scores only the test pairs it was
 * given (gibbs_sbpmf_final.cpp:539-563).  A watch list is a caller-chosen set
 * of users whose score against EVERY item is tracked inside the chain: after
 * each collected sweep s the sampler adds score_s(w, j) = u_s[users[w]] . v_s[j]
 * (+ b0 + b_u + b_j with the biased quirk sets, as the test prediction adds
 * them) and its square to device-resident f64 sums, so the posterior mean is
 * the mean over sweeps of u_s . v_s, not the product of mean factors.  The
 * products and sums are f64 in both precisions (an F32 context's table values
 * are widened on load), every element is summed in a fixed order without
 * atomics, and the sampler's chain is untouched: a context with a watch list
 * draws bit for bit what it draws without one.
 * Scope: the SBPMF sampler (SBMF_METHOD_MCMC, every quirk set) on one rank.
 * Out of scope here, each refused with SBMF_E_STATE and a message naming the
 * reason: the VB, libFM-MCMC and ALS learners (the libFM learners have a list
 * of their own over a relation's block rows: sbmf_fm_query_cases below); a
 * context that joined a communicator; a virtual rank; and reading results
 * before any sweep was accumulated.
 *
 * sbmf_watch_users: register (or replace) the list.  After sbmf_prepare, also
 * between sbmf_run calls.  Allocates and zeroes two [n][Jp] f64 accumulators
 * (Jp = num_items rounded up to 16) and restarts the list's own count n_w of
 * accumulated sweeps; n = 0 drops the list and frees them.  flags bit 0: clamp
 * each sweep's score to the context's [clamp_lo, clamp_hi] before accumulating,
 * as the test prediction is clamped (default: unclamped, which is what ranking
 * wants -- clamped scores saturate and tie).  Ids may repeat (duplicate rows).
 * An id >= num_users is SBMF_E_ARG; a failed allocation SBMF_E_NOMEM with the
 * byte count in the message (the list is then dropped).  Memory: 16 n Jp bytes
 * -- every user of ML-20M would need 59 GB, which is why the list is the
 * caller's.  sbmf_set_factors leaves the sums alone. */
int sbmf_watch_users(sbmf_ctx* ctx, uint32_t n, const uint32_t* users, uint32_t flags);
/* The full row of watched user w (index into the list): mean[j] = S1 / n_w,
 * stdev[j] = sqrt(max(0, S2 / n_w - mean^2)), j < num_items: the population
 * spread over the n_w sweeps collected since registration.  The reference's
 * running-mean quirk (divide by sweep + 1, burn-in included: sbmf_config.average)
 * is NOT reproduced here; with clamping on, mean differs from sbmf_predict only
 * when burnin > 0 under that default divisor (or when the list was registered
 * after the first collected sweep).  stdev may be NULL. */
int sbmf_watch_scores(sbmf_ctx* ctx, uint32_t w, double* mean, double* stdev);
/* Per watched user the topn (1..1024, else SBMF_E_ARG) items with the largest
 * key mean - risk * stdev, formed in IEEE double arithmetic from exactly the
 * values sbmf_watch_scores returns: risk = 0 ranks by posterior mean, risk > 0
 * by a lower confidence bound.  Order: key descending, ties by ascending item
 * id -- exact and deterministic.  Items the user rated in the training set are
 * left out unless flags bit 0 is set.  items / mean / stdev: [n][topn], row w
 * for users[w]; slots past the number of candidates hold item 0xffffffff and
 * NaN.  stdev may be NULL. */
int sbmf_recommend(sbmf_ctx* ctx, uint32_t topn, uint32_t flags, double risk, uint32_t* items, double* mean,
                   double* stdev);
/* Device time (HIP events), ms: the last collected sweep's scoring launch and
 * the last sbmf_recommend's selection (mask + select kernels); 0 before the
 * first.  A call of its own because sbmf_timing keeps its size (ABI 2). */
int sbmf_watch_timing(sbmf_ctx* ctx, double* ms_score, double* ms_select);

/* --- fold-in list: posterior top-N for users outside the training set ------------------------ */
/* Guests are users who have no row in U: they arrived after the chain started,
 * and the caller gives their ratings instead of an id.  Given a sweep's item
 * factors V_s, the user-side hyperparameters and tau, a guest's factor row has
 * exactly the conditional the user half draws its rows from; drawing it once per
 * sweep beside the chain gives a posterior sample of the guest's factors.  The
 * guests' ratings never feed back: with or without a list, U, V, the
 * hyperparameters, the predictions and the watch list's results are bit for bit
 * the same.  Scores, moments and the top-N are the watch list's, kept in sums
 * of the fold-in list's own; both lists may be registered at once.
 *
 * The draw, after every sweep's item half since registration (burn-in included),
 * starting from the row the previous sweep left (zero at registration), with the
 * sigma_u, mu_u and tau the sweep's user half used, all in f64 (an F32 context's V
 * is widened on load, the row rounded once on store):
 *   e_j = r_j - G[g] . V_s[item_j]             over the guest's ratings, then for k = 0..K-1:
 *   P = sum_j v_jk^2,  Q = sum_j v_jk (e_j + v_jk u_k)
 *   var = 1 / (sigma_k + tau P),  mean = var (tau Q + sigma_k mu_k)
 *   u_k' = mean + s z_k,  s = var under the quirk sets final / sbpmf2 (the reference's
 *                          variance-as-stdev quirk), sqrt(var) under none
 *   e_j += v_jk (u_k - u_k')
 * z_k = sbmf_philox_normals(seed, absolute sweep index, 7, g, K)[k] in both RNG
 * modes (to the last bits of the device's log / sincos, as for the other tags);
 * the reference-mode host stream is not touched.  A guest without ratings is
 * drawn from N(mu_u, .): the cold start.  A rerun gives bit-identical rows and sums.
 *
 * Scope: the SBPMF sampler with the unbiased quirk sets, one rank, both
 * precisions, both RNG modes.  SBMF_E_STATE with a message naming the reason:
 * the biased quirk sets (a guest bias would need a draw of its own); the VB,
 * libFM-MCMC and ALS learners; a context that joined a communicator; a virtual
 * rank; reading results before a sweep was drawn (factors) or accumulated
 * (scores, top-N).
 *
 * sbmf_foldin_users: register (or replace) the list of n guests, a CSR:
 * ptr[n + 1], guest g's ratings are items[ptr[g] .. ptr[g + 1]) (each below
 * num_items; a repeated item counts as separate ratings) with ratings[] beside
 * them; a guest may have none.  After sbmf_prepare, also between sbmf_run calls.
 * Allocates the guest table ([n + 2][Kp] in the context's precision), a residual
 * scratch of ptr[n] - ptr[0] doubles and two [n][Jp] f64 accumulators, copies the
 * CSR, and restarts the rows (zero) and counts; n = 0 drops the list and frees
 * everything.  flags bit 0: clamp each sweep's score as sbmf_watch_users does.
 * SBMF_E_ARG: an item id >= num_items, a decreasing ptr, unknown flags.
 * SBMF_E_NOMEM with the byte count in the message on a failed allocation (the
 * list is then dropped). */
int sbmf_foldin_users(sbmf_ctx* ctx, uint32_t n, const uint32_t* ptr, const uint32_t* items, const double* ratings,
                      uint32_t flags);
/* The current sample's guest rows, rows[n][K] (the last sweep's draw). */
int sbmf_foldin_factors(sbmf_ctx* ctx, double* rows);
/* Guest g's row of posterior means and standard deviations over the sweeps
 * collected since registration; definitions as sbmf_watch_scores.  stdev may be NULL. */
int sbmf_foldin_scores(sbmf_ctx* ctx, uint32_t g, double* mean, double* stdev);
/* sbmf_recommend for the guests: key, order, tie rule, outputs [n][topn] and
 * empty slots as there.  "Rated" means the guest's own items (left out unless
 * flags bit 0 is set); a guest without ratings excludes nothing. */
int sbmf_foldin_recommend(sbmf_ctx* ctx, uint32_t topn, uint32_t flags, double risk, uint32_t* items, double* mean,
                          double* stdev);
/* Device time (HIP events), ms: the last sweep's draw, the last collected
 * sweep's scoring launch, the last sbmf_foldin_recommend's selection; 0 before
 * the first. */
int sbmf_foldin_timing(sbmf_ctx* ctx, double* ms_draw, double* ms_score, double* ms_select);

/* --- posterior sample store: top-N and pair predictions for any user after the run ----------- */
/* Not a reference interface.  The lists above are named before the first
 * collected sweep and their sums live in the process; a sample store keeps
 * thinned samples of the chain itself -- U, V and, with the biased quirk sets,
 * b0, b_u, b_j -- on the device, so that the chain can be used after it ends:
 * top-N for users chosen later, mean and spread of arbitrary pairs, both also
 * from a file in a later process.  One sample takes (I + J) Kp elements of the
 * context's precision (Kp = K rounded up to 16) plus, with biases, (I + J)
 * doubles: ML-20M K = 100 f64 is 148 MB a sample.  The chain is untouched: a
 * context with a store draws bit for bit what it draws without one, and
 * sbmf_set_factors leaves the store alone.
 * Scope: the SBPMF sampler (SBMF_METHOD_MCMC), every quirk set, both
 * precisions, both RNG modes, one rank.  SBMF_E_STATE with a message naming
 * the reason: the VB, libFM-MCMC and ALS learners; a context that joined a
 * communicator; a virtual rank; reading before a sample is kept ("no sample
 * kept yet").
 *
 * sbmf_keep_samples: register (or replace) the store.  After sbmf_prepare,
 * also between sbmf_run calls.  Allocates cap slots up front (a failure is
 * SBMF_E_NOMEM with the byte count in the message; the store is then dropped).
 * The collected sweeps are counted from registration, starting at 0, and
 * every sweep whose count is a multiple of `every` is copied into the next
 * slot -- the first collected sweep after registration is kept; burn-in
 * sweeps never are.  A full store overwrites its oldest sample.  cap = 0
 * drops the store; every = 0 or cap > 65535 is SBMF_E_ARG. */
int sbmf_keep_samples(sbmf_ctx* ctx, uint32_t every, uint32_t cap);
/* The store's state: samples kept, slots, the thinning and the device bytes of
 * the slots (all 0, every 1, without a store).  Any pointer may be NULL. */
int sbmf_samples_info(sbmf_ctx* ctx, uint32_t* count, uint32_t* cap, uint32_t* every, uint64_t* bytes);
/* Sample s, 0 the oldest kept: its absolute sweep index, U [I][K], V [J][K] as
 * doubles (an F32 store widens exactly), bu [I], bv [J], b0 (zeros without
 * biases).  Any output pointer may be NULL.  s >= count is SBMF_E_ARG. */
int sbmf_get_sample(sbmf_ctx* ctx, uint32_t s, uint32_t* sweep, double* U, double* V, double* bu, double* bv,
                    double* b0);
/* sbmf_recommend for any n users, named now: per user the topn (1..1024) items
 * with the largest key mean - risk * stdev over the stored samples, the key,
 * order, tie rule, outputs [n][topn] and empty slots as there.  The score of
 * (user, j) at sample s is U_s[user] . V_s[j] (+ (b0_s + bu_s[user]) + bv_s[j]
 * with biases), its sums run over the samples oldest first in f64, in a fixed
 * order without atomics (a rerun is bit-identical; a watch list registered
 * before the first kept sweep of an every = 1 store adds the same products in
 * the same order).  flags bit 0: keep the items the user rated in training;
 * bit 1: clamp each sample's score to [clamp_lo, clamp_hi].  Ids may repeat.
 * The temporary [n][Jp] sums are allocated for the call and freed after it;
 * the users are processed in slices whose two sums stay within 1 GiB (whole
 * groups of 64 users, one group at least).  stdev may be NULL; with one
 * sample it is exactly 0. */
int sbmf_samples_recommend(sbmf_ctx* ctx, uint32_t n, const uint32_t* users, uint32_t topn, uint32_t flags, double risk,
                           uint32_t* items, double* mean, double* stdev);
/* One user's full row, mean[j] and stdev[j] for j < num_items: exactly the
 * values sbmf_samples_recommend ranks by.  flags bit 1: clamp. */
int sbmf_samples_scores(sbmf_ctx* ctx, uint32_t user, uint32_t flags, double* mean, double* stdev);
/* Posterior mean and population stdev of n arbitrary pairs (users[p],
 * items[p]) over the stored samples, oldest first, dots in f64 in a fixed
 * order.  flags bit 1: clamp.  An id out of range is SBMF_E_ARG.  stdev may
 * be NULL. */
int sbmf_samples_predict(sbmf_ctx* ctx, uint64_t n, const uint32_t* users, const uint32_t* items, uint32_t flags,
                         double* mean, double* stdev);
/* Device time (HIP events), ms: the last kept sweep's copy into the store, the
 * last scoring launch of sbmf_samples_recommend / sbmf_samples_scores (its
 * last slice) and the last selection; 0 before the first. */
int sbmf_samples_timing(sbmf_ctx* ctx, double* ms_copy, double* ms_score, double* ms_select);
/* The store to and from one little-endian file (the format: INTEGRATION.md
 * 3d).  Loading needs a prepared context of the file's num_users, num_items,
 * K, precision and bias-ness (else SBMF_E_ARG naming the field and both
 * values); it replaces the store's samples (cap grows to the file's count if
 * it was smaller, a context without a store gets one of that cap) and does
 * not touch the chain: a context may be created, given its train set (for the
 * rated-item mask), prepared, loaded and queried without one sweep.  File
 * errors are SBMF_E_IO. */
int sbmf_save_samples(sbmf_ctx* ctx, const char* path);
int sbmf_load_samples(sbmf_ctx* ctx, const char* path);
/* Reads and validates a sample file's header alone (no context, no GPU) and
 * reports its fields and the file's size in bytes; any pointer but path may
 * be NULL.  SBMF_E_IO with a message (sbmf_last_global_error) for a file that
 * cannot be opened, a bad magic, an unknown version, a bad field, and a file
 * shorter ("truncated in its header" / "in its body") or longer ("trailing
 * bytes") than its header implies. */
int sbmf_samples_file_info(const char* path, uint32_t* version, uint32_t* precision, uint32_t* num_users,
                           uint32_t* num_items, uint32_t* num_factor, uint32_t* count, uint32_t* bias, uint64_t* bytes);

/* --- sample store: fold-in guests after the run ------------------------------------------- */
/* Not a reference interface.  A user who turns up after training, served from
 * the stored samples with no sweep run: the guest's factor row at sample s is
 * the user half's coordinate loop against V_s (the fold-in list's draw, above),
 * which needs sigma_u, mu_u and tau of the sweep the sample came from.  The
 * store keeps them on the host beside every sample it keeps, and they travel
 * in a companion file of their own (the sample file does not change).
 *
 * sbmf_get_sample_hyper: sample s (as sbmf_get_sample) its [sigma_u | mu_u |
 * sigma_v | mu_v], 4 K doubles in sbmf_get_hyper's layout, and tau: the values
 * the halves of that sweep used.  Either pointer may be NULL.  Works with the
 * biased quirk sets too.  SBMF_E_STATE for samples without hyperparameters:
 * sbmf_load_samples replaces the samples and so clears them; loading the
 * companion file (sbmf_load_samples_hyper) sets them. */
int sbmf_get_sample_hyper(sbmf_ctx* ctx, uint32_t s, double* hyper4k, double* tau);
/* The samples' hyperparameters to and from a little-endian companion file (the
 * format: INTEGRATION.md 3e).  Loading needs a store whose count, K and
 * per-sample sweep indices equal the file's -- the store the sample file saved
 * beside it was loaded into -- else SBMF_E_ARG naming the field (or the first
 * sample whose sweep index differs) and both values.  File errors are
 * SBMF_E_IO. */
int sbmf_save_samples_hyper(sbmf_ctx* ctx, const char* path);
int sbmf_load_samples_hyper(sbmf_ctx* ctx, const char* path);
/* Reads and validates a companion file's header alone (no context, no GPU), as
 * sbmf_samples_file_info does for a sample file, with the same kinds of
 * message; bytes = 24 + 4 count + 8 count (4 K + 1). */
int sbmf_samples_hyper_file_info(const char* path, uint32_t* version, uint32_t* num_factor, uint32_t* count,
                                 uint64_t* bytes);
/* sbmf_foldin_recommend from the stored samples, stateless: each call names the
 * n guests as the CSR of sbmf_foldin_users (ptr [n + 1], items, ratings; a
 * guest may have no ratings, an item may repeat) and re-draws.  Per guest one
 * row is carried from the oldest sample (entered with a zero row) to the
 * newest: at each sample `scans` (1..64) coordinate scans against V_s with
 * that sample's sigma_u, mu_u and tau, scan r taking the Philox normals
 * 256 r + k of the key (seed, sample's absolute sweep index, tag 7, guest g)
 * -- sbmf_philox_normals(seed, sweep, 7, g, 256 scans) lists them -- and every
 * scan starting from e_j = r_j - u . v_j; after the last scan the row is
 * rounded to the context's precision.  With scans = 1 and a store of every = 1
 * kept from the sweep a fold-in list was registered at, the rows, scores and
 * lists are that list's, bit for bit.  A thinned store's consecutive samples
 * are far apart: more scans let the row forget the previous sample's.  The
 * seed and quirks (s_is_var) are this context's: reproducing an in-chain
 * list's numbers from a file needs the training run's seed and quirks.
 * The scores of guest g at sample s are row_s[g] . V_s[j]; key, order, tie
 * rule, outputs [n][topn] and empty slots as sbmf_recommend.  flags bit 0: keep
 * the guest's own items; bit 1: clamp each sample's score.  All arithmetic in
 * f64, every sum in a fixed order, no atomics: a rerun is bit-identical, and
 * calls agree with each other.  Guests are processed in slices of whole groups
 * of 64 whose two [rows][Jp] sums and rows stay within 1 GiB; every temporary
 * is allocated for the call and freed after it (a failure is SBMF_E_NOMEM with
 * the byte count).  stdev may be NULL; with one sample it is exactly 0.
 * Scope: the SBPMF sampler, the unbiased quirk sets, both precisions, both RNG
 * modes, one rank.  SBMF_E_STATE: what the store refuses; no sample kept yet; a
 * store with biases (a guest bias would need a draw of its own); samples
 * without hyperparameters (sbmf_load_samples_hyper).  SBMF_E_ARG: scans 0 or
 * above 64, topn outside 1..1024, an item id >= num_items, a decreasing ptr,
 * unknown flags. */
int sbmf_samples_foldin_recommend(sbmf_ctx* ctx, uint32_t n, const uint32_t* ptr, const uint32_t* items,
                                  const double* ratings, uint32_t scans, uint32_t topn, uint32_t flags, double risk,
                                  uint32_t* out_items, double* mean, double* stdev);
/* The guests' rows themselves: rows [count][n][K] as doubles, oldest sample
 * first. */
int sbmf_samples_foldin_rows(sbmf_ctx* ctx, uint32_t n, const uint32_t* ptr, const uint32_t* items, const double* ratings,
                             uint32_t scans, double* rows);
/* One guest's (guest 0: its `len` items and ratings) full row, mean[j] and
 * stdev[j] for j < num_items: exactly the values sbmf_samples_foldin_recommend
 * ranks by.  flags bit 1: clamp. */
int sbmf_samples_foldin_scores(sbmf_ctx* ctx, uint32_t len, const uint32_t* items, const double* ratings, uint32_t scans,
                               uint32_t flags, double* mean, double* stdev);
/* Device time (HIP events), ms, of the last of the three calls above (its last
 * slice): the draw, the scoring launch and the selection; 0 before the first. */
int sbmf_samples_foldin_timing(sbmf_ctx* ctx, double* ms_draw, double* ms_score, double* ms_select);

/* --- multi-GPU (one process per GPU, RCCL over xGMI) ---------------------------------------- */
/* 128-byte RCCL unique id, produced by rank 0 and shared by the launcher. */
int sbmf_comm_unique_id(uint8_t id[128]);
/* Join an nranks-wide communicator; users and items are then block-partitioned
 * (nnz-balanced) and U / V blocks are all-gathered between half-sweeps. */
int sbmf_comm_init(sbmf_ctx* ctx, int nranks, int rank, const uint8_t id[128]);
/* One communicator for the whole process, shared by several contexts in turn (a
 * driver running many learners on the same ranks, e.g. bench.py's legs): RCCL's
 * set-up (ncclCommInitRank) runs once.  sbmf_comm_attach joins a context to it
 * in place of sbmf_comm_init (before sbmf_prepare); the communicator must
 * outlive every context attached to it.  Contexts attached to one communicator
 * must not run at the same time.  `device` is this rank's HIP device (the contexts'
 * sbmf_config.device); RCCL binds the communicator to it. */
typedef struct sbmf_comm sbmf_comm;
int sbmf_comm_create(int device, int nranks, int rank, const uint8_t id[128], sbmf_comm** out);
int sbmf_comm_attach(sbmf_ctx* ctx, sbmf_comm* comm);
void sbmf_comm_destroy(sbmf_comm* comm);

/* --- loaders (the reference's input formats) ------------------------------------------------ */
typedef struct sbmf_ratings {
    uint64_t n;
    uint32_t* user;
    uint32_t* item;
    double* rating;
} sbmf_ratings;
/* SBPMF triple format "u<sep>i<sep>r" per line, lines accepted iff
 * sscanf("%u%c%u%c%lf") >= 5 (gibbs_sbpmf_final.cpp:43).  Replaces the three
 * serial text passes of gibbs_sbpmf_final.cpp:26-215: one read, line-aligned
 * chunks parsed on threads (SBMF_LOAD_THREADS, default min(cores,
 * OMP_NUM_THREADS)), concatenated in file order. */
int sbmf_load_triples(const char* path, sbmf_ratings* out);
/* libFM text "r f1:v f2:v" (Data.h:192-217) with exactly one user and one
 * item feature per line: the first feature is the user id, the second the
 * item id minus item_offset (users-first layout, e.g. data/m1m/m100k). */
int sbmf_load_libfm(const char* path, uint32_t item_offset, sbmf_ratings* out);
/* libFM binary input <stem>.x + <stem>.y (or .data + .target, preferred as in
 * Data::load, Data.h:113-160): the files tools/convert.cpp:55-205 writes,
 * layouts fmatrix.h:36-52 (sparse rows) and matrix.h:280-328 (targets).  Same
 * one-user-one-item rule and item_offset meaning as sbmf_load_libfm.  Replaces
 * the binary branch of Data::load (Data.h:115-160). */
int sbmf_load_libfm_binary(const char* stem, uint32_t item_offset, sbmf_ratings* out);
/* The transpose <stem>.xt + <stem>.y (or .datat + .target, preferred): the
 * file tools/transpose.cpp:54-172 writes from a .x, one sparse row per
 * feature listing its cases.  This is what bin/libFM -method mcmc|als reads:
 * its data sets are built with has_x = false (libfm.cpp:132-149), so Data::load
 * (Data.h:113-117,143-151) opens only the transpose.  Each case must hold two
 * features; the lower id is the user, the higher the item (item_offset as
 * above).  Replaces the has_xt branch of Data::load. */
int sbmf_load_libfm_binary_t(const char* stem, uint32_t item_offset, sbmf_ratings* out);
/* Data::load's choice of input (Data.h:112-117) for a data set that needs the
 * row-major cases (has_x) and / or the transpose (has_xt): 1 = <stem>.data
 * [+ .datat] + .target, 2 = <stem>.x [+ .xt] + .y, 0 = neither (Data::load
 * then parses <stem> as libFM text); SBMF_E_ARG if both flags are 0. */
int sbmf_libfm_binary_kind(const char* stem, int has_x, int has_xt);
/* Data::load (Data.h:106-283) for rating data: the binary input
 * sbmf_libfm_binary_kind picks for (has_x, has_xt) -- the cases read from the
 * row-major file when has_x, from the transpose otherwise -- else <stem> as libFM text
 * (sbmf_load_libfm).  bin/libFM's sets: has_x = 0, has_xt = 1 for -method
 * mcmc and als, both 1 for the other methods (libfm.cpp:132-149). */
int sbmf_load_libfm_data(const char* stem, int has_x, int has_xt, uint32_t item_offset, sbmf_ratings* out);
/* Writes <stem>.xt / <stem>.y: what tools/convert.cpp then tools/transpose.cpp
 * write for the same cases, byte for byte (rows per feature 0..num_cols-1,
 * ascending case ids, value 1). */
int sbmf_save_libfm_binary_t(const char* stem, const sbmf_ratings* in, uint32_t item_offset, uint32_t num_cols);
/* Writes <stem>.x / <stem>.y in that format (the convert tool's output for
 * rating data): row q = {user[q]:1, item_offset + item[q]:1}, f32 targets;
 * num_cols = max(num_cols, largest feature id + 1). */
int sbmf_save_libfm_binary(const char* stem, const sbmf_ratings* in, uint32_t item_offset, uint32_t num_cols);
/* Writes the SBPMF triple format "u\tv\tr\n" (0-based ids) that the reference's
 * data scripts produce (data/m100k/create_file_scalable_bpmf.py:6-12) and
 * sbmf_load_triples reads back bit for bit: integer ratings as integers, others
 * with %.17g. */
int sbmf_save_triples(const char* path, const sbmf_ratings* in);
void sbmf_free_ratings(sbmf_ratings* r);

/* --- libFM cases with any number of features (the general MCMC / ALS learner) ---------------- */
/* A libFM data set as data: a CSR by case.  Case c holds the features
 * attr[ptr[c] .. ptr[c+1]) with the values x[] beside them (libFM's DATA_FLOAT,
 * fm_data.h:25) and the target target[c]; a case may hold no feature.  num_attr
 * is Data::num_feature (Data.h:220-222): the largest feature id + 1, or 0 for a
 * set without features.  Within a case the entries are sorted by attribute id:
 * the order libFM's in-memory transpose (Data::create_data_t) gives every
 * per-case accumulation (add_main_q, predict_data_and_write_to_eterms).  An
 * attribute repeated inside one case is refused (SBMF_E_ARG): the learner's
 * passes write one {e, q} record per case of the attribute being drawn, and a
 * repeat would make two entries of one row collide on it. */
typedef struct sbmf_cases {
    uint64_t n;        /* cases                                   */
    uint64_t nnz;      /* features over all cases (= ptr[n])      */
    uint32_t num_attr; /* largest feature id + 1 (0: no feature)  */
    uint64_t* ptr;     /* [n + 1]                                 */
    uint32_t* attr;    /* [nnz]                                   */
    float* x;          /* [nnz]                                   */
    float* target;     /* [n]                                     */
} sbmf_cases;
/* libFM text "target id:value id:value ..." with any number of features per
 * line: Data::load's text branch (Data.h:173-283) with its acceptance rules
 * (:192-217: leading blanks, empty and '#' lines skipped, anything unparsable
 * an error naming the line), parsed by the threaded line-aligned parser of
 * sbmf_load_libfm with the same number rules.  Entries come back sorted by id
 * within each case (stable); a repeated id in one case is SBMF_E_ARG naming the
 * line; a negative id is SBMF_E_IO.  Text only: libFM's binary files (.x / .xt)
 * are read by the two-feature loaders above. */
int sbmf_load_libfm_cases(const char* path, sbmf_cases* out);
void sbmf_free_cases(sbmf_cases* c);
/* The fewest contiguous id ranges [bounds[r], bounds[r+1]) covering [0, num_attr)
 * such that no training case holds two attributes of one range (greedy over the
 * ascending ids, linear in nnz; attributes without a training case never
 * conflict).  draw_w / draw_v (fm_learn_mcmc.h:671-718, :780-835) touch the
 * cache of the drawn attribute's cases only, so the attributes of one range
 * commute exactly and libFM's ascending loop over them (:435-457, :555-577) is
 * one launch.  Writes *nranges and, when bounds is non-NULL, bounds[0 ..
 * *nranges]; SBMF_E_ARG when cap < *nranges + 1 (call with bounds = NULL to
 * size it) or an attribute id is >= num_attr.  Host only. */
int sbmf_fm_ranges(const sbmf_cases* train, uint32_t num_attr, uint32_t* bounds, uint32_t cap, uint32_t* nranges);
/* The training / test cases of a SBMF_METHOD_LIBFM_MCMC or SBMF_METHOD_ALS
 * context, in place of sbmf_set_train / sbmf_set_test (the arrays are copied;
 * unsorted cases are sorted, a repeated attribute is SBMF_E_ARG).  Replaces
 * Data::load + create_data_t for fm_learn_mcmc (libfm.cpp:140-171).  Any other
 * method: SBMF_E_STATE naming it.  The learner (fm_learn_mcmc.h:411-623 on the
 * GPU, csrc/fmg.cpp) then runs libFM's chain draw for draw over
 * num_attribute = max(train, test num_attr) + 1 attributes (libfm.cpp:328), one
 * launch per (range of sbmf_fm_ranges, row-length bin); sbmf_prepare, sbmf_run,
 * sbmf_predict, sbmf_get_hyper and sbmf_get_timing work as for the
 * two-attribute learner.  One rank: a context that joined a communicator or a
 * virtual rank is SBMF_E_STATE at sbmf_prepare.  sbmf_get_factors /
 * sbmf_get_biases on such a context are SBMF_E_STATE: the model is read with
 * sbmf_get_fm.  SBMF_FMM_GENERAL=1 in the environment sends the triples of
 * sbmf_set_train through this learner too (user u -> attribute u, item i ->
 * num_users + i, x = 1), for tests and for measuring the price of generality;
 * factors and biases are then read as for the two-attribute learner. */
int sbmf_set_train_cases(sbmf_ctx* ctx, const sbmf_cases* cases);
int sbmf_set_test_cases(sbmf_ctx* ctx, const sbmf_cases* cases);
/* fm_model (fm_model.h:35-60) of the general learner: w0, w[num_attribute] and
 * v[K][num_attribute] (f-major, as fm_model::v).  Any pointer may be NULL. */
int sbmf_get_fm(sbmf_ctx* ctx, double* w0, double* w, double* v);
/* num_attribute, the ranges of the training set, and the kernel launches of the
 * last iteration (0 before the first).  Any pointer may be NULL.  SBMF_E_STATE
 * on a context that does not run the general learner. */
int sbmf_fm_info(sbmf_ctx* ctx, uint32_t* num_attr, uint32_t* nranges, uint32_t* launches_per_iter);

/* --- libFM's attribute groups (bin/libFM -meta) -------------------------------------------- */
/* libFM's MCMC / ALS learner draws its hyperparameters per attribute group
 * (fm_learn_mcmc.h:931-1089 loop over meta->num_attr_groups): w_mu[g], w_lambda[g],
 * v_mu[g][f], v_lambda[g][f], and draw_w / draw_v of attribute a take its group's
 * (:445-455, :565-577).  group[a] is the group of attribute a for every a <
 * num_attribute = the largest attribute id over train and test + 2 (libFM counts a
 * trailing attribute, libfm.cpp:328; for triples the ids are user u -> u, item i ->
 * num_users + i; sbmf_fm_info reports the number after sbmf_prepare); G = the
 * largest group id + 1.  A group id no attribute carries is a group of 0 attributes:
 * its hyperparameters are still drawn (and consume variates), as in libFM.  Groups
 * need not be contiguous.  Call before sbmf_prepare on a SBMF_METHOD_LIBFM_MCMC /
 * SBMF_METHOD_ALS context; n != num_attribute is SBMF_E_ARG naming both (here when
 * the data is already set, else at sbmf_prepare); n = 0 drops the groups; another
 * method, a context that joined a communicator or a virtual rank is SBMF_E_STATE
 * naming the reason.  One group (all zeros) is the ungrouped chain, bit for bit.
 * A triples context (sbmf_set_train) given groups runs through the general learner
 * (the route of SBMF_FMM_GENERAL=1): the two-attribute kernels keep one group. */
int sbmf_set_attr_groups(sbmf_ctx* ctx, uint32_t n, const uint32_t* group);
/* -regular with 1 + 2G values (libfm.cpp:514-521): the groups' fixed (ALS) or starting
 * (MCMC) precisions regw[g] of w and regv[g] of every v[.][f]; cfg.reg0 stays w0's.
 * Without it every group takes cfg.regw / cfg.regv.  G must match the groups set by
 * sbmf_set_attr_groups (checked here when they are set, else at sbmf_prepare):
 * SBMF_E_ARG.  G = 0 drops the values.  State errors as sbmf_set_attr_groups. */
int sbmf_set_group_regular(sbmf_ctx* ctx, uint32_t G, const double* regw, const double* regv);
/* The groups and their hyperparameters after sbmf_prepare: *G, cnt[G] (attributes
 * per group, over all num_attribute ids), w_lambda[G], w_mu[G], v_lambda[G][K],
 * v_mu[G][K].  Any pointer may be NULL; works for one group too.  sbmf_get_hyper on a
 * context with G > 1 is SBMF_E_STATE and points here. */
int sbmf_get_fm_groups(sbmf_ctx* ctx, uint32_t* G, uint32_t* cnt, double* w_lambda, double* w_mu, double* v_lambda,
                       double* v_mu);
/* A -meta file (DataMetaInfo::loadGroupsFromFile, Data.h:49-61): the first num_attr
 * whitespace-separated unsigned integers into group[], *G = the largest + 1.  A file
 * with fewer entries, or an entry that is no unsigned integer, is SBMF_E_IO naming
 * the entry (sbmf_loader_error) -- the reference reads past the end there; entries
 * after the first num_attr are ignored.  Host only. */
int sbmf_load_libfm_meta(const char* path, uint32_t num_attr, uint32_t* group, uint32_t* G);

/* --- libFM's block-structure relations (bin/libFM -relation) ------------------------------- */
/* A relation holds features that are a property of one field of the cases -- the user's
 * age and occupation, the item's genres -- once per value of that field (a "block row")
 * instead of once per case (relation.h; fm_learn_mcmc.h relation_cache :57-65, draw_all
 * :458-491 and :521-620, draw_w_rel :721-777, draw_v_rel :839-899, the block rows' part
 * of predict_data_and_write_to_eterms :117-348).  The chain is the one of the same cases
 * with the block rows' features written out on every case; the relation's attributes are
 * drawn from per-block-row sums, so their passes touch block->n rows, not the cases.
 *
 * block: the block table as cases (targets ignored, target may be NULL); block->num_attr is
 * the relation's num_feature.  train_row[c] / test_row[c]: the block row case c of the train /
 * test set joins.  group[a] for a < block->num_attr with G = the number of the relation's own
 * groups (its .groups file), or NULL / 0 for one group.  Every array is copied.
 *
 * Call after the train / test data is set (sbmf_set_train_cases, or sbmf_set_train: triples
 * given a relation run through the general learner, as triples given groups do) and before
 * sbmf_prepare, once per relation in -relation order; at most 4 relations.
 *
 * Attribute ids (libfm.cpp:328-341): relation 0's attributes follow the main table's
 * num_attribute = max(train, test num_attr) + 1, relation r + 1's follow relation r's
 * block->num_attr ids (no + 1 there); num_attribute of the model is the final sum, and
 * sbmf_get_fm / sbmf_fm_info speak of that joined space.  Groups (:343-364): the main
 * table's (1, or those of sbmf_set_attr_groups, which keeps describing the main ids only),
 * then each relation's; sbmf_set_group_regular -- called after the last sbmf_add_relation --
 * and sbmf_get_fm_groups speak of the joined groups.
 *
 * SBMF_E_ARG, each naming the numbers: a row index >= block->n, a map whose length is not
 * the set's case count, an attribute repeated inside a block row, an attribute >=
 * block->num_attr, a group >= G, a fifth relation.  SBMF_E_STATE: another method (named), a
 * context that joined a communicator or is a virtual rank (named), no data yet, data
 * already prepared. */
int sbmf_add_relation(sbmf_ctx* ctx, const sbmf_cases* block, const uint32_t* train_row, uint64_t n_train,
                      const uint32_t* test_row, uint64_t n_test, const uint32_t* group, uint32_t G);
/* After sbmf_prepare: *nrel relations, and for the first min(*nrel, cap) of them the first
 * attribute id, the attribute count, the block rows, the ranges of the block table
 * (sbmf_fm_ranges applied to it: the relation's launches per row-length bin), the first
 * group id and the group count.  Any pointer may be NULL. */
int sbmf_fm_relation_info(sbmf_ctx* ctx, uint32_t* nrel, uint32_t cap, uint32_t* attr_offset, uint32_t* num_attr,
                          uint32_t* block_rows, uint32_t* nranges, uint32_t* group_offset, uint32_t* num_groups);
/* libFM's relation files (relation.h): <stem>.xt or, failing that, <stem>.x -- the block table
 * as libFM's binary sparse matrix (fmatrix.h; rows = block rows in .x, attributes in .xt) --
 * into block (targets 0; num_attr = the file's num_feature); <stem>.train / <stem>.test, the
 * block row of every case, as text (one unsigned integer per case) or as a binary
 * DVector<uint> (RelationJoin::load, relation.h:65-88); and the optional <stem>.groups into
 * *group ([block->num_attr], *G = the largest + 1; NULL and 0 without the file).  IO errors
 * (sbmf_loader_error) name the file and the entry.  Free with sbmf_free_relation.  Host only. */
int sbmf_load_libfm_relation(const char* stem, sbmf_cases* block, uint32_t** train_row, uint64_t* n_train,
                             uint32_t** test_row, uint64_t* n_test, uint32_t** group, uint32_t* G);
void sbmf_free_relation(sbmf_cases* block, uint32_t** train_row, uint32_t** test_row, uint32_t** group);
/* The writers of those files: a block table as <path> in the .x layout (rows = block rows), and
 * a map as text (binary = 0) or as a binary DVector<uint>.  Host only. */
int sbmf_save_libfm_block(const char* path, const sbmf_cases* block);
int sbmf_save_libfm_row_map(const char* path, const uint32_t* row, uint64_t n, int binary);

/* --- query list: posterior top-N of query cases over a relation's block rows ---------------- */
/* Not a reference interface: bin/libFM scores the test cases it was given.  For
 * libFM's MCMC / ALS learner (SBMF_METHOD_LIBFM_MCMC, SBMF_METHOD_ALS) with
 * relations, a query list names one relation R, the candidates, and n query
 * cases; every query holds main-table features and joins one block row of every
 * other relation.  After each iteration the learner adds, for every query q and
 * every block row j of R, libFM's prediction of "q joined to j" and its square to
 * two device-resident [n][nBp] f64 tables (nBp = R's block rows rounded up to 16):
 *   score(q, j) = ((w0 + a_q) + y_j) + sum_f s_q[f] * qB_R[j][f]
 *   s_q[f] = sum over q's entries of v[attr][f] x + sum_{r != R} qB_r[rows[r][q]][f]
 *   a_q    = sum_f 1/2 s_q[f]^2 - sum_f sum_entries 1/2 v^2 x^2 + sum_entries w x
 *            + sum_{r != R} qs_r[rows[r][q]]
 * with qB_r[j][f] = sum over block row j's entries of v x, qs_r[j] = - sum_f sum
 * 1/2 v^2 x^2 + sum w x and y_j = sum_f 1/2 qB_R[j][f]^2 + qs_R[j]: the model's
 * prediction with the square 1/2 (s + qB)^2 multiplied out (w0 / w only with the
 * -dim flags k0 / k1).  Regression adds the score, clamped to the train targets'
 * [min, max] with flags bit 0 as the test prediction is; classification adds the
 * probability cdf_gaussian(score) (flags bit 0 has no effect).  All in f64, every
 * element summed in a fixed order without atomics: a rerun gives the same bits.
 * The chain is untouched: w0, w, v, the hyperparameters and the predictions are
 * bit for bit what they are without a list, and a context without a list launches
 * what it launched before this interface existed.
 * MCMC: the tables hold every iteration run since registration (libFM's sum_all
 * has no burn-in; registering between sbmf_run calls skips early iterations).
 * ALS: the result is the latest iteration's model, as its predictions are -- the
 * tables are overwritten, the count is 1 and stdev reads back as exactly 0.
 * Memory: 16 n nBp bytes for the tables, plus the operand copies ((n + n_B) (Kp + 1)
 * doubles, Kp = K rounded up to 16) and the queries.
 *
 * sbmf_fm_query_cases: register (or replace, zeroing the tables and the count)
 * the list, after sbmf_prepare, also between sbmf_run calls; queries->n = 0 drops
 * it and frees everything.  queries: a CSR of main-table features (ids below
 * attr_offset_0 of sbmf_fm_relation_info; a query may have none; targets ignored).
 * rows: [nrel] arrays of [n] block-row indices; rows[relation] is ignored and may
 * be NULL (rows itself may be NULL with one relation).  excl_ptr[n + 1] /
 * excl_rows: a CSR of the block rows left out of query q's top-N (both NULL:
 * none).  flags bit 0: clamp.
 * SBMF_E_STATE, with a message naming the reason: a context of another method
 * (the SBPMF sampler, VB), one that joined a communicator or is a virtual rank,
 * one not prepared, one without relations; reading results before any iteration
 * ran.  SBMF_E_ARG: relation not below the number of relations; an attribute id
 * at or above attr_offset_0; a block row at or above its relation's count; a
 * missing rows[r], r != relation; an exclusion row out of range or a decreasing
 * excl_ptr; unknown flags.  SBMF_E_NOMEM with the byte count in the message (the
 * list is then dropped). */
int sbmf_fm_query_cases(sbmf_ctx* ctx, uint32_t relation, const sbmf_cases* queries, const uint32_t* const* rows,
                        const uint32_t* excl_ptr, const uint32_t* excl_rows, uint32_t flags);
/* Query q's row of posterior means and population standard deviations over the
 * iterations accumulated, one value per block row of the candidates' relation
 * ([n_B]); definitions as sbmf_watch_scores.  stdev may be NULL. */
int sbmf_fm_query_scores(sbmf_ctx* ctx, uint32_t q, double* mean, double* stdev);
/* sbmf_recommend over the block rows: per query the topn (1..1024) rows with the
 * largest mean - risk * stdev, ties by ascending row; the query's excluded rows
 * are left out unless flags bit 0 is set.  rows / mean / stdev: [n][topn]; empty
 * slots hold 0xffffffff and NaN.  stdev may be NULL. */
int sbmf_fm_query_recommend(sbmf_ctx* ctx, uint32_t topn, uint32_t flags, double risk, uint32_t* rows, double* mean,
                            double* stdev);
/* Device time (HIP events), ms, of the last iteration's query terms and operand
 * copy (two launches), of its scoring launch, and of the last selection; 0 before
 * the first. */
int sbmf_fm_query_timing(sbmf_ctx* ctx, double* ms_terms, double* ms_score, double* ms_select);

/* --- multi-GPU layout (host only) ---------------------------------------------------------- */
/* The row partition every rank uses: contiguous row blocks balanced by
 * ratings (ptr = CSR/CSC offsets [R+1]), boundaries rounded to 256 rows.
 * bounds: [nranks+1]; rank k owns rows [bounds[k], bounds[k+1]). */
int sbmf_partition_rows(const uint32_t* ptr, uint32_t R, int nranks, uint64_t* bounds);

/* --- process exit (host only; not a reference interface) -------------------------------- */
/* First call: registers an exit handler that ends the process with _Exit(rc) once
 * the exit handlers registered after it (a profiler's, e.g. rocprofv3's output
 * writer) have run, skipping the shared-library finalizers -- under rocprofv3
 * (ROCm 7.2) the HIP runtime's finalizer faults after the profiler has finished
 * (profiles/r03_rocprof_teardown.txt).  Call it before the first HIP call; later
 * calls only set rc.  The handler belongs to libsbmf: do not dlclose it after.
 * Opt-in since round 4 (SBMF_EXIT=guard in bench.py and the CLI): the fault came
 * with RCCL linked at load time, and libsbmf now loads RCCL (dlopen) only for a
 * multi-GPU communicator, so a single-GPU process of the default schedule exits
 * normally under rocprofv3; a process that launched k_gres cooperatively (tune
 * bit 24, experiments only since round 5) faulted there. */
int sbmf_exit_guard(int rc);

/* --- test hooks ---------------------------------------------------------------------------- */
/* The host glibc-compatible stream (reference mode): n values of rand(),
 * ran_gaussian() and ran_gamma(shape) for seed. */
int sbmf_ref_stream(uint32_t seed, int kind, double shape, uint64_t n, double* out);
/* Philox normals as the kernels draw them: z for (seed, sweep, tag, row, k<K). out [K]. */
int sbmf_philox_normals(uint64_t seed, uint32_t sweep, uint32_t tag, uint32_t row, uint32_t K, double* out);

/* Timing only: make this context rank `rank` of an `nranks`-rank sampler run on
 * its one GPU, with every exchange skipped (no communicator: other ranks' rows
 * keep their initial values, residuals from other ranks read as 0).  The rank
 * runs exactly its own row blocks, stages, bins and streaming tasks, so its
 * device time is the per-rank compute of the multi-GPU schedule; its numbers are
 * not a chain.  Before sbmf_prepare; the SBPMF sampler only. */
int sbmf_test_virtual_rank(sbmf_ctx* ctx, int nranks, int rank);
/* A virtual rank's device time per stage of the last sweep's halves
 * (HIP events on the compute stream): ms[side * nstages + stage]. */
int sbmf_test_stage_ms(sbmf_ctx* ctx, double* ms, uint32_t cap, uint32_t* nstages);
/* RCCL self-test on one GPU (a prepared one-rank sampler context after at least
 * one sweep): a one-rank RCCL communicator through the library's own dlopen /
 * dlsym table issues, per repetition and on the multi-GPU comm stream, the
 * exchange's calls -- one group of three in-place ncclBroadcast over adjacent
 * blocks of an nbytes buffer, the grouped ncclSend / ncclRecv of the residual
 * exchange (to the rank itself), an ncclAllGather of nbytes/4 -- while the item
 * half's persistent k_gres grids run on the compute streams.  Every byte is
 * checked; the comm stream must finish within deadline_s (else SBMF_E_COMM). */
typedef struct sbmf_rccl_selftest {
    double ms_half;        /* the repetitions' item halves on the compute stream          */
    double ms_rccl;        /* the RCCL calls on the comm stream, first to last            */
    double ms_rccl_end;    /* from the first half's start to the last RCCL call's end     */
    uint64_t bad_bcast;    /* bytes the in-place broadcasts changed (must be 0)           */
    uint64_t bad_p2p;      /* received bytes that differ from the sent ones               */
    uint64_t bad_allgather;
    uint32_t n_calls;      /* RCCL collective / point-to-point calls issued               */
    uint32_t overlapped;   /* 1: the RCCL calls finished while the halves were running    */
} sbmf_rccl_selftest;
int sbmf_test_rccl_selftest(sbmf_ctx* ctx, uint64_t nbytes, uint32_t reps, double deadline_s,
                            sbmf_rccl_selftest* out);
/* The self-test runs `reps` extra item halves on the context's live chain, so the
 * context is spent afterwards: sbmf_run returns SBMF_E_STATE on it (create a new
 * one).  On a timeout the communicator is aborted (ncclCommAbort), the buffers
 * are left allocated, and sbmf_destroy leaks the context instead of waiting on
 * its queued work. */

/* Resource audit: hipMemGetInfo of `device` and what the library holds in this
 * process right now, counted where it is created and released (every device
 * buffer, pinned host buffer, stream, event, context and RCCL communicator of
 * every learner kind).  A process that has destroyed all of its contexts holds
 * nothing: the counts return to zero. */
typedef struct sbmf_device_usage {
    uint64_t device_free, device_total; /* hipMemGetInfo                                  */
    int64_t dev_bytes, dev_allocs;      /* device buffers the library holds              */
    int64_t pinned_bytes, pinned_allocs;/* pinned host buffers                           */
    int64_t streams, events, contexts, comms;
} sbmf_device_usage;
int sbmf_test_device_usage(int device, sbmf_device_usage* out);
/* The grouped column-sums kernel (k_fmg_gsums) on the general learner's current
 * model and current mu: out[(c * G + g) * 2 + {0: gm, 1: m}] for the columns c = 0 ..
 * K (v column c, then w) and the groups g, as the next iteration's hyperparameter
 * draws would read them. */
int sbmf_test_fm_group_sums(sbmf_ctx* ctx, double* out);
/* The latent targets of libFM's classification alone: out[i] = a normal with mean mean[i] and
 * variance 1 truncated to (0, inf) where sign[i] >= 0 and to (-inf, 0) otherwise
 * (fm_learn_mcmc_simultaneous.h:197-218).  mode 0 (device): the Philox draw of the train frames
 * for the key (seed, it, index[i]) -- index: the cases' places in the train file, null for i --,
 * on `device`.  mode 1 (host, needs no GPU): the reference's ran_left_tgaussian /
 * ran_right_tgaussian restated over its own stream seeded with `seed`, consumed in the order of
 * i (`it`, `index` and `device` unused). */
int sbmf_test_tgauss(int mode, int device, uint64_t seed, uint32_t it, uint64_t n, const double* mean,
                     const int32_t* sign, const uint32_t* index, double* out);
/* The shape the lists' scoring launch takes for factor rows of Kp values (needs no GPU): the
 * rows of the list one workgroup holds in LDS, and the bytes of dynamic LDS it asks for. */
int sbmf_test_watch_lds(uint32_t Kp, uint32_t* rows, uint64_t* bytes);
/* The same for the sample store's scoring launch (a sample's user rows, their biases and ids). */
int sbmf_test_samples_lds(uint32_t Kp, uint32_t* rows, uint64_t* bytes);
/* The sample store's scoring, for tests and measurements: budget_bytes replaces the 1 GiB of
 * sbmf_samples_recommend's temporaries (0: the default); unfused bit 0 scores with one launch of the
 * watch list's kernel per stored sample into sums in memory in place of the fused kernel; bit 1 draws
 * the guests of sbmf_samples_foldin_* with the one fused launch (the sample loop inside) in place of
 * the default, one launch per sample and scan (the faster form on the device: DESIGN.md 4.8). */
int sbmf_test_samples_tune(sbmf_ctx* ctx, uint64_t budget_bytes, int unfused);

/* --- online VB: the posterior, closed-form top-N for users and guests, a model file ---------- */
/* Not a reference interface.  The online VB learner (SBMF_METHOD_VB) keeps a
 * Gaussian mean and variance for the global bias, every bias and every factor,
 * so the moments of a score need no sampling.  With user u's and item j's means
 * m, variances s (biases: w) and the global bias (m0, s0):
 *   d    = sum_f m_uf m_jf
 *   tv   = sum_f (s_uf s_jf + s_uf m_jf^2 + s_jf m_uf^2)
 *   mean = ((d + m^w_u) + m^w_j) + m0        var = ((tv + s^w_u) + s^w_j) + s0
 * stdev = sqrt(var).  These are the moments of the model's prediction: no clamp
 * (the moments of a clamped product are not closed-form) and no 1 / alpha noise
 * term.  Every call below answers from the context's current state -- before any
 * epoch, the initial one -- and leaves training untouched: an epoch after it is
 * bit-identical to one without it.
 * SBMF_E_STATE: a context that does not run the online VB learner, that joined a
 * communicator or is a virtual rank, or is not prepared.  SBMF_E_ARG: topn
 * outside 1..1024, scans outside 1..64, an id out of range, flags other than
 * bit 0 (keep rated items; a clamp bit is refused). */
/* The posterior itself; any pointer may be NULL.  U_* [num_users][K], V_*
 * [num_items][K], bu_* [num_users], bv_* [num_items], b0 = {mean, variance},
 * hyper [K + 3] = alpha, sigma_0, sigma_w, sigma_v[K]. */
int sbmf_vb_get_posterior(sbmf_ctx* ctx, double* U_mean, double* U_var, double* V_mean, double* V_var, double* bu_mean,
                          double* bu_var, double* bv_mean, double* bv_var, double* b0, double* hyper);
/* One user's full row: mean[j], stdev[j] for j < num_items (stdev may be NULL). */
int sbmf_vb_scores(sbmf_ctx* ctx, uint32_t user, double* mean, double* stdev);
/* Per named user (repeats allowed) the topn items with the largest
 * mean - risk * stdev, ties by ascending item id, the user's train items left
 * out unless flags bit 0 is set; outputs [n][topn], slots past the candidates
 * hold item 0xffffffff and NaN.  Lists longer than a device budget are served
 * in slices, with the same result. */
int sbmf_vb_recommend(sbmf_ctx* ctx, uint32_t n, const uint32_t* users, uint32_t topn, uint32_t flags, double risk,
                      uint32_t* items, double* mean, double* stdev);
/* mean[q], stdev[q] of the pairs (users[q], items[q]). */
int sbmf_vb_predict(sbmf_ctx* ctx, uint64_t n, const uint32_t* users, const uint32_t* items, double* mean, double* stdev);
/* Guests given by their ratings, the CSR of sbmf_foldin_users.  A guest's
 * posterior, items, m0 and alpha held fixed, is the learner's update_w then
 * update_v (factor-outer) at step size 1: with n ratings (j, r_j),
 *   P_b = sigma_w + alpha n,  P_f = sigma_v[f] + alpha sum_j (m_jf^2 + s_jf),
 * from b = 0, g = 0, e_j = r_j - m0 - m^w_j, `scans` (1..64) times
 *   b   <- alpha sum_j (e_j + b) / P_b;               e_j -= delta b
 *   g_f <- alpha sum_j m_jf (e_j + g_f m_jf) / P_f;    e_j -= m_jf delta g_f   (f in order)
 * and variances 1 / P_b, 1 / P_f.  A guest without ratings gets the prior.
 * Outputs row_mean, row_var [n][K], b_mean, b_var [n]; any may be NULL. */
int sbmf_vb_foldin_rows(sbmf_ctx* ctx, uint32_t n, const uint32_t* ptr, const uint32_t* items, const double* ratings,
                        uint32_t scans, double* row_mean, double* row_var, double* b_mean, double* b_var);
/* One guest's (its `len` items and ratings) full row, as sbmf_vb_scores. */
int sbmf_vb_foldin_scores(sbmf_ctx* ctx, uint32_t len, const uint32_t* items, const double* ratings, uint32_t scans,
                          double* mean, double* stdev);
/* sbmf_vb_recommend for guests; "rated" items are the guest's own. */
int sbmf_vb_foldin_recommend(sbmf_ctx* ctx, uint32_t n, const uint32_t* ptr, const uint32_t* items, const double* ratings,
                             uint32_t scans, uint32_t topn, uint32_t flags, double risk, uint32_t* out_items, double* mean,
                             double* stdev);
/* The posterior as a file (little-endian): magic "SBMFVBP1", uint32 version (1),
 * num_users, num_items, K; then float64 m0, s0, alpha, sigma_0, sigma_w,
 * sigma_v[K]; then float64 arrays in sbmf_vb_get_posterior's order: U_mean,
 * U_var, V_mean, V_var, bu_mean, bu_var, bv_mean, bv_var.
 * bytes = 24 + 8 (5 + K) + 16 (K + 1) (num_users + num_items).
 * load needs a prepared VB context of the same dims and replaces its means and
 * variances; sbmf_run on that context is then SBMF_E_STATE (the file holds no
 * natural parameters or step counts).  A file that cannot be opened, a bad
 * magic, an unknown version, a truncated file or trailing bytes: SBMF_E_IO;
 * other dims than the context's: SBMF_E_ARG; either way nothing is loaded. */
int sbmf_vb_save_posterior(sbmf_ctx* ctx, const char* path);
int sbmf_vb_load_posterior(sbmf_ctx* ctx, const char* path);
/* Reads and validates a file's header alone (no context, no GPU). */
int sbmf_vb_posterior_file_info(const char* path, uint32_t* version, uint32_t* num_users, uint32_t* num_items,
                                uint32_t* num_factor, uint64_t* bytes);
/* Device time (HIP events), ms, of the last transpose of the tables (made by the
 * first call after an epoch or a load), scoring launch, selection and guest
 * launch; 0 before the first. */
int sbmf_vb_timing(sbmf_ctx* ctx, double* ms_transpose, double* ms_score, double* ms_select, double* ms_guest);
/* Test hooks: one user's mean[j] and variance[j] as the scoring kernel wrote
 * them; the temporaries' budget of the lists in bytes (0: the default); the
 * scoring launch's rows per workgroup and LDS bytes at Kp. */
int sbmf_test_vb_moments(sbmf_ctx* ctx, uint32_t user, double* mean, double* var);
int sbmf_test_vb_tune(sbmf_ctx* ctx, uint64_t budget_bytes);
int sbmf_test_vb_score_lds(uint32_t Kp, uint32_t* rows, uint64_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* SBMF_H_ */
