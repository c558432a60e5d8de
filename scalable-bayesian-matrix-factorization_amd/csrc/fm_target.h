// fm_target.h -- libFM's classification task (-task c, a probit model) in the prediction frames
// of the two libFM learners (fmm.h, fmg.h; the frames themselves are fm_dev.h's).
//
// Each train case keeps a latent Gaussian target on its label's side of 0; the residual the
// passes work on is e = prediction - latent target (fm_learn_mcmc_simultaneous.h:176-222).  The
// train frame forms it in the pass that predicts the case, in one of three ways:
//   FM_TGT_ALS     the truncated normal's expected value as the reference writes it (:203-216)
//   FM_TGT_PHILOX  a draw on the device from the counter-based stream of (seed, iteration, the
//                  case's index in the train file): a function of that key and the prediction
//                  alone, so neither the layout nor the launch geometry changes it.  The
//                  reference's two rejection algorithms (random.h:72-102), each bounded to 64
//                  tries, after which the draw is the truncation point itself.  The naive branch
//                  accepts with probability >= 1/2 (64 rejections: <= 2^-64), Robert's translated
//                  exponential with probability >= 0.76 (<= 2^-131).
//   FM_TGT_HOST    the reference's own stream.  Its rejection loops consume the sequential glibc
//                  stream a data-dependent number of times per case, so the host draws: the frame
//                  leaves the prediction in the residual and in yhat, the host draws case by case
//                  in the train file's order (rng.h), uploads the targets, and fm*_sub_targets
//                  subtracts them.  One download, one serial host loop and one upload of N
//                  doubles per iteration: this mode is for parity with the reference, not speed.
#pragma once
#include <cstdint>

namespace sbmf {

enum { FM_TGT_ALS = 0, FM_TGT_PHILOX = 1, FM_TGT_HOST = 2 };

struct FMTargetArgs {
    int mode;              // FM_TGT_*
    uint64_t seed;         // FM_TGT_PHILOX: the key's seed and iteration
    uint32_t it;
    const uint32_t* fidx;  // FM_TGT_PHILOX: [n] the train file index of the case at each position (null: the position)
    double* yhat;          // FM_TGT_HOST: [n] the predictions, by position
    uint32_t* cnt;         // [blocks] the cases each 256-case block classifies correctly
};

}  // namespace sbmf
