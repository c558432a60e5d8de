// kernels_instr.h -- diagnostic instrumentation of the row kernels (kernels.hip).
// Never part of the product build: the Makefile pre-includes it (-include) only
// for CHECK=1 / KPROF=1 builds, which go to their own output directory
// (OUT=../build_check, ../build_kprof).  kernels.hip defines these hooks away
// when this header is absent.
#pragma once
#define SBMF_KERNELS_INSTR_H_ 1

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#ifdef SBMF_CHECK_BUILD
// CHECK=1: CHK(i, extent) validates a global index; a violation is printed (the
// first 32 over the process) and the access goes to element 0 instead, so a bad
// index is reported without faulting the device.
__device__ unsigned int g_chk_count = 0;
__device__ __noinline__ uint64_t chk_fail(uint64_t i, uint64_t lim, int line) {
    if (atomicAdd(&g_chk_count, 1u) < 32u)
        printf("[sbmf check] kernels.hip:%d index %llu >= extent %llu (block %u thread %u)\n", line,
               (unsigned long long)i, (unsigned long long)lim, blockIdx.x, threadIdx.x);
    return 0;
}
#define CHK(i, lim) ((uint64_t)(i) < (uint64_t)(lim) ? (uint64_t)(i) : chk_fail((uint64_t)(i), (uint64_t)(lim), __LINE__))
// a split row's partial whose bits equal the slab sentinel (kernels.hip, XSENT): its readers
// would wait for it until their spin gives up
__device__ __noinline__ void xsent_fail(int line) {
    if (atomicAdd(&g_chk_count, 1u) < 32u)
        printf("[sbmf check] kernels.hip:%d a partial has the sentinel's bits (block %u thread %u)\n", line, blockIdx.x,
               threadIdx.x);
}
#define SBMF_XSENT_CHECK(bad) do { if (bad) xsent_fail(__LINE__); } while (0)
#else
#define CHK(i, lim) (i)
#define SBMF_XSENT_CHECK(bad) ((void)0)
#endif

#ifdef SBMF_KPROF_BUILD
// KPROF=1 (run with SBMF_KPROF=1): wave 0's clock cycles per phase, added into
// a.prof / the streaming kernels' cold block's prof (sbmf.cpp prints them).  k_gblock: multi-wave rows only.
// k_gres: also per chunk-count class (whole rows / 2..16 chunks / more) at
// [32 + 24*SIDE + 8*cls], slot 7 of a class counting its tasks.  A split row's exchange is
// stamped in three parts: 7 (the cross-wave sum and the publish) and 8 (from the publish to
// wave 0's first valid batch; stamp_first: once per block) go to [96 + 2*SIDE + ph - 7] and,
// per class, [100 + 6*SIDE + 2*cls + ph - 7]; the rest (read + sum) is phase 4.
#define SBMF_GBLOCK_PHASES(on)                                                   \
    unsigned long long tp_ = (a.prof && threadIdx.x == 0) ? clock64() : 0ull;   \
    auto stamp = [&](int ph) {                                                   \
        if ((on) && a.prof && threadIdx.x == 0) {                                \
            const unsigned long long now = clock64();                            \
            atomicAdd(&a.prof[ph], now - tp_);                                   \
            tp_ = now;                                                           \
        }                                                                        \
    }
#define SBMF_GRES_PHASES(nch, prof_)                                                                        \
    unsigned long long tp_ = ((prof_) && threadIdx.x == 0) ? clock64() : 0ull;                         \
    unsigned long long* const pcls_ =                                                                  \
        (prof_) ? (prof_) - 8 * SIDE + 32 + 24 * SIDE + 8 * ((nch) == 1 ? 0 : (nch) <= 16 ? 1 : 2) : nullptr; \
    if ((prof_) && threadIdx.x == 0) atomicAdd(&pcls_[7], 1ull);                                       \
    bool xfirst_ = false;                                                                              \
    auto stamp = [&](int ph) {                                                                         \
        if ((prof_) && threadIdx.x == 0) {                                                             \
            const unsigned long long now = clock64();                                                  \
            unsigned long long* const base_ = (prof_) - 8 * SIDE;                                      \
            const long cls_ = (pcls_ - base_ - 32 - 24 * SIDE) / 8;                                    \
            atomicAdd(ph < 7 ? &(prof_)[ph] : &base_[96 + 2 * SIDE + ph - 7], now - tp_);              \
            atomicAdd(ph < 7 ? &pcls_[ph] : &base_[100 + 6 * SIDE + 2 * cls_ + ph - 7], now - tp_);    \
            tp_ = now;                                                                                 \
            xfirst_ = ph == 7;                                                                         \
        }                                                                                              \
    };                                                                                                 \
    auto stamp_first = [&](int ph) {                                                                   \
        if (xfirst_) stamp(ph);                                                                        \
    }
#else
#define SBMF_GBLOCK_PHASES(on) auto stamp = [](int) {}
#define SBMF_GRES_PHASES(nch, prof_) \
    auto stamp = [](int) {};         \
    auto stamp_first = [](int) {}
#endif
