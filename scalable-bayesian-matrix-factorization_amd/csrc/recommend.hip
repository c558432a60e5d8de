// recommend.hip -- gfx950 kernels of the watch list (include/sbmf.h, sbmf_watch_users):
//   k_watch_accum   one sweep's scores of the watched users against every item, added to the
//                   running first and second moments (MFMA f64 16x16x4)
//   k_watch_select  exact top-N of mean - risk * stdev per watched user
//   k_watch_mask    the watched users' rated items as a bit mask (for the selection)
//   k_watch_moments one row's mean / stdev (sbmf_watch_scores)
#include "recommend.h"

#include <cmath>

#include "recommend_dev.h"
#include "rng.h"

namespace sbmf {

// ------------------------------------------------------------------ accumulation
// A workgroup of four waves takes 16 MU watched users and WATCH_TILES item tiles of 16.  It
// gathers its users' U rows once into LDS as doubles (rows of Kp + 2: the 16 rows a quarter
// wave reads 16 bytes of fall on different banks); a wave then takes every fourth item tile:
// one pass over the tile's V rows feeds MU accumulators.  MFMA f64 16x16x4, per step: A[m][k]
// from lane m + 16 k (the users, from LDS), B[k][n] from lane n + 16 k (the items, V rows from
// memory), D[(l >> 4) + 4 j][l & 15] in acc[j] (tests/hip/mfma_layout.hip) -- items along the
// columns, so 16 lanes add to one 128-byte line of S1 and of S2.  A lane loads four
// consecutive k of its row at once (32 bytes; the four quarter waves cover 128 contiguous
// bytes of a V row): within a block of 16 k, step s multiplies column 4 (l >> 4) + s of both
// operands, a fixed permutation of the k order.  The padding columns of both tables are zero.
// A tile's old sums are loaded before its K loop and added after it (0.41 -> 0.32 ms per launch
// at ML-20M K=100, 1,024 users, together with the user groups along grid x).
// EPI (recommend.h): what becomes of a score before it meets the sums.  0 is the watch and
// fold-in lists' kernel; the libFM query list (fmq.h) adds WATCH_EPI_CDF -- the score's probit
// probability, as fm_class_test_frame forms it -- and WATCH_EPI_SET -- the sums are written, not
// added to, and the old ones never read (ALS: the latest model alone).
constexpr uint32_t WATCH_TILES = 16;

template <typename T, int MU, int EPI>
__global__ __launch_bounds__(256) void k_watch_accum(const uint32_t* __restrict__ users, uint32_t n,
                                                     const T* __restrict__ U, const T* __restrict__ V, uint32_t J,
                                                     uint32_t Jp, uint32_t Kp, const double* __restrict__ bu,
                                                     const double* __restrict__ bv, double b0, int clamp, double lo,
                                                     double hi, double* __restrict__ S1, double* __restrict__ S2) {
    extern __shared__ double us[];  // [16 MU][Kp + 2], then the rows' user ids
    const uint32_t ld = Kp + 2;
    uint32_t* uid = reinterpret_cast<uint32_t*>(us + (size_t)16 * MU * ld);
    const uint32_t w0 = blockIdx.x * 16 * MU;
    if (threadIdx.x < 16 * MU) uid[threadIdx.x] = w0 + threadIdx.x < n ? users[w0 + threadIdx.x] : 0u;
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < 16 * MU * Kp; x += 256) {
        const uint32_t r = x / Kp, k = x - r * Kp;
        us[r * ld + k] = w0 + r < n ? (double)U[(size_t)uid[r] * Kp + k] : 0.0;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t n16 = lane & 15, kq = lane >> 4;
    const uint32_t ntile = Jp / 16;
    const uint32_t tend = min(ntile, (blockIdx.y + 1) * WATCH_TILES);
    for (uint32_t tile = blockIdx.y * WATCH_TILES + wave; tile < tend; tile += 4) {
        const uint32_t item = tile * 16 + n16;
        const T* vp = V + (size_t)min(item, J - 1) * Kp + 4 * kq;  // a padding item reads the last row (not stored)
        wd4 acc[MU];
#pragma unroll
        for (int t = 0; t < MU; ++t) acc[t] = wd4{0, 0, 0, 0};
        // the old sums, asked for before the K loop so that they arrive under it
        double o1[MU][4], o2[MU][4];
        if constexpr (!(EPI & WATCH_EPI_SET)) {
#pragma unroll
            for (int t = 0; t < MU; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t w = w0 + t * 16 + kq + 4 * j;
                    const bool ok = w < n && item < J;
                    const size_t o = ok ? (size_t)w * Jp + item : 0;
                    o1[t][j] = ok ? S1[o] : 0.0;
                    o2[t][j] = ok ? S2[o] : 0.0;
                }
        }
        watch_tile_products<T, MU>(us, ld, vp, Kp, w0, n, n16, kq, acc);
        if (item >= J) continue;
        const double bj = bu ? bv[item] : 0.0;
#pragma unroll
        for (int t = 0; t < MU; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t r = t * 16 + kq + 4 * j, w = w0 + r;
                if (w >= n) continue;
                double s = watch_biased(acc[t][j], bu != nullptr, b0, bu ? bu[uid[r]] : 0.0, bj);
                if constexpr (EPI & WATCH_EPI_CDF) s = ref_cdf_gaussian(s);
                s = watch_clamped(s, clamp, lo, hi);
                const size_t o = (size_t)w * Jp + item;
                if constexpr (EPI & WATCH_EPI_SET) {
                    S1[o] = s;
                    S2[o] = s * s;
                } else {
                    watch_sums_add(o1[t][j], o2[t][j], s, S1[o], S2[o]);
                }
            }
    }
}

template <typename T, int MU, int EPI>
static hipError_t watch_accum_mu(const uint32_t* users, uint32_t n, const T* U, const T* V, uint32_t J, uint32_t Kp,
                                 const double* bu, const double* bv, double b0, int clamp, double lo, double hi,
                                 double* S1, double* S2, hipStream_t st) {
    const uint32_t Jp = watch_jp(J);
    // the user groups along x: workgroups launched together read the same V rows
    const dim3 grid((n + 16 * MU - 1) / (16 * MU), (Jp / 16 + WATCH_TILES - 1) / WATCH_TILES);
    const size_t lds = watch_lds_bytes(MU, Kp);
    k_watch_accum<T, MU, EPI><<<grid, 256, lds, st>>>(users, n, U, V, J, Jp, Kp, bu, bv, b0, clamp, lo, hi, S1, S2);
    return hipGetLastError();
}

template <typename T, int EPI>
static hipError_t watch_accum_epi(const uint32_t* users, uint32_t n, const T* U, const T* V, uint32_t J, uint32_t Kp,
                                  const double* bu, const double* bv, double b0, int clamp, double lo, double hi,
                                  double* S1, double* S2, hipStream_t st) {
    if (n == 0 || J == 0) return hipSuccess;
    // users per workgroup: as many as 64 KB of LDS hold (watch_mu, recommend.h)
    switch (watch_mu(Kp)) {
        case 4:
            return watch_accum_mu<T, 4, EPI>(users, n, U, V, J, Kp, bu, bv, b0, clamp, lo, hi, S1, S2, st);
        case 2:
            return watch_accum_mu<T, 2, EPI>(users, n, U, V, J, Kp, bu, bv, b0, clamp, lo, hi, S1, S2, st);
    }
    return watch_accum_mu<T, 1, EPI>(users, n, U, V, J, Kp, bu, bv, b0, clamp, lo, hi, S1, S2, st);
}

template <typename T>
hipError_t launch_watch_accum(const uint32_t* users, uint32_t n, const T* U, const T* V, uint32_t J, uint32_t Kp,
                              const double* bu, const double* bv, double b0, int clamp, double lo, double hi,
                              double* S1, double* S2, hipStream_t st) {
    return watch_accum_epi<T, 0>(users, n, U, V, J, Kp, bu, bv, b0, clamp, lo, hi, S1, S2, st);
}
template hipError_t launch_watch_accum<double>(const uint32_t*, uint32_t, const double*, const double*, uint32_t,
                                               uint32_t, const double*, const double*, double, int, double, double,
                                               double*, double*, hipStream_t);
template hipError_t launch_watch_accum<float>(const uint32_t*, uint32_t, const float*, const float*, uint32_t, uint32_t,
                                              const double*, const double*, double, int, double, double, double*,
                                              double*, hipStream_t);

hipError_t launch_watch_accum_epi(int epi, const uint32_t* rows, uint32_t n, const double* A, const double* B,
                                  uint32_t J, uint32_t Kp, const double* ba, const double* bb, double b0, int clamp,
                                  double lo, double hi, double* S1, double* S2, hipStream_t st) {
    if (!ba || !bb) return hipErrorInvalidValue;
    switch (epi) {
        case 0:
            return watch_accum_epi<double, 0>(rows, n, A, B, J, Kp, ba, bb, b0, clamp, lo, hi, S1, S2, st);
        case WATCH_EPI_CDF:
            return watch_accum_epi<double, WATCH_EPI_CDF>(rows, n, A, B, J, Kp, ba, bb, b0, clamp, lo, hi, S1, S2, st);
        case WATCH_EPI_SET:
            return watch_accum_epi<double, WATCH_EPI_SET>(rows, n, A, B, J, Kp, ba, bb, b0, clamp, lo, hi, S1, S2, st);
        case WATCH_EPI_CDF | WATCH_EPI_SET:
            return watch_accum_epi<double, WATCH_EPI_CDF | WATCH_EPI_SET>(rows, n, A, B, J, Kp, ba, bb, b0, clamp, lo, hi, S1,
                                                                         S2, st);
    }
    return hipErrorInvalidValue;
}

// ------------------------------------------------------------------ moments and keys
// (watch_moments, the one place for the mean / stdev expressions: recommend_dev.h)
// The key as an unsigned integer of the same order (a larger key is a larger integer); -0 as +0.
__device__ __forceinline__ uint64_t watch_key(double mean, double sd, double risk) {
#pragma clang fp contract(off)
    const double rs = risk * sd;
    double key = mean - rs;
    if (key == 0.0) key = 0.0;
    const uint64_t b = (uint64_t)__double_as_longlong(key);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ __launch_bounds__(256) void k_watch_moments(const double* __restrict__ s1, const double* __restrict__ s2,
                                                       uint32_t J, double nw, double* __restrict__ mean,
                                                       double* __restrict__ sd) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= J) return;
    double m, s;
    watch_moments(s1[j], s2[j], nw, m, s);
    mean[j] = m;
    if (sd) sd[j] = s;
}

hipError_t launch_watch_moments(const double* s1, const double* s2, uint32_t J, double nw, double* mean, double* sd,
                                hipStream_t st) {
    if (J == 0) return hipSuccess;
    k_watch_moments<<<(J + 255) / 256, 256, 0, st>>>(s1, s2, J, nw, mean, sd);
    return hipGetLastError();
}

// ------------------------------------------------------------------ rated-item mask
__global__ __launch_bounds__(256) void k_watch_mask(const uint32_t* __restrict__ users,
                                                    const uint32_t* __restrict__ uptr,
                                                    const uint32_t* __restrict__ upart, uint32_t* __restrict__ mask,
                                                    uint32_t Jw) {
    const uint32_t u = users[blockIdx.x];
    uint32_t* m = mask + (size_t)blockIdx.x * Jw;
    for (uint32_t q = uptr[u] + threadIdx.x; q < uptr[u + 1]; q += 256) {
        const uint32_t it = upart[q];
        if ((it >> 5) < Jw) atomicOr(&m[it >> 5], 1u << (it & 31));  // an OR: the order does not matter
    }
}

hipError_t launch_watch_mask(const uint32_t* users, uint32_t n, const uint32_t* uptr, const uint32_t* upart,
                             uint32_t* mask, uint32_t Jw, hipStream_t st) {
    if (n == 0) return hipSuccess;
    k_watch_mask<<<n, 256, 0, st>>>(users, uptr, upart, mask, Jw);
    return hipGetLastError();
}

// ------------------------------------------------------------------ selection
// One workgroup of 1024 threads per watched user; thread t holds items t, t + 1024, ...
// CACHED (J <= 32768): the row is read once and every candidate's key stays in registers (32
// per thread); otherwise a key is formed again from S1 / S2 wherever it is used.  A key of 0
// marks a non-candidate (a rated item, or a slot past J).
// The order is total: key descending, then item ascending, i.e. the 96-bit number
// (key, ~item) descending.  A radix select over its twelve 8-bit digits, most significant
// first, finds the topn-th largest such number: per digit a 256-bin count of the elements that
// match the digits chosen so far (integer LDS atomics: the counts do not depend on the order),
// and a scan from the top bin for the one that holds rank `rem`.  The elements at or above the
// threshold -- exactly topn of them, or every candidate if there are fewer -- go to LDS and
// are put in order by a bitonic sort of 1024 slots; empty slots (key 0, item all ones) sort last.
// GIVEN: the two rows are a mean and a variance (watch_given_moments), not sums over nw samples.
constexpr int WATCH_P = 32;

template <bool CACHED, bool GIVEN = false>
__global__ __launch_bounds__(1024) void k_watch_select(const double* __restrict__ S1, const double* __restrict__ S2,
                                                       uint32_t Jp, uint32_t J, double nw, double risk,
                                                       const uint32_t* __restrict__ mask, uint32_t Jw, uint32_t topn,
                                                       uint32_t* __restrict__ out_items, double* __restrict__ out_mean,
                                                       double* __restrict__ out_sd) {
    const uint32_t tid = threadIdx.x;
    const double* s1 = S1 + (size_t)blockIdx.x * Jp;
    const double* s2 = S2 + (size_t)blockIdx.x * Jp;
    const uint32_t* mk = mask ? mask + (size_t)blockIdx.x * Jw : nullptr;
    auto key_of = [&](uint32_t item) -> uint64_t {
        if (mk && ((mk[item >> 5] >> (item & 31)) & 1u)) return 0;
        double m, sd;
        if constexpr (GIVEN) watch_given_moments(s1[item], s2[item], m, sd);
        else watch_moments(s1[item], s2[item], nw, m, sd);
        return watch_key(m, sd, risk);
    };
    uint64_t kreg[CACHED ? WATCH_P : 1];
    if constexpr (CACHED) {
#pragma unroll
        for (int i = 0; i < WATCH_P; ++i) {
            const uint32_t item = (uint32_t)i * 1024 + tid;
            kreg[i] = item < J ? key_of(item) : 0;
        }
    }
// BODY sees `item` and its `key` for each of this thread's elements
#define WATCH_EACH(BODY)                                            \
    if constexpr (CACHED) {                                         \
        _Pragma("unroll") for (int i_ = 0; i_ < WATCH_P; ++i_) {    \
            const uint32_t item = (uint32_t)i_ * 1024 + tid;        \
            const uint64_t key = kreg[i_];                          \
            BODY                                                    \
        }                                                           \
    } else {                                                        \
        for (uint32_t item = tid; item < J; item += 1024) {         \
            const uint64_t key = key_of(item);                      \
            BODY                                                    \
        }                                                           \
    }

    __shared__ uint32_t hist[256];
    __shared__ uint32_t sel[3];  // digit, rank left inside it, 1: fewer candidates than topn
    __shared__ uint64_t skey[1024];
    __shared__ uint32_t sitem[1024];
    __shared__ uint32_t cnt;
    uint64_t pk = 0, kmask = 0;  // the chosen digits of the key and of ~item so far
    uint32_t pi = 0, imask = 0;
    uint32_t rem = topn;
    bool all = false;
    for (int d = 0; d < 12 && !all; ++d) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const int sh = d < 8 ? 56 - 8 * d : 24 - 8 * (d - 8);
        WATCH_EACH({
            const uint32_t ni = ~item;
            if (key && (key & kmask) == pk && (ni & imask) == pi)
                atomicAdd(&hist[d < 8 ? (uint32_t)(key >> sh) & 255u : (ni >> sh) & 255u], 1u);
        })
        __syncthreads();
        if (tid == 0) {
            uint32_t cum = 0;
            int b = 255;
            for (; b >= 0; --b) {
                const uint32_t c = hist[b];
                if (cum + c >= rem) break;
                cum += c;
            }
            sel[0] = (uint32_t)max(b, 0);
            sel[1] = rem - cum;
            sel[2] = b < 0 ? 1u : 0u;
        }
        __syncthreads();
        all = sel[2] != 0;
        rem = sel[1];
        if (d < 8) {
            pk |= (uint64_t)sel[0] << sh;
            kmask |= 0xffull << sh;
        } else {
            pi |= sel[0] << sh;
            imask |= 0xffu << sh;
        }
    }
    skey[tid] = 0;
    sitem[tid] = 0xffffffffu;
    if (tid == 0) cnt = 0;
    __syncthreads();
    WATCH_EACH({
        if (key && (all || key > pk || (key == pk && ~item >= pi))) {
            const uint32_t slot = atomicAdd(&cnt, 1u);
            if (slot < 1024) {
                skey[slot] = key;
                sitem[slot] = item;
            }
        }
    })
#undef WATCH_EACH
    __syncthreads();
    for (uint32_t k = 2; k <= 1024; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint32_t o = tid ^ j;
            if (o > tid) {
                const uint64_t ka = skey[tid], kb = skey[o];
                const uint32_t ia = sitem[tid], ib = sitem[o];
                const bool a_first = ka > kb || (ka == kb && ia < ib);
                const bool b_first = kb > ka || (ka == kb && ib < ia);
                if ((tid & k) == 0 ? b_first : a_first) {
                    skey[tid] = kb, skey[o] = ka;
                    sitem[tid] = ib, sitem[o] = ia;
                }
            }
            __syncthreads();
        }
    if (tid < topn) {
        const uint32_t it = sitem[tid];
        double m = NAN, sd = NAN;
        if (it != 0xffffffffu) {
            if constexpr (GIVEN) watch_given_moments(s1[it], s2[it], m, sd);
            else watch_moments(s1[it], s2[it], nw, m, sd);
        }
        const size_t o = (size_t)blockIdx.x * topn + tid;
        out_items[o] = it;
        out_mean[o] = m;
        if (out_sd) out_sd[o] = sd;
    }
}

hipError_t launch_watch_select(uint32_t n, const double* S1, const double* S2, uint32_t J, double nw, double risk,
                               const uint32_t* mask, uint32_t topn, uint32_t* items, double* mean, double* sd,
                               hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (topn == 0 || topn > 1024) return hipErrorInvalidValue;
    const uint32_t Jp = watch_jp(J), Jw = watch_jw(J);
    if (J <= (uint32_t)WATCH_P * 1024)
        k_watch_select<true><<<n, 1024, 0, st>>>(S1, S2, Jp, J, nw, risk, mask, Jw, topn, items, mean, sd);
    else
        k_watch_select<false><<<n, 1024, 0, st>>>(S1, S2, Jp, J, nw, risk, mask, Jw, topn, items, mean, sd);
    return hipGetLastError();
}

hipError_t launch_watch_select_given(uint32_t n, const double* M, const double* Vr, uint32_t J, double risk,
                                     const uint32_t* mask, uint32_t topn, uint32_t* items, double* mean, double* sd,
                                     hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (topn == 0 || topn > 1024) return hipErrorInvalidValue;
    const uint32_t Jp = watch_jp(J), Jw = watch_jw(J);
    if (J <= (uint32_t)WATCH_P * 1024)
        k_watch_select<true, true><<<n, 1024, 0, st>>>(M, Vr, Jp, J, 1.0, risk, mask, Jw, topn, items, mean, sd);
    else
        k_watch_select<false, true><<<n, 1024, 0, st>>>(M, Vr, Jp, J, 1.0, risk, mask, Jw, topn, items, mean, sd);
    return hipGetLastError();
}

}  // namespace sbmf
