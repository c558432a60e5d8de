// foldin.hip -- gfx950 kernel of the fold-in list (include/sbmf.h, sbmf_foldin_users):
//   k_foldin   one draw of every guest's factor row from the user half's row conditional,
//              given the sweep's item factors (Gram blocks by MFMA f64 16x16x4)
// The guests' scores, rated-item mask and selection are the watch list's kernels (recommend.hip).
#include "foldin.h"

#include "foldin_dev.h"

namespace sbmf {

// One workgroup per guest (foldin_dev.h): the row, the sweep's [sg | mu] and the normals into LDS,
// one scan against the sweep's V, the row rounded once on store.
template <typename T>
__global__ __launch_bounds__(FOLDIN_NT) void k_foldin(const uint32_t* __restrict__ order, const uint32_t* __restrict__ ptr,
                                                      const uint32_t* __restrict__ items,
                                                      const double* __restrict__ ratings, T* __restrict__ G,
                                                      const T* __restrict__ V, uint32_t K, uint32_t Kp,
                                                      const double* __restrict__ hyper, double tau, int sd_is_var,
                                                      uint64_t seed, uint32_t sweep, double* E) {
    __shared__ FoldinLds L;
    const uint32_t g = order[blockIdx.x], tid = threadIdx.x;
    const uint32_t beg = ptr[g], ng = ptr[g + 1] - beg;
    T* grow = G + (size_t)g * Kp;
    for (uint32_t k = tid; k < Kp; k += FOLDIN_NT) {
        L.urow[k] = (double)grow[k];
        L.hyp[k] = hyper[k];
        L.hyp[FOLDIN_KP_MAX + k] = hyper[Kp + k];
    }
    foldin_normals(L, seed, g, sweep, 0, Kp, tid);
    __syncthreads();
    foldin_scan<T>(L, items + beg, ratings + beg, E + beg, ng, V, K, Kp, tau, sd_is_var, tid);
    for (uint32_t k = tid; k < Kp; k += FOLDIN_NT) grow[k] = (T)L.urow[k];  // padding columns: zero
}

template <typename T>
hipError_t launch_foldin(uint32_t n, const uint32_t* order, const uint32_t* ptr, const uint32_t* items,
                         const double* ratings, T* G, const T* V, uint32_t K, uint32_t Kp, const double* hyper,
                         double tau, int sd_is_var, uint64_t seed, uint32_t sweep, double* E, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (Kp > FOLDIN_KP_MAX || Kp % 16 || K > Kp) return hipErrorInvalidValue;
    k_foldin<T><<<n, FOLDIN_NT, 0, st>>>(order, ptr, items, ratings, G, V, K, Kp, hyper, tau, sd_is_var, seed, sweep, E);
    return hipGetLastError();
}
template hipError_t launch_foldin<double>(uint32_t, const uint32_t*, const uint32_t*, const uint32_t*, const double*,
                                          double*, const double*, uint32_t, uint32_t, const double*, double, int,
                                          uint64_t, uint32_t, double*, hipStream_t);
template hipError_t launch_foldin<float>(uint32_t, const uint32_t*, const uint32_t*, const uint32_t*, const double*,
                                         float*, const float*, uint32_t, uint32_t, const double*, double, int, uint64_t,
                                         uint32_t, double*, hipStream_t);

}  // namespace sbmf
