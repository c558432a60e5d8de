// samples_foldin.hip -- gfx950 kernels that fold guests into the posterior sample store after the
// run (include/sbmf.h, sbmf_samples_foldin_recommend):
//   k_samples_foldin_step  every guest's factor row at one stored sample, one scan of it per launch
//                          (the default: the faster form on the device)
//   k_samples_foldin       its fused twin: every sample and scan inside one launch (a test hook)
// The scan is k_foldin's (foldin_dev.h); scores and selection are the store's and the watch
// list's kernels (samples.hip, recommend.hip).
#include "samples_foldin.h"

#include "foldin_dev.h"

namespace sbmf {

// the s-th oldest sample's V
template <typename T>
__device__ __forceinline__ const T* sample_v(const SampleView& sv, uint32_t s, uint32_t& slot) {
    const uint32_t p = sv.head + s;  // head < cap, s < cap <= 65535
    slot = p >= sv.cap ? p - sv.cap : p;
    return static_cast<const T*>(sv.V) + (size_t)slot * sv.sv;
}

// sample s's [sg | mu] into LDS
__device__ __forceinline__ void sample_hyper(FoldinLds& L, const double* __restrict__ hyper, uint32_t s, uint32_t Kp) {
    const double* h = hyper + (size_t)s * 2 * Kp;
    for (uint32_t k = threadIdx.x; k < Kp; k += FOLDIN_NT) {
        L.hyp[k] = h[k];
        L.hyp[FOLDIN_KP_MAX + k] = h[Kp + k];
    }
}

// One workgroup of 16 waves per guest, the longest first, as k_foldin.  The row stays in LDS over
// the whole sample loop; what a scan leaves behind it (foldin_scan's exit) is safe to overwrite,
// so a sample costs its hyperparameters' and normals' loads, one barrier, and its scans.
template <typename T>
__global__ __launch_bounds__(FOLDIN_NT) void k_samples_foldin(SamplesFoldinArgs a) {
    __shared__ FoldinLds L;
    const uint32_t g = a.order[blockIdx.x], tid = threadIdx.x, Kp = a.Kp;
    const uint32_t beg = a.ptr[g], ng = a.ptr[g + 1] - beg;
    for (uint32_t k = tid; k < Kp; k += FOLDIN_NT) L.urow[k] = 0.0;
    for (uint32_t s = 0; s < a.sv.count; ++s) {
        uint32_t slot;
        const T* V = sample_v<T>(a.sv, s, slot);
        const double tau = a.tau[s];
        const uint32_t sweep = a.sweeps[s];
        sample_hyper(L, a.hyper, s, Kp);
        for (uint32_t r = 0; r < a.scans; ++r) {
            // what a scan derives from the thread's index is derived again per scan, not held in
            // registers over the whole loop nest (the kernel then fits the 128 of a 16-wave workgroup)
            uint32_t t = tid;
            asm volatile("" : "+v"(t));
            foldin_normals(L, a.seed, g, sweep, r, Kp, t);
            __syncthreads();
            foldin_scan<T>(L, a.items + beg, a.ratings + beg, a.E + beg, ng, V, a.K, Kp, tau, a.sd_is_var, t);
        }
        // the row as the chain's table would hold it (padding columns: zero); thread k owns
        // urow[k] here, and the next scan's barrier orders it before any other thread's read
        T* grow = static_cast<T*>(a.GS) + (size_t)slot * a.gs + (size_t)(g - a.g0) * Kp;
        for (uint32_t k = tid; k < Kp; k += FOLDIN_NT) {
            const T u = (T)L.urow[k];
            grow[k] = u;
            L.urow[k] = (double)u;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(FOLDIN_NT) void k_samples_foldin_step(SamplesFoldinArgs a, uint32_t s, uint32_t r,
                                                                   double* __restrict__ carry) {
    __shared__ FoldinLds L;
    const uint32_t g = a.order[blockIdx.x], tid = threadIdx.x, Kp = a.Kp;
    const uint32_t beg = a.ptr[g], ng = a.ptr[g + 1] - beg;
    double* crow = carry + (size_t)(g - a.g0) * Kp;
    uint32_t slot;
    const T* V = sample_v<T>(a.sv, s, slot);
    for (uint32_t k = tid; k < Kp; k += FOLDIN_NT) L.urow[k] = crow[k];
    sample_hyper(L, a.hyper, s, Kp);
    foldin_normals(L, a.seed, g, a.sweeps[s], r, Kp, tid);
    __syncthreads();
    foldin_scan<T>(L, a.items + beg, a.ratings + beg, a.E + beg, ng, V, a.K, Kp, a.tau[s], a.sd_is_var, tid);
    const bool last = r + 1 == a.scans;
    T* grow = static_cast<T*>(a.GS) + (size_t)slot * a.gs + (size_t)(g - a.g0) * Kp;
    for (uint32_t k = tid; k < Kp; k += FOLDIN_NT) {
        if (last) {
            const T u = (T)L.urow[k];
            grow[k] = u;
            crow[k] = (double)u;
        } else {
            crow[k] = L.urow[k];
        }
    }
}

static bool samples_foldin_ok(const SamplesFoldinArgs& a) {
    return a.Kp <= FOLDIN_KP_MAX && a.Kp % 16 == 0 && a.K <= a.Kp && a.scans >= 1 && a.scans <= SAMPLES_FOLDIN_SCANS_MAX &&
           a.sv.count >= 1 && a.sv.count <= a.sv.cap && a.sv.head < a.sv.cap && a.gs >= ((size_t)a.n + 2) * a.Kp;
}

template <typename T>
hipError_t launch_samples_foldin(const SamplesFoldinArgs& a, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    if (!samples_foldin_ok(a)) return hipErrorInvalidValue;
    k_samples_foldin<T><<<a.n, FOLDIN_NT, 0, st>>>(a);
    return hipGetLastError();
}
template hipError_t launch_samples_foldin<double>(const SamplesFoldinArgs&, hipStream_t);
template hipError_t launch_samples_foldin<float>(const SamplesFoldinArgs&, hipStream_t);

template <typename T>
hipError_t launch_samples_foldin_step(const SamplesFoldinArgs& a, uint32_t s, uint32_t r, double* carry, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    if (!samples_foldin_ok(a) || s >= a.sv.count || r >= a.scans) return hipErrorInvalidValue;
    k_samples_foldin_step<T><<<a.n, FOLDIN_NT, 0, st>>>(a, s, r, carry);
    return hipGetLastError();
}
template hipError_t launch_samples_foldin_step<double>(const SamplesFoldinArgs&, uint32_t, uint32_t, double*, hipStream_t);
template hipError_t launch_samples_foldin_step<float>(const SamplesFoldinArgs&, uint32_t, uint32_t, double*, hipStream_t);

}  // namespace sbmf
