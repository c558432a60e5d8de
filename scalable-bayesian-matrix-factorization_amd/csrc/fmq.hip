// fmq.hip -- gfx950 kernels of the libFM learner's query list (fmq.h): the queries' terms and
// the candidates' operands of an iteration.  The scores themselves are the watch list's
// accumulation kernel's (recommend.hip, launch_watch_accum_epi).
#include "fmq.h"

namespace sbmf {

namespace {
__device__ __forceinline__ double fmq_wsum(double x) {  // xor butterfly: bit-identical in every lane
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}
}  // namespace

// One wave per query (four to a workgroup), lane l takes the factors l, l + 64, ...: per factor
// the entries in ascending attribute and then the other relations in relation order, as fg_pred
// forms its q; the lane's shares of sum_f 1/2 s^2 and of -sum 1/2 v^2 x^2 in ascending f, then the
// butterfly.  The w and q-terms are added by every lane alike (uniform loads).
__global__ __launch_bounds__(256) void k_fmq_terms(FMQTermsArgs a) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.nq) return;
    const uint32_t j0 = a.ptr[q], j1 = a.ptr[q + 1];
    uint32_t br[FG_MAX_REL];
#pragma unroll
    for (uint32_t r = 0; r < FG_MAX_REL; ++r) br[r] = r < a.nrel ? a.rel[r].rows[q] : 0u;
    double e = 0.0, q2 = 0.0;
    for (uint32_t f = lane; f < a.Kp; f += 64) {
        double s = 0.0;
        if (f < a.K) {
            for (uint32_t j = j0; j < j1; ++j) {
                const double v = a.vT[(size_t)a.attr[j] * a.Kp + f];
                const float x = a.x[j];
                s += v * x;
                q2 -= 0.5 * v * v * x * x;
            }
#pragma unroll
            for (uint32_t r = 0; r < FG_MAX_REL; ++r)
                if (r < a.nrel) s += a.rel[r].qbf[(size_t)br[r] * a.K + f];
            e += 0.5 * s * s;
        }
        a.s[(size_t)q * a.Kp + f] = s;  // the padding columns: zero
    }
    e = fmq_wsum(e);
    q2 = fmq_wsum(q2);
    if (a.k1)
        for (uint32_t j = j0; j < j1; ++j) q2 += a.w[a.attr[j]] * a.x[j];
#pragma unroll
    for (uint32_t r = 0; r < FG_MAX_REL; ++r)
        if (r < a.nrel) q2 += a.rel[r].qs[br[r]];
    if (lane == 0) a.a[q] = e + q2;
}

__global__ __launch_bounds__(256) void k_fmq_operands(const double* __restrict__ qbf, const double4* __restrict__ rb,
                                                      uint32_t nb, uint32_t K, uint32_t Kp, double* __restrict__ B,
                                                      double* __restrict__ y) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)nb * Kp) return;
    const uint32_t j = (uint32_t)(i / Kp), f = (uint32_t)(i - (size_t)j * Kp);
    B[i] = f < K ? qbf[(size_t)j * K + f] : 0.0;
    if (f == 0) y[j] = rb[2 * (size_t)j].y;
}

hipError_t fmq_terms(const FMQTermsArgs& a, hipStream_t st) {
    if (a.nq == 0) return hipSuccess;
    k_fmq_terms<<<(a.nq + 3) / 4, 256, 0, st>>>(a);
    return hipGetLastError();
}

hipError_t fmq_operands(const double* qbf, const double4* rb, uint32_t nb, uint32_t K, uint32_t Kp, double* B,
                        double* y, hipStream_t st) {
    if (nb == 0) return hipSuccess;
    const size_t n = (size_t)nb * Kp;
    k_fmq_operands<<<(uint32_t)((n + 255) / 256), 256, 0, st>>>(qbf, rb, nb, K, Kp, B, y);
    return hipGetLastError();
}

}  // namespace sbmf
