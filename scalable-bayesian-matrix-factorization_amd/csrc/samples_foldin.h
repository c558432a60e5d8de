// samples_foldin.h -- host-callable launchers of the sample store's guest kernels in
// samples_foldin.hip: every guest's factor row drawn at every stored sample, after the run
// (include/sbmf.h, sbmf_samples_foldin_recommend).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "foldin.h"
#include "samples.h"

namespace sbmf {

// Most coordinate scans per sample (the scan's normals are pairs 128 scan + p of one Philox key).
constexpr uint32_t SAMPLES_FOLDIN_SCANS_MAX = 64;

// What both launchers read.  The guests are launch_foldin's CSR (ptr, items, ratings) and E its
// residual scratch, one double per rating.  A launch draws the n guests order[0..n) (the longest
// first), all of them in g0 <= g < g0 + n: guest g's normals are keyed by g, its row is row g - g0
// of a GS table.  sv: the store's view (only V, sv, head, cap and count
// are read).  For the s-th oldest sample: hyper + s 2 Kp is its [sg_u | mu_u] (zero padding),
// tau[s] its noise precision, sweeps[s] its absolute sweep index -- the Philox key of its normals,
// with the context's seed.  GS holds one table [n + 2][Kp] of T per ring slot (stride gs
// elements), the slot being the sample's in the store: the scoring kernel then reads GS through
// the store's own view, U replaced.  Rows n and n + 1 and the padding columns are the caller's
// to zero.
struct SamplesFoldinArgs {
    SampleView sv;
    uint32_t n = 0, g0 = 0;
    const uint32_t *order = nullptr, *ptr = nullptr, *items = nullptr;
    const double* ratings = nullptr;
    void* GS = nullptr;
    size_t gs = 0;
    uint32_t K = 0, Kp = 0;
    const double *hyper = nullptr, *tau = nullptr;
    const uint32_t* sweeps = nullptr;
    uint32_t scans = 1;
    int sd_is_var = 1;
    uint64_t seed = 0;
    double* E = nullptr;
};

// Every guest's row at every stored sample in one launch: per guest one workgroup carries the row
// in LDS from the oldest sample (entered with a zero row) to the newest, running `scans`
// launch_foldin scans per sample (scan r with normals 256 r + k of the sample's key; every scan
// recomputes the residuals from the row), rounding the row through T after a sample's last scan and
// writing it to the sample's GS table.  With scans = 1 and a store kept with every = 1 from the
// chain's first sweep, GS is what launch_foldin left in G after each of those sweeps, bit for bit.
template <typename T>
hipError_t launch_samples_foldin(const SamplesFoldinArgs& a, hipStream_t st);

// The unfused twin, and the form the store's calls use (the faster one on the device, DESIGN.md
// 4.8): the same scan of sample s (age), scan r alone.  The row travels between launches in `carry`
// [n][Kp] doubles (row g - g0; zeroed by the caller before the oldest sample's first scan):
// unrounded between a sample's scans, rounded through T after its last one, whose launch also
// writes GS.  The launches s = 0.., r = 0..scans-1 in order leave the fused launch's GS, bit for bit.
template <typename T>
hipError_t launch_samples_foldin_step(const SamplesFoldinArgs& a, uint32_t s, uint32_t r, double* carry, hipStream_t st);

}  // namespace sbmf
