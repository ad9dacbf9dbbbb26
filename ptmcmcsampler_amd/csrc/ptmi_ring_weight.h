// ptmi_ring_weight.h -- what the units that read the AM ring a second time share (ptmi_hist.hip, ptmi_pairs.hip, ptmi_diag.hip,
// ptmi_samples.hip, ptmi_best.hip): the checks their *_update / *_take calls open with and, for the two that count, the weight of every
// ring row in a range of iterations and the check of the bin bounds.  Every includer gets its own copy; PTMI_RING_RANGE_ONLY
// (ptmi_diag.hip, ptmi_samples.hip, ptmi_best.hip) leaves out what only the counting units use.
#pragma once
#include "ptmi_common.h"
#include <math.h>

namespace {

// What the update call `fn` of a ring reader checks once it has its state: PTMI_OK and *base, the iteration the ring's period starts
// behind; RING_IDLE where there is nothing to do; else the refusal.
constexpr int RING_IDLE = 1;
inline int ring_range(const ptmi_engine *h, const char *fn, int64_t iter_lo, int64_t iter_hi, long long *base)
{
    const ptmi_config &c = h->cfg;
    if (c.temp0 != 0) return RING_IDLE;                 // only the GPU holding rank 0 has the cold chains (as ptmi_update_cov)
    if (iter_hi < iter_lo) return RING_IDLE;
    const long long cu = c.cov_update;
    *base = iter_hi > 0 ? ((long long)(iter_hi - 1) / cu) * cu : 0;
    if (iter_lo <= *base || iter_hi < 1)
        return fail(PTMI_EINVAL, "%s: iterations %lld..%lld cross a covariance period: the ring holds (%lld, %lld], the period of the last one", fn,
                    (long long)iter_lo, (long long)iter_hi, *base, *base + cu);
    if (!h->buf.AM) return fail(PTMI_EINVAL, "%s: the handle has no AM buffer", fn);
    return PTMI_OK;
}

#ifndef PTMI_RING_RANGE_ONLY
// iteration base + k, k in 1 .. cu, sits in ring row k % cu
__device__ __forceinline__ bool stored_at(const AmFlag *fw, int k, int cu) { return (fw[k == cu ? 0 : k] & (AMROW_NEW | AMROW_KEY)) != 0; }

__global__ __launch_bounds__(256) void hist_weight_kernel(const AmFlag *flag, u32 *wgt, int cu, int klo, int khi)
{
    const size_t w = blockIdx.x;
    const AmFlag *fw = flag ? flag + w * cu : nullptr;
    u32 *ww = wgt + w * cu;
    for (int r = (int)threadIdx.x; r < cu; r += 256) ww[r] = 0u;
    __syncthreads();
    for (int k = klo + (int)threadIdx.x; k <= khi; k += 256) {
        int s = k;                                             // the stored row iteration k is counted with
        if (fw && !stored_at(fw, k, cu)) {
            if (k != klo) continue;                            // counted with its run's stored row
            while (s > 1 && !stored_at(fw, s, cu)) --s;        // (ring row 1 of a period is a KEY row)
        }
        int n = k + 1;
        if (fw) while (n <= khi && !stored_at(fw, n, cu)) ++n;
        ww[s == cu ? 0 : s] = (u32)(n - k);
    }
}

// The weights of iterations iter_lo .. iter_hi of the period behind `base` into wgt [W][cov_update], on the handle's stream.
inline int ring_weigh(const ptmi_engine *h, const char *fn, u32 *wgt, long long base, int64_t iter_lo, int64_t iter_hi)
{
    const ptmi_config &c = h->cfg;
    const long long nrows = (long long)c.nwalkers * c.cov_update;
    if (nrows >= (1ll << 32)) return fail(PTMI_EUNSUPPORTED, "%s: a ring of %lld rows (32-bit counts per block: below 2^32)", fn, nrows);
    hipLaunchKernelGGL(hist_weight_kernel, dim3((unsigned)c.nwalkers), dim3(256), 0, h->stream, (const AmFlag *)h->buf.AMflag, wgt, (int)c.cov_update,
                       (int)(iter_lo - base), (int)(iter_hi - base));
    return PTMI_OK;
}

// lo / scale [ndim] of the attach call `fn` of a reader that counts in bins
inline int ring_bounds(const char *fn, int ndim, const double *lo, const double *scale)
{
    for (int j = 0; j < ndim; ++j)
        if (!isfinite(lo[j]) || !isfinite(scale[j]) || !(scale[j] > 0.0))
            return fail(PTMI_EINVAL, "%s: parameter %d: lo must be finite and scale = nbins / (hi - lo) finite and positive (got %g, %g)", fn, j,
                        lo[j], scale[j]);
    return PTMI_OK;
}
#endif

}  // namespace
