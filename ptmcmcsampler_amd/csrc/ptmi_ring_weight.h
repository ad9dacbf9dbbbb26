// ptmi_ring_weight.h -- the weight of every AM ring row in a range of iterations, for the units that read the ring a second time
// (ptmi_hist.hip, ptmi_pairs.hip).  Every includer gets its own copy of the kernel.
#pragma once
#include "ptmi_common.h"

namespace {

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

}  // namespace
