// ptmi_hist.hip -- marginal posterior histograms of EVERY cold chain, accumulated on the device (ptmi_hist_attach / ptmi_hist_update,
// include/ptmi.h).  The AM ring (ptmi_buffers.AM, [W][cov_update][ndim]) holds the rank-0 row of every walker for every iteration of the
// current covariance period -- what the reference's updateChains stores (PTMCMCSampler.py:327-328): the post-swap row at swap iterations,
// the repeated row behind a rejection.  ptmi_update_cov streams it once per period for the covariance; this unit is a second reader that
// bins every element:
//
//     t = (x - lo[j]) * scale[j]              one subtraction, one multiplication (the build has -ffp-contract=off: no fma)
//     !(t >= 0)   -> under[j]  (x < lo, NaN)      t >= nbins -> over[j]  (x >= hi as scale rounds, +inf)      else counts[j][(int)t]
//
// into uint64 [ndim][nbins + 2] in PARAMETER order (columns 0 .. nbins - 1 the bins, nbins = under, nbins + 1 = over).  Counts are
// integers: any accumulation order gives the same result, and a NumPy restatement of the rule checks it to the last count.
//
// Two kernels per call, both on the handle's stream, nothing read back:
//
//   hist_weight_kernel   a 4-byte weight beside every ring row (the library's scratch): how many iterations of [iter_lo, iter_hi] the row
//                        stands for.  Without AM row flags 1 inside the range and 0 outside.  With them (am_mode "rle") a row without
//                        NEW / KEY repeats the last stored row before it (am_expand_kernel's rule): a stored row carries the length of
//                        its run clipped to the range, the stored row a run that is under way at iter_lo hangs on included, and a row
//                        that was not stored carries 0.  One block per walker (pool_rle_kernel's job, per walker and clipped).
//   hist_rows_kernel     one pass over the rows.  A block owns a tile of columns of the row format and walks slabs of 1024 ring rows: the
//                        slab's weights go to LDS, the threads take the slab's rows x columns in memory order (a wave instruction = 64
//                        consecutive doubles of a row, or the end of one and the start of the next: contiguous wherever the tile is the
//                        whole row), eight elements in flight per thread, rows of weight 0 are never requested (43 % of an rle ring).  The
//                        block's private histogram sits in LDS as u32 [bin][column] and takes the weights with LDS adds, which keep
//                        the counts right wherever two lanes meet in a word.  Word bin * tc + column: lanes of one bin hold neighbouring
//                        columns = neighbouring banks; lanes of different bins collide when tc (b1 - b2) + (c1 - c2) is a multiple of 64,
//                        so the tile is free of bank conflicts only where tc is a multiple of 64 (at tc = 100 it is not: a performance
//                        cost, the stride is not padded).  Columns are tiled so that weights, bounds
//                        and histogram fit 64 KB (14 columns per tile at nbins = 1024, the whole row of 100-d at nbins <= 155).  A block
//                        keeps its tile over all its slabs and adds it to the global uint64 buffer ONCE at its end, bins of a parameter
//                        to consecutive threads, zeros skipped: (nbins + 2) x columns vector atomics per block, none per element.  The
//                        row format (am_pos: the permuted rows of the exact 4-lane shape) is undone there and where the bounds are read:
//                        position p of a row is parameter am_inv(p).
//
// A u32 cell cannot overflow: the weights of a call sum to W x (iter_hi - iter_lo + 1) <= W x cov_update per column over ALL blocks, and
// the call refuses rings of 2^32 rows or more.
#include "ptmi_common.h"
#include "ptmi_ring_weight.h"      // hist_weight_kernel, ring_range, ring_weigh, ring_bounds

struct ptmi_hist_state {
    u64 *counts;               // caller-owned [ndim][nbins + 2]
    double *d_lo, *d_scale;    // [ndim] each, the library's copies
    u32 *d_wgt;                // [W][cov_update] weight of every ring row in the call under way (cold handles)
    int nbins;
};

namespace {

constexpr int RS = 1024;               // ring rows per slab
constexpr int UNR = 8;                 // elements in flight per thread
constexpr int LDS_BYTES = 65536;       // weights + bounds + histogram of a block
constexpr int TC_MAX = 512;            // columns per tile at most
constexpr int NBLOCKS = 1024;          // blocks of a launch, about (every block flushes its tile once)

struct HistArgs {
    const double *AM;
    const u32 *wgt;
    const double *lo, *scale;
    u64 *counts;
    long long nrows;           // W * cov_update
    int d, epl, nbins, tc, nslab;
};

__global__ __launch_bounds__(256) void hist_rows_kernel(const HistArgs a)
{
    extern __shared__ double hist_smem[];
    const int tid = (int)threadIdx.x, nb = a.nbins, nb2 = a.nbins + 2;
    const int c0 = (int)blockIdx.y * a.tc, tc = a.d - c0 < a.tc ? a.d - c0 : a.tc;
    double *los = hist_smem, *scs = hist_smem + a.tc;
    u32 *wl = reinterpret_cast<u32 *>(hist_smem + 2 * a.tc), *hist = wl + RS;
    for (int i = tid; i < tc; i += 256) {
        const int par = am_inv(c0 + i, a.epl);
        los[i] = a.lo[par];
        scs[i] = a.scale[par];
    }
    for (int i = tid; i < nb2 * tc; i += 256) hist[i] = 0u;
    const double top = (double)nb;
    const int dc = 256 / tc, dp = 256 % tc;
    for (int s = (int)blockIdx.x; s < a.nslab; s += (int)gridDim.x) {
        const long long r0 = (long long)s * RS;
        const int nr = (int)(a.nrows - r0 < RS ? a.nrows - r0 : RS);
        __syncthreads();                                       // the slab before is done with wl (first trip: los / scs / hist are set)
        for (int i = tid; i < nr; i += 256) wl[i] = a.wgt[r0 + i];
        __syncthreads();
        const double *src = a.AM + (size_t)r0 * a.d + c0;
        const int total = nr * tc;
        // element p = tid + 256 j of the slab's tile: row p / tc, column p % tc -- kept current by increments
        int rl = tid / tc, c = tid % tc;
        for (int p0 = tid; p0 < total; p0 += 256 * UNR) {
            double v[UNR];
            u32 wt[UNR];
            int cc[UNR];
#pragma unroll
            for (int j = 0; j < UNR; ++j) {
                wt[j] = 0u; cc[j] = c; v[j] = 0.0;
                if (p0 + 256 * j < total) {
                    wt[j] = wl[rl];
                    if (wt[j]) v[j] = src[(size_t)rl * a.d + c];
                }
                rl += dc; c += dp;
                if (c >= tc) { c -= tc; rl += 1; }
            }
#pragma unroll
            for (int j = 0; j < UNR; ++j) {
                if (!wt[j]) continue;
                const double t = (v[j] - los[cc[j]]) * scs[cc[j]];
                const int b = !(t >= 0.0) ? nb : (t >= top ? nb + 1 : (int)t);
                atomicAdd(&hist[b * tc + cc[j]], wt[j]);
            }
        }
    }
    __syncthreads();
    // the tile into the caller's buffer: thread i takes bin i % (nbins + 2) of column i / (nbins + 2)
    for (int i = tid; i < nb2 * tc; i += 256) {
        const int col = i / nb2, b = i - col * nb2;
        const u32 n = hist[b * tc + col];
        if (n) atomicAdd(a.counts + (size_t)am_inv(c0 + col, a.epl) * nb2 + b, (u64)n);
    }
}

}  // namespace

void ptmi_hist_free(ptmi_engine *h)
{
    ptmi_hist_state *s = h->hist;
    if (!s) return;
    (void)hipFree(s->d_lo); (void)hipFree(s->d_scale); (void)hipFree(s->d_wgt);
    delete s;
    h->hist = nullptr;
}

extern "C" {

int ptmi_hist_attach(ptmi_handle h, uint64_t *counts, const double *lo, const double *scale, int32_t nbins)
{
    if (!h || !lo || !scale) return fail(PTMI_EINVAL, "NULL argument");
    if (h->hist) return fail(PTMI_EINVAL, "ptmi_hist_attach: already attached");
    if (nbins < 2 || nbins > 1024) return fail(PTMI_EINVAL, "ptmi_hist_attach: 2 <= nbins <= 1024 (got %d)", (int)nbins);
    if (!counts || ((uintptr_t)counts & 7) != 0) return fail(PTMI_EINVAL, "ptmi_hist_attach: counts must be non-NULL and 8-byte aligned");
    const ptmi_config &c = h->cfg;
    if (int r = ring_bounds("ptmi_hist_attach", c.ndim, lo, scale)) return r;
    ptmi_hist_state *s = new ptmi_hist_state();
    s->counts = (u64 *)counts;
    s->nbins = (int)nbins;
    h->hist = s;
    const size_t bytes = sizeof(double) * (size_t)c.ndim;
    hipError_t e = hipMalloc((void **)&s->d_lo, bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_scale, bytes);
    if (e == hipSuccess && c.temp0 == 0) e = hipMalloc((void **)&s->d_wgt, sizeof(u32) * (size_t)c.nwalkers * c.cov_update);
    if (e == hipSuccess) e = hipMemcpy(s->d_lo, lo, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_scale, scale, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        ptmi_hist_free(h);
        return fail(PTMI_EHIP, "ptmi_hist_attach: %s", hipGetErrorString(e));
    }
    return PTMI_OK;
}

int ptmi_hist_update(ptmi_handle h, int64_t iter_lo, int64_t iter_hi)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    const ptmi_hist_state *s = h->hist;
    if (!s) return fail(PTMI_EINVAL, "ptmi_hist_update: no histogram is attached (ptmi_hist_attach)");
    const ptmi_config &c = h->cfg;
    long long base;
    if (int r = ring_range(h, "ptmi_hist_update", iter_lo, iter_hi, &base)) return r == RING_IDLE ? PTMI_OK : r;
    if (int r = ring_weigh(h, "ptmi_hist_update", s->d_wgt, base, iter_lo, iter_hi)) return r;
    const long long nrows = (long long)c.nwalkers * c.cov_update;
    HistArgs a;
    a.AM = h->buf.AM; a.wgt = s->d_wgt; a.lo = s->d_lo; a.scale = s->d_scale; a.counts = s->counts;
    a.nrows = nrows; a.d = c.ndim; a.epl = am_row_epl(h->G, h->EPL); a.nbins = s->nbins;
    // columns per tile: 4 (nbins + 2) bytes of histogram and 16 of bounds each, beside the slab's weights
    int tcmax = (LDS_BYTES - 4 * RS) / (4 * (s->nbins + 2) + 16);
    if (tcmax > TC_MAX) tcmax = TC_MAX;
    const int ntile = (c.ndim + tcmax - 1) / tcmax;
    a.tc = (c.ndim + ntile - 1) / ntile;
    a.nslab = (int)((nrows + RS - 1) / RS);
    int gx = NBLOCKS / ntile;
    if (gx < 1) gx = 1;
    if (gx > a.nslab) gx = a.nslab;
    const size_t lds = (size_t)16 * a.tc + 4 * RS + (size_t)4 * (s->nbins + 2) * a.tc;
    hipLaunchKernelGGL(hist_rows_kernel, dim3((unsigned)gx, (unsigned)((c.ndim + a.tc - 1) / a.tc)), dim3(256), lds, h->stream, a);
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

}  // extern "C"
