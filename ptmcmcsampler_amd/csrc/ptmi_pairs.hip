// ptmi_pairs.hip -- joint posterior histograms of parameter PAIRS of EVERY cold chain, accumulated on the device (ptmi_pairs_attach /
// ptmi_pairs_update, include/ptmi.h): the off-diagonal panels of a corner plot.  A second reader of the AM ring beside ptmi_hist.hip,
// with its rule per axis:
//
//     t = (x - lo[k]) * scale[k]              one subtraction, one multiplication (the build has -ffp-contract=off: no fma)
//     inside(t) = t >= 0 and not t >= nbins   (NaN, x < lo, x >= hi as scale rounds, +-inf: outside)
//     pair (i, j):  both inside -> counts[p][(int)ti * nbins + (int)tj]      else -> counts[p][nbins * nbins], the pair's "outside" cell
//
// into uint64 [npairs][nbins * nbins + 1].  Counts are integers: any accumulation order gives the same result, and a NumPy
// restatement of the rule (ptmcmcsampler_amd/pairs.py pairs_rule) checks it to the last count.
//
// Two kernels per call, both on the handle's stream, nothing read back:
//
//   hist_weight_kernel   ptmi_hist.hip's (ptmi_ring_weight.h): how many iterations of [iter_lo, iter_hi] every ring row stands for.
//   pairs_rows_kernel    one pass over the rows per TILE of pairs.  ptmi_pairs_attach cuts the pair list, in its order, into tiles whose
//                        private tables fit the block's LDS as u32 cells (4 (nbins^2 + 1) bytes a pair: two pairs at nbins = 128, 37 at
//                        32, thousands at 2) and lists the DISTINCT columns each tile needs, sorted by their position in a ring row
//                        (am_pos: the permuted rows of the exact 4-lane shape are undone here, once, on the host).  A block owns a tile
//                        (blockIdx.x: the blocks that walk the same slabs are neighbours in dispatch order and meet in the caches) and
//                        walks slabs of 1024 ring rows (blockIdx.y).  Per slab:
//                          1. the slab's weights go to LDS;
//                          2. the threads take the slab's rows x the tile's columns in memory order along the row, eight elements in
//                             flight per thread, rows of weight 0 never requested, and write one byte per (row, column) into LDS: the
//                             bin, or 255 for "outside" -- a float is compared once however many pairs share its column, and HBM sees
//                             the needed columns only;
//                          3. the (row, pair) work items, pair fastest (the lanes of a wave spread over the tile's tables: a peaked
//                             posterior does not pile them on one word), combine two bytes and add the row's weight to the pair's
//                             cell with one LDS add.
//                        The block keeps its tile over all its slabs and adds it to the global uint64 buffer ONCE at its end, cells of
//                        a pair to consecutive threads, zeros skipped: no global atomics per element.
//
// LDS budget: the whole 160 KB of a CU for ONE block of 512 threads (the dynamic size attribute beyond 64 KB).  One pair at nbins = 128
// needs 64 KB + 4 B of cells, so 64 KB cannot hold it beside the slab's weights.  Every tile is one more pass over the ring, and the
// ring's bytes are what the kernel waits for: 45 pairs at 32 bins are three tiles at 80 KB (two blocks of 256 threads a CU; measured
// first: 837 us at the headline ring) and two at 160 KB.  The block has 512 threads so that the CU keeps its 8 waves.  The
// launch has about 256 blocks: one a CU, one wave of blocks.
//
// A u32 cell cannot overflow: the weights of a call sum to W x (iter_hi - iter_lo + 1) <= W x cov_update per pair over ALL blocks, and
// the call refuses rings of 2^32 rows or more.
#include "ptmi_common.h"
#include "ptmi_ring_weight.h"      // hist_weight_kernel, ring_range, ring_weigh, ring_bounds
#include <algorithm>
#include <vector>

namespace {

constexpr int RS = 1024;               // ring rows per slab
constexpr int UNR = 8;                 // elements in flight per thread
constexpr int NT = 512;                // threads of a block of pairs_rows_kernel: 8 waves, the CU's share with one block a CU
constexpr int LDS_BYTES = 163840;      // bounds + weights + lists + tables + bin bytes of a block: the whole LDS of a CU
constexpr int NBLOCKS = 256;           // blocks of a launch, about: one a CU (every block flushes its tile once)
constexpr int NPAIRS_MAX = 8192, NBINS_MAX = 128;

struct PairTile { int pair0, np, col0, nc; };      // pairs pair0 .. pair0 + np - 1; columns col0 .. col0 + nc - 1 of the column lists

// LDS of a tile: lo / scale / ring position of every column, the slab's weights, slot pair and table of every pair, bin bytes
inline size_t tile_lds(int np, int nc, int nbins) { return (size_t)20 * nc + 4 * RS + (size_t)4 * np * (nbins * nbins + 2) + (size_t)RS * nc; }

struct PairsArgs {
    const double *AM;
    const u32 *wgt;
    const PairTile *tile;
    const int *cpos;                   // ring-row position of every listed column
    const double *clo, *csc;           // its lo and scale
    const u32 *pslot;                  // per pair: slot of i | slot of j << 16, slots counting the tile's columns
    u64 *counts;
    long long nrows;                   // W * cov_update
    int d, nbins, nslab;
};

__global__ __launch_bounds__(NT) void pairs_rows_kernel(const PairsArgs a)
{
    extern __shared__ double pairs_smem[];
    const PairTile t = a.tile[blockIdx.x];
    const int tid = (int)threadIdx.x, nb = a.nbins, cells = nb * nb + 1, np = t.np, nc = t.nc;
    double *los = pairs_smem, *scs = pairs_smem + nc;
    u32 *wl = reinterpret_cast<u32 *>(pairs_smem + 2 * nc);
    int *cp = reinterpret_cast<int *>(wl + RS);
    u32 *ps = reinterpret_cast<u32 *>(cp + nc), *hist = ps + np;
    unsigned char *binl = reinterpret_cast<unsigned char *>(hist + (size_t)np * cells);      // [row of the slab][column of the tile]
    for (int i = tid; i < nc; i += NT) {
        los[i] = a.clo[t.col0 + i];
        scs[i] = a.csc[t.col0 + i];
        cp[i] = a.cpos[t.col0 + i];
    }
    for (int i = tid; i < np; i += NT) ps[i] = a.pslot[t.pair0 + i];
    for (int i = tid; i < np * cells; i += NT) hist[i] = 0u;
    const double top = (double)nb;
    const int dc = NT / nc, dp = NT % nc, ec = NT / np, ep = NT % np;
    for (int s = (int)blockIdx.y; s < a.nslab; s += (int)gridDim.y) {
        const long long r0 = (long long)s * RS;
        const int nr = (int)(a.nrows - r0 < RS ? a.nrows - r0 : RS);
        __syncthreads();                                       // the slab before is done with wl / binl (first trip: the lists and tables are set)
        for (int i = tid; i < nr; i += NT) wl[i] = a.wgt[r0 + i];
        __syncthreads();
        const double *src = a.AM + (size_t)r0 * a.d;
        // element p = tid + NT j of the slab: row p / nc, column slot p % nc -- kept current by increments; its byte is binl[p]
        const int total = nr * nc;
        int rl = tid / nc, c = tid % nc;
        for (int p0 = tid; p0 < total; p0 += NT * UNR) {
            double v[UNR];
            int cc[UNR];                                       // the element's column slot, -1: not requested
#pragma unroll
            for (int j = 0; j < UNR; ++j) {
                cc[j] = -1; v[j] = 0.0;
                if (p0 + NT * j < total && wl[rl] != 0u) {
                    cc[j] = c;
                    v[j] = src[(size_t)rl * a.d + cp[c]];
                }
                rl += dc; c += dp;
                if (c >= nc) { c -= nc; rl += 1; }
            }
#pragma unroll
            for (int j = 0; j < UNR; ++j) {
                if (cc[j] < 0) continue;
                const double x = (v[j] - los[cc[j]]) * scs[cc[j]];
                binl[p0 + NT * j] = (x >= 0.0 && !(x >= top)) ? (unsigned char)(int)x : (unsigned char)255;
            }
        }
        __syncthreads();
        // work item q = tid + NT j: row q / np, pair q % np
        const int items = nr * np;
        int r = tid / np, p = tid % np;
        for (int q = tid; q < items; q += NT) {
            const u32 wt = wl[r];
            if (wt) {
                const u32 sl = ps[p];
                const u32 bi = binl[r * nc + (int)(sl & 0xffffu)], bj = binl[r * nc + (int)(sl >> 16)];
                const int cell = ((bi | bj) & 0x80u) ? nb * nb : (int)(bi * (u32)nb + bj);      // bins are below 128: bit 7 says "outside"
                atomicAdd(&hist[p * cells + cell], wt);
            }
            r += ec; p += ep;
            if (p >= np) { p -= np; r += 1; }
        }
    }
    __syncthreads();
    // the tile into the caller's buffer: its pairs are neighbours there as they are here
    u64 *dst = a.counts + (size_t)t.pair0 * cells;
    for (int i = tid; i < np * cells; i += NT) {
        const u32 n = hist[i];
        if (n) atomicAdd(dst + i, (u64)n);
    }
}

}  // namespace

struct ptmi_pairs_state {
    u64 *counts;               // caller-owned [npairs][nbins * nbins + 1]
    PairTile *d_tile;          // [ntile]
    int *d_cpos;               // [ncol]: the tiles' column lists, one behind the other
    double *d_clo, *d_csc;     // [ncol]
    u32 *d_pslot;              // [npairs]
    u32 *d_wgt;                // [W][cov_update] weight of every ring row in the call under way (cold handles)
    int nbins, npairs, ntile;
    size_t lds;                // of the largest tile
};

void ptmi_pairs_free(ptmi_engine *h)
{
    ptmi_pairs_state *s = h->pairs;
    if (!s) return;
    (void)hipFree(s->d_tile); (void)hipFree(s->d_cpos); (void)hipFree(s->d_clo); (void)hipFree(s->d_csc); (void)hipFree(s->d_pslot);
    (void)hipFree(s->d_wgt);
    delete s;
    h->pairs = nullptr;
}

extern "C" {

int ptmi_pairs_attach(ptmi_handle h, uint64_t *counts, const int32_t *pairs, int32_t npairs, const double *lo, const double *scale,
                      int32_t nbins)
{
    if (!h || !pairs || !lo || !scale) return fail(PTMI_EINVAL, "NULL argument");
    if (h->pairs) return fail(PTMI_EINVAL, "ptmi_pairs_attach: already attached");
    if (nbins < 2 || nbins > NBINS_MAX) return fail(PTMI_EINVAL, "ptmi_pairs_attach: 2 <= nbins <= %d (got %d)", NBINS_MAX, (int)nbins);
    if (npairs < 1 || npairs > NPAIRS_MAX) return fail(PTMI_EINVAL, "ptmi_pairs_attach: 1 <= npairs <= %d (got %d)", NPAIRS_MAX, (int)npairs);
    if (!counts || ((uintptr_t)counts & 7) != 0) return fail(PTMI_EINVAL, "ptmi_pairs_attach: counts must be non-NULL and 8-byte aligned");
    const ptmi_config &c = h->cfg;
    for (int p = 0; p < npairs; ++p) {
        const int i = pairs[2 * p], j = pairs[2 * p + 1];
        if (i < 0 || i >= c.ndim || j < 0 || j >= c.ndim || i == j)
            return fail(PTMI_EINVAL, "ptmi_pairs_attach: pair %d: two different parameters in 0 .. %d (got %d, %d)", p, c.ndim - 1, i, j);
    }
    if (int r = ring_bounds("ptmi_pairs_attach", c.ndim, lo, scale)) return r;
    // the tiles: the pair list in its order, a tile closed where the next pair (with the columns it adds) no longer fits
    const int epl = am_row_epl(h->G, h->EPL);
    std::vector<PairTile> tiles;
    std::vector<int> cpos, slot(c.ndim, -1), cols;
    std::vector<double> clo, csc;
    std::vector<u32> pslot((size_t)npairs);
    size_t lds = 0;
    auto close = [&](int pair0, int pend) {
        std::sort(cols.begin(), cols.end(), [&](int x, int y) { return am_pos(x, epl) < am_pos(y, epl); });
        for (size_t k = 0; k < cols.size(); ++k) slot[cols[k]] = (int)k;
        for (int p = pair0; p < pend; ++p) pslot[p] = (u32)slot[pairs[2 * p]] | ((u32)slot[pairs[2 * p + 1]] << 16);
        tiles.push_back(PairTile{pair0, pend - pair0, (int)cpos.size(), (int)cols.size()});
        lds = std::max(lds, tile_lds(pend - pair0, (int)cols.size(), nbins));
        for (int k : cols) {
            cpos.push_back(am_pos(k, epl)); clo.push_back(lo[k]); csc.push_back(scale[k]);
            slot[k] = -1;
        }
        cols.clear();
    };
    int pair0 = 0;
    for (int p = 0; p < npairs; ++p) {
        const int i = pairs[2 * p], j = pairs[2 * p + 1];
        const int add = (slot[i] < 0) + (slot[j] < 0);
        if (p > pair0 && tile_lds(p - pair0 + 1, (int)cols.size() + add, nbins) > (size_t)LDS_BYTES) {
            close(pair0, p);
            pair0 = p;
        }
        if (slot[i] < 0) { slot[i] = 0; cols.push_back(i); }
        if (slot[j] < 0) { slot[j] = 0; cols.push_back(j); }
    }
    close(pair0, npairs);
    if (lds > (size_t)LDS_BYTES) return fail(PTMI_EINVAL, "ptmi_pairs_attach: a tile of %zu bytes", lds);      // (one pair at nbins = 128: 71 728)
    ptmi_pairs_state *s = new ptmi_pairs_state();
    s->counts = (u64 *)counts;
    s->nbins = (int)nbins; s->npairs = (int)npairs; s->ntile = (int)tiles.size(); s->lds = lds;
    h->pairs = s;
    const size_t ncol = cpos.size();
    hipError_t e = hipMalloc((void **)&s->d_tile, sizeof(PairTile) * tiles.size());
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_cpos, sizeof(int) * ncol);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_clo, sizeof(double) * ncol);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_csc, sizeof(double) * ncol);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_pslot, sizeof(u32) * (size_t)npairs);
    if (e == hipSuccess && c.temp0 == 0) e = hipMalloc((void **)&s->d_wgt, sizeof(u32) * (size_t)c.nwalkers * c.cov_update);
    if (e == hipSuccess) e = hipMemcpy(s->d_tile, tiles.data(), sizeof(PairTile) * tiles.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_cpos, cpos.data(), sizeof(int) * ncol, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_clo, clo.data(), sizeof(double) * ncol, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_csc, csc.data(), sizeof(double) * ncol, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_pslot, pslot.data(), sizeof(u32) * (size_t)npairs, hipMemcpyHostToDevice);
    // a block's LDS beyond 64 KB has to be asked for
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)pairs_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    if (e != hipSuccess) {
        ptmi_pairs_free(h);
        return fail(PTMI_EHIP, "ptmi_pairs_attach: %s", hipGetErrorString(e));
    }
    return PTMI_OK;
}

int ptmi_pairs_update(ptmi_handle h, int64_t iter_lo, int64_t iter_hi)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    const ptmi_pairs_state *s = h->pairs;
    if (!s) return fail(PTMI_EINVAL, "ptmi_pairs_update: no pair histogram is attached (ptmi_pairs_attach)");
    const ptmi_config &c = h->cfg;
    long long base;
    if (int r = ring_range(h, "ptmi_pairs_update", iter_lo, iter_hi, &base)) return r == RING_IDLE ? PTMI_OK : r;
    if (int r = ring_weigh(h, "ptmi_pairs_update", s->d_wgt, base, iter_lo, iter_hi)) return r;
    const long long nrows = (long long)c.nwalkers * c.cov_update;
    PairsArgs a;
    a.AM = h->buf.AM; a.wgt = s->d_wgt; a.tile = s->d_tile; a.cpos = s->d_cpos; a.clo = s->d_clo; a.csc = s->d_csc; a.pslot = s->d_pslot;
    a.counts = s->counts; a.nrows = nrows; a.d = c.ndim; a.nbins = s->nbins;
    a.nslab = (int)((nrows + RS - 1) / RS);
    int gy = NBLOCKS / s->ntile;
    if (gy < 1) gy = 1;
    if (gy > a.nslab) gy = a.nslab;
    hipLaunchKernelGGL(pairs_rows_kernel, dim3((unsigned)s->ntile, (unsigned)gy), dim3(NT), s->lds, h->stream, a);
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

}  // extern "C"
