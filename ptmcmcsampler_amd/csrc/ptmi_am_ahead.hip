// ptmi_am_ahead.hip -- the AM increments of libptmi.so computed on the matrix cores ahead of a launch: the kernels that list a
// piece's AM picks and multiply them, their scratch, ptmi_am_prepare for ptmi_mh_steps and the split path's entry points.  They
// reach the engine through the handle's fields only (ptmi_common.h).
#include <math.h>
#include <stdlib.h>

#include "ptmi_common.h"

typedef double ps_d4 __attribute__((ext_vector_type(4)));       // a matrix tile's accumulators (am_gemm_kernel; ptmi_cov.hip has its own)

// ------------------------------------------------- AM increments ahead of the launch (large ndim)
// The AM proposal q = x + U (cd sqrt(S) z) (PT:879-933) costs 2 ndim^2 flops per pick, and its increment depends on the chain's
// stream, the iteration and the scale branch only -- not on its state.  For the 16- and 64-lane shapes (ndim > 104), where a
// chain is a quarter of a wave or a whole one and the kernel's own product ran on the vector pipe (1.2 s per 100 steps of the
// default mix at ndim = 1000), the increments of a piece of the launch are computed AHEAD of it as one matrix product on the
// matrix cores: the piece's AM picks are listed (am_count / am_scan / am_fill: one thread per chain repeats the kernel's cycle
// draw), am_gemm_kernel computes INC[event][:] = sum_k Ut[k][:] w_event[k] -- 64 events per block, every weight generated in the
// block from the event's stream, v_mfma_f64_16x16x4 accumulating k ascending: the oracle's fma chain -- and the step kernel
// reads its increment instead of computing it.
struct AmEvent { long long it; double cd; u32 sid, pad /* the pick's parameter group */; };
struct AmArgs {
    u64 seed;
    long long iter0, nch;
    int nsteps, nt, ntg, temp0, walker0, w_host, w_scam, w_am, w_de, pick_walker;
    int w_gj;                          // NUTS + HMC entries behind the others in the cycle (propose() with GJ)
    int ngroups;                       // parameter groups (PT:129-145): > 1: the pick's group is drawn as propose() draws it
    int per_walker;                    // per-walker covariances: an event's table is its walker's (key = walker * ngroups + group), else key = group
    const double *gcn;                 // [ngroups] 2.4 / sqrt(2 size of the group) (PT:928)
    const int32_t *temp_of;
    const double *temps_mh;
};
// the cycle draw of propose() (ptmi_mh.inc.h) for one (chain, iteration); cd = 2.4 / sqrt(2 ndim) * scale (PT:846-862, 928)
__device__ __forceinline__ bool am_pick(const AmArgs &p, long long ch, long long it, AmEvent &e)
{
    const int w = (int)(ch / p.nt), t = p.temp_of[ch];
    const u32 sid0 = (u32)((u64)(p.walker0 + w) * (u32)p.ntg), sid = sid0 + (u32)(p.temp0 + t);
    u64 p0, p1;
    philox_words(p.seed, (u64)it, sid, 0u, p0, p1);
    u32 pickw = (u32)(p0 >> 32);
    if (p.pick_walker) {
        u64 q0, q1;
        philox_words(p.seed, (u64)it, sid0, 0u, q0, q1);
        pickw = (u32)(q0 >> 32);
    }
    const int L = p.w_host + p.w_scam + p.w_am + p.w_de + p.w_gj;
    const int ind = (int)__umulhi(pickw, (u32)L) - p.w_host;
    if (ind < p.w_scam || ind >= p.w_scam + p.w_am) return false;
    constexpr u32 T97 = (u32)(0.97 * 4294967296.0), T90 = (u32)(0.9 * 4294967296.0);
    const u32 plo = (u32)p0;
    const double temp = p.temps_mh[t];
    const bool warm = temp <= 100.0;
    const double sT = warm ? det_sqrt(temp) : 1.0;
    const double base = plo > T97 ? 10.0 : (plo > T90 ? 0.2 : 1.0);
    u32 g = 0;
    if (p.ngroups > 1) {               // propose()'s group draw (PT:897): its own Philox call
        u64 g0, g1;
        philox_words(p.seed, (u64)it, sid, 2u, g0, g1);
        g = __umulhi((u32)(g0 >> 32), (u32)p.ngroups);
    }
    e.it = it; e.sid = sid; e.pad = g;
    e.cd = p.gcn[g] * (warm ? base * sT : base);
    return true;
}
// (gtot: with parameter groups the picks per group, [ngroups] zeroed by the caller: the block's histogram first)
constexpr int AM_MAXG = 1024;         // = the ABI's limit on ngroups
__global__ __launch_bounds__(256) void am_count_kernel(const AmArgs p, int32_t *count, int32_t *gtot)
{
    __shared__ int32_t lh[AM_MAXG];
    const bool hist = gtot && !p.per_walker;                             // (per walker: thousands of keys, a handful of picks each: straight to memory)
    if (hist)
        for (int g = (int)threadIdx.x; g < p.ngroups; g += 256) lh[g] = 0;
    if (hist) __syncthreads();
    const long long ch = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ch < p.nch) {
        int n = 0;
        AmEvent e;
        const long long kw = p.per_walker ? (ch / p.nt) * p.ngroups : 0;
        for (int s = 0; s < p.nsteps; ++s)
            if (am_pick(p, ch, p.iter0 + s, e)) {
                n += 1;
                if (hist) atomicAdd(&lh[e.pad], 1);
                else if (gtot) atomicAdd(&gtot[kw + e.pad], 1);
            }
        count[ch] = n;
    }
    if (hist) {
        __syncthreads();
        for (int g = (int)threadIdx.x; g < p.ngroups; g += 256)
            if (lh[g]) atomicAdd(&gtot[g], lh[g]);
    }
}
// exclusive prefix sums of the chains' counts, base[nch] = the number of events; two launches of 1024-chain blocks: the blocks' sums, then
// every block adds up the sums before it and scans its own counts (one block over all chains took 0.44 ms at 262 144 chains: its
// threads walked the counts 256 apart)
__device__ __forceinline__ int am_block_scan(int v, int &total, int *wsum /* [16] */)
{
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < 16; ++w) { const int t = wsum[w]; all += t; if (w < wave) before += t; }
    total = all;
    return before + inc - v;                                             // exclusive
}
__global__ __launch_bounds__(1024) void am_scan_sums_kernel(const int32_t *count, int32_t *part, long long nch)
{
    __shared__ int wsum[16];
    const long long i = (long long)blockIdx.x * 1024 + threadIdx.x;
    int total;
    (void)am_block_scan(i < nch ? count[i] : 0, total, wsum);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}
__global__ __launch_bounds__(1024) void am_scan_kernel(const int32_t *count, const int32_t *part, long long *base, long long nch)
{
    __shared__ int wsum[16];
    __shared__ long long off_s;
    __shared__ long long red[16];
    long long off = 0;
    for (int j = (int)threadIdx.x; j < (int)blockIdx.x; j += 1024) off += part[j];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) off += __shfl_down(off, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = off;
    __syncthreads();
    if (threadIdx.x == 0) { long long t = 0; for (int w = 0; w < 16; ++w) t += red[w]; off_s = t; }
    __syncthreads();
    const long long i = (long long)blockIdx.x * 1024 + threadIdx.x;
    int total;
    const int ex = am_block_scan(i < nch ? count[i] : 0, total, wsum);
    if (i < nch) base[i] = off_s + ex;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) base[nch] = off_s + total;
}
// The events in chain order (the step kernel walks its chain's increments in step order); with parameter groups also perm: the
// events' indices listed group by group (group g: perm[gbase[g] ...), in no particular order inside a group -- an event's increment
// does not depend on its neighbours), so that a block of am_gemm_kernel holds 64 events of ONE group and multiplies by that group's
// rows only.  A block reserves its share of every group's list with one atomic per group.
__global__ __launch_bounds__(256) void am_fill_kernel(const AmArgs p, const long long *base, AmEvent *ev, const long long *gbase, int32_t *cursor, int32_t *perm)
{
    __shared__ int32_t lh[AM_MAXG];
    __shared__ long long lb[AM_MAXG];
    const long long ch = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    AmEvent e;
    const bool hist = perm && !p.per_walker;
    if (hist) {
        for (int g = (int)threadIdx.x; g < p.ngroups; g += 256) lh[g] = 0;
        __syncthreads();
        if (ch < p.nch)
            for (int s = 0; s < p.nsteps; ++s)
                if (am_pick(p, ch, p.iter0 + s, e)) atomicAdd(&lh[e.pad], 1);
        __syncthreads();
        for (int g = (int)threadIdx.x; g < p.ngroups; g += 256) {
            lb[g] = lh[g] ? gbase[g] + atomicAdd(&cursor[g], lh[g]) : 0;
            lh[g] = 0;
        }
        __syncthreads();
    }
    if (ch >= p.nch) return;
    long long at = base[ch];
    const long long kw = p.per_walker ? (ch / p.nt) * p.ngroups : 0;
    for (int s = 0; s < p.nsteps; ++s)
        if (am_pick(p, ch, p.iter0 + s, e)) {
            if (hist) perm[lb[e.pad] + atomicAdd(&lh[e.pad], 1)] = (int32_t)at;
            else if (perm) perm[gbase[kw + e.pad] + atomicAdd(&cursor[kw + e.pad], 1)] = (int32_t)at;      // per walker: the key's own cursor
            ev[at++] = e;
        }
}
// 64 events per block of four waves; wave v holds the output tiles v, v + 4, ... (16 rows of the increment each) of all four event
// tiles: at most 8 x 4 tiles of 8 registers = the 256 accumulation registers, i.e. 512 rows of the increment per block.  Beyond
// (ndim <= 1024) two blocks (blockIdx.y) share an event tile, each with half of the output rows and its own copy of the weights.
// The weights of 2 G consecutive directions -- G Box-Muller pairs (k, k + G) per event, the pairing of the step kernels -- are
// generated into LDS one super-chunk ahead of the products that use them.
// Parameter groups (PT:129-145, 897): one launch per group with the group's table (its eigenvectors embedded in the full space, rows
// k < nk = the group's size) over the group's list of events (am_fill_kernel's perm): an event's increment is the k-ascending fma
// chain over ITS group's rows, as the step kernel's own product, and lands in the event's row of inc.
template <int G, int MAXT>
__global__ __launch_bounds__(256, 1) void am_gemm_kernel(const AmEvent *ev, const long long *base, long long nch, int d, const double *Ut,
                                                        const double *S, u64 seed, double *inc, int nk, const long long *kbase /* the lists' starts (+ the end) */,
                                                        const int32_t *perm, int grp, int ngroups, int z0 /* first walker of this launch's grid rows */)
{
    constexpr int NEV = 64, K2 = 2 * G;
    extern __shared__ __attribute__((aligned(16))) double Wl[];          // [2][K2][NEV]
    __shared__ int32_t evi[NEV];                                         // parameter groups: the events' indices (their rows of inc)
    // one group (perm == nullptr): the events e0 .. of the chain-ordered list; else entries e0 .. of the group's list
    // the list's key: the group, or (blockIdx.z = the walker, group) with per-walker covariances -- and the key's table
    const long long key = perm ? ((long long)blockIdx.z + z0) * ngroups + grp : 0;
    const long long seg0 = perm ? kbase[key] : 0;
    const long long nev = perm ? kbase[key + 1] - seg0 : base[nch], e0 = (long long)blockIdx.x * NEV;
    if (e0 >= nev) return;
    Ut += (size_t)key * d * d;
    S += (size_t)key * d;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const bool ev_on = e0 + lane < nev;
    const long long mine = ev_on ? e0 + lane : e0;
    const long long ei = perm ? (long long)perm[seg0 + mine] : mine;
    const AmEvent me = ev[ei];
    if (perm && wave == 0) evi[lane] = (int32_t)ei;
    ps_d4 acc[MAXT][4];
#pragma unroll
    for (int tt = 0; tt < MAXT; ++tt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[tt][ct] = ps_d4{0.0, 0.0, 0.0, 0.0};
    const int ntile = (d + 15) / 16, nsup = (nk + K2 - 1) / K2;
    const int tile0 = (int)blockIdx.y * 4 * MAXT + wave;               // this wave's first output tile
    auto gen = [&](int m, int buf) {
        for (int kk = wave; kk < G; kk += 4) {                          // pair (k, k + G) of event `lane`
            const int k = m * K2 + kk;
            double wa = 0.0, wb = 0.0;
            if (ev_on && k < nk) {
                u64 w0, w1;
                philox_words(seed, (u64)me.it, me.sid, SLOT_AM + (u32)k, w0, w1);
                const double r = det_sqrt(-2.0 * unit_log<0>(w0));
                u32 aj;
                double at, sn, cs;
                unit_angle64(w1, aj, at);
                unit_sincos<0>(aj, at, sn, cs);
                wa = (r * cs) * me.cd * det_sqrt(S[k]);                   // PT:930
                if (k + G < nk) wb = (r * sn) * me.cd * det_sqrt(S[k + G]);
            }
            Wl[((size_t)buf * K2 + kk) * NEV + lane] = wa;
            Wl[((size_t)buf * K2 + kk + G) * NEV + lane] = wb;
        }
    };
    gen(0, 0);
    __syncthreads();
    int buf = 0;
    for (int m = 0; m < nsup; ++m) {
        if (m + 1 < nsup) gen(m + 1, buf ^ 1);
        const double *Wb = Wl + (size_t)buf * K2 * NEV + (size_t)g * NEV + c;
        // The table values go four output tiles at a time: the next group's (the next k-step's first group after the last) are
        // requested before the 16 matrix instructions of this one -- one wave per SIMD, nothing else hides the round trip, and
        // the 256 accumulation registers leave no room to hold a whole k-step ahead.
        auto rows_of = [&](int k0, int grp, double (&dst)[4]) {
            const int kr = k0 + g < nk ? k0 + g : nk - 1;                // rows past the end: their weights are zero
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int col = 16 * (tile0 + 4 * (4 * grp + u)) + c;
                dst[u] = Ut[(size_t)kr * d + (col < d ? col : d - 1)];
            }
        };
        double ga[4], gn[4];
        rows_of(m * K2, 0, ga);
#pragma unroll 1
        for (int ks = 0; ks < K2 / 4; ++ks) {
            const int k0 = m * K2 + 4 * ks;
            if (k0 >= nk) break;                                         // uniform
            double bq[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) bq[ct] = Wb[(size_t)(4 * ks) * NEV + 16 * ct];
#pragma unroll
            for (int grp = 0; grp < MAXT / 4; ++grp) {
                if (grp + 1 < MAXT / 4) rows_of(k0, grp + 1, gn);
                else rows_of(k0 + 4 < nk ? k0 + 4 : k0, 0, gn);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (tile0 + 4 * (4 * grp + u) < ntile) {
#pragma unroll
                        for (int ct = 0; ct < 4; ++ct)
                            acc[4 * grp + u][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(ga[u], bq[ct], acc[4 * grp + u][ct], 0, 0, 0);
                    }
#pragma unroll
                for (int u = 0; u < 4; ++u) ga[u] = gn[u];
            }
        }
        __syncthreads();
        buf ^= 1;
    }
#pragma unroll
    for (int tt = 0; tt < MAXT; ++tt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * (tile0 + 4 * tt) + g + 4 * r;
                const long long e = e0 + 16 * ct + c;
                if (i < d && e < nev) inc[(size_t)(perm ? (long long)evi[16 * ct + c] : e) * d + i] = acc[tt][ct][r];
            }
}

// am_gemm_kernel for up to max_events events (blocks beyond the actual count leave at once: no host round trip for it)
template <int G, int MAXT>
static int launch_am_gemm_t(ptmi_engine *h, long long max_events)
{
    const size_t lds = sizeof(double) * 2 * (2 * G) * 64;
    auto kern = am_gemm_kernel<G, MAXT>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return fail(PTMI_EHIP, "hipFuncSetAttribute(%zu B of LDS): %s", lds, hipGetErrorString(e));
    }
    const int d = h->cfg.ndim, ntile = (d + 15) / 16, parts = (ntile + 4 * MAXT - 1) / (4 * MAXT);      // blocks per event tile
    const int ngr = h->cfg.ngroups > 1 ? h->cfg.ngroups : 1;
    // parameter groups: a launch per group (am_gemm_kernel); with per-walker covariances a grid row per walker, its blocks enough for
    // every pick of the walker's chains in the piece
    const int pw = h->cfg.cov_per_walker ? 1 : 0;
    const long long per_key = pw ? (max_events / h->cfg.nwalkers) : max_events;
    // (a grid's z extent ends at 65535: more walkers than that go in several launches)
    const int nz = pw ? h->cfg.nwalkers : 1;
    for (int g = 0; g < ngr; ++g)
        for (int z0 = 0; z0 < nz; z0 += 65535)
            hipLaunchKernelGGL(kern, dim3((unsigned)((per_key + 63) / 64), parts, (unsigned)(nz - z0 < 65535 ? nz - z0 : 65535)), dim3(256), lds, h->stream,
                               (const AmEvent *)h->d_am_ev, (const long long *)h->d_am_base, (long long)h->cfg.nwalkers * h->cfg.ntemps, d,
                               (const double *)h->buf.Ut, (const double *)h->buf.S, h->cfg.seed, h->d_am_inc, ngr > 1 ? h->gsize_host[g] : d,
                               h->d_am_perm ? (const long long *)h->d_am_kbase : nullptr, (const int32_t *)h->d_am_perm, g, ngr, z0);
    return PTMI_OK;
}
static int launch_am_gemm(ptmi_engine *h, long long max_events)
{
    const int ntile = (h->cfg.ndim + 15) / 16;                          // output tiles of an increment
    if (h->G == 4) return launch_am_gemm_t<4, 4>(h, max_events);        // (parameter groups at ndim <= 104: 7 tiles at most)
    if (h->G == 16) return ntile <= 16 ? launch_am_gemm_t<16, 4>(h, max_events) : launch_am_gemm_t<16, 8>(h, max_events);
    if (h->G == 64) return launch_am_gemm_t<64, 8>(h, max_events);
    return fail(PTMI_EINVAL, "AM increments ahead of the launch: unknown shape");
}

// Scratch for the AM increments of one piece of iterations (am_gemm_kernel), and the split path's cursors into it.  An allocation that
// does not fit is no error: the handle then computes its AM products in the step kernels (split_am_piece = am_piece = 0).
hipError_t ptmi_am_scratch_alloc(ptmi_engine *h, bool am_main)
{
    const ptmi_config &c = h->cfg;
    const ptmi_buffers *buf = &h->buf;
    hipError_t e = hipSuccess;
    const long long nch = (long long)c.nwalkers * c.ntemps;
    // scratch for the increments of one piece (6 GB; 2 GB for the split path alone)
    const double budget = (am_main ? ptmi_env("PTMI_AM_BUDGET_MB", 6144.0) : ptmi_env("PTMI_SPLIT_AM_BUDGET_MB", 2048.0)) * 1048576.0;
    long long piece = (long long)(budget / ((double)c.ndim * 8.0 * (double)nch));
    piece = piece < 1 ? 1 : (piece > 64 ? 64 : piece);
    if ((c.ngroups > 1 || c.cov_per_walker) && nch * piece > 0x7FFFFFFFLL) piece = 0x7FFFFFFFLL / nch;      // (the group lists index the events with 32 bits; nch itself is below 2^32 / ntemps)
    if (piece < 1) piece = 1;
    h->am_piece = am_main ? (int)piece : 0;
    h->split_am_piece = (int)piece;
    h->am_cap = nch * piece;
    if (buf->Q != nullptr) e = hipMalloc((void **)&h->d_am_next, sizeof(long long) * (size_t)(nch + 1));
    if (e == hipSuccess)
    e = hipMalloc((void **)&h->d_am_ev, sizeof(AmEvent) * (size_t)h->am_cap);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_am_count, sizeof(int32_t) * (size_t)(nch + (nch + 1023) / 1024));      // counts | the scan's block sums
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_am_base, sizeof(long long) * (size_t)(nch + 1));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_am_inc, sizeof(double) * (size_t)h->am_cap * c.ndim);
    if (e == hipSuccess && (c.ngroups > 1 || c.cov_per_walker)) {    // the events listed key by key: totals | cursors | the scan's block sums; list starts (+ the end)
        const size_t nkeys = (size_t)(c.ngroups > 1 ? c.ngroups : 1) * (c.cov_per_walker ? (size_t)c.nwalkers : 1);
        if (h->am_cap > 0x7FFFFFFFLL) e = hipErrorInvalidValue;
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_am_grp, sizeof(int32_t) * (2 * nkeys + (nkeys + 1023) / 1024 + 1));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_am_kbase, sizeof(long long) * (nkeys + 1));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_am_perm, sizeof(int32_t) * (size_t)h->am_cap);
    }
    if (e == hipErrorOutOfMemory) {
        // no room for the scratch: the step kernels compute their own AM products (slower, the same results) instead of failing the
        // handle -- configurations that fitted before this path existed still do
        (void)hipGetLastError();
        (void)hipFree(h->d_am_ev); (void)hipFree(h->d_am_count); (void)hipFree(h->d_am_base); (void)hipFree(h->d_am_inc);
        (void)hipFree(h->d_am_grp); (void)hipFree(h->d_am_perm); (void)hipFree(h->d_am_kbase);
        h->d_am_ev = nullptr; h->d_am_count = nullptr; h->d_am_base = nullptr; h->d_am_inc = nullptr;
        h->d_am_grp = nullptr; h->d_am_perm = nullptr; h->d_am_kbase = nullptr;
        (void)hipFree(h->d_am_next); h->d_am_next = nullptr;
        h->am_piece = 0; h->am_cap = 0; h->split_am_piece = 0;
        e = hipSuccess;
    }
    return e;
}

// The AM picks of iterations iter0 .. iter0 + ns - 1 listed (am_count / am_scan / am_fill) and their increments computed on the matrix
// cores (am_gemm_kernel) into h->d_am_inc: increment j of a chain's picks in the piece is row h->d_am_base[chain] + j.
int ptmi_am_prepare(ptmi_engine *h, long long iter0, int ns)
{
    const ptmi_config &c = h->cfg;
    const long long nch = (long long)c.nwalkers * c.ntemps;
    AmArgs p;
    p.seed = c.seed; p.iter0 = iter0; p.nch = nch; p.nsteps = ns; p.nt = c.ntemps; p.ntg = c.ntemps_global; p.temp0 = c.temp0;
    p.walker0 = c.walker0; p.w_host = c.w_host; p.w_scam = c.w_scam; p.w_am = c.w_am; p.w_de = h->de_on ? c.w_de : 0;
    p.w_gj = c.w_nuts + c.w_hmc;
    p.pick_walker = c.pick_mode == PTMI_PICK_WALKER; p.ngroups = c.ngroups > 1 ? c.ngroups : 1; p.gcn = h->d_gcn;
    p.per_walker = c.cov_per_walker ? 1 : 0;
    p.temp_of = h->buf.temp_of; p.temps_mh = h->d_temps;
    const unsigned gch = (unsigned)((nch + 255) / 256);
    const int ngr = p.ngroups;
    const long long nkeys = (long long)ngr * (c.cov_per_walker ? c.nwalkers : 1);
    int32_t *gtot = h->d_am_perm ? h->d_am_grp : nullptr, *gcur = gtot ? gtot + nkeys : nullptr, *gpart = gtot ? gtot + 2 * nkeys : nullptr;
    if (gtot) HIPCHK(hipMemsetAsync(gtot, 0, sizeof(int32_t) * 2 * (size_t)nkeys, h->stream));          // the keys' totals and the fill's cursors
    hipLaunchKernelGGL(am_count_kernel, dim3(gch), dim3(256), 0, h->stream, p, h->d_am_count, gtot);
    if (gtot) {                                                  // the lists' starts: the chains' scan over the keys' totals
        const unsigned gk = (unsigned)((nkeys + 1023) / 1024);
        hipLaunchKernelGGL(am_scan_sums_kernel, dim3(gk), dim3(1024), 0, h->stream, (const int32_t *)gtot, gpart, nkeys);
        hipLaunchKernelGGL(am_scan_kernel, dim3(gk), dim3(1024), 0, h->stream, (const int32_t *)gtot, (const int32_t *)gpart, h->d_am_kbase, nkeys);
    }
    const unsigned gsc = (unsigned)((nch + 1023) / 1024);
    hipLaunchKernelGGL(am_scan_sums_kernel, dim3(gsc), dim3(1024), 0, h->stream, (const int32_t *)h->d_am_count, h->d_am_count + nch, nch);
    hipLaunchKernelGGL(am_scan_kernel, dim3(gsc), dim3(1024), 0, h->stream, (const int32_t *)h->d_am_count, (const int32_t *)(h->d_am_count + nch),
                       h->d_am_base, nch);
    hipLaunchKernelGGL(am_fill_kernel, dim3(gch), dim3(256), 0, h->stream, p, (const long long *)h->d_am_base, (AmEvent *)h->d_am_ev,
                       (const long long *)h->d_am_kbase, gcur, gtot ? h->d_am_perm : nullptr);
    if (int rc = launch_am_gemm(h, nch * ns)) return rc;
    return PTMI_OK;
}

extern "C" {

int ptmi_split_am_piece(ptmi_handle h, int32_t *piece)
{
    if (!h || !piece) return fail(PTMI_EINVAL, "NULL argument");
    *piece = (h->cfg.w_am > 0 && ptmi_split_rows_ok(h)) ? h->split_am_piece : 0;
    return PTMI_OK;
}

int ptmi_split_am_prepare(ptmi_handle h, int64_t iter0, int32_t nsteps)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (h->cfg.w_am <= 0) return PTMI_OK;
    if (h->split_am_piece <= 0 || !h->d_am_next) return fail(PTMI_EUNSUPPORTED, "this handle's split path takes its AM proposals from the shape kernels");
    if (nsteps < 1 || nsteps > h->split_am_piece) return fail(PTMI_EINVAL, "ptmi_split_am_prepare: 1 <= nsteps <= %d (ptmi_split_am_piece)", h->split_am_piece);
    if (int rc = ptmi_am_prepare(h, (long long)iter0, nsteps)) return rc;
    const long long nch = (long long)h->cfg.nwalkers * h->cfg.ntemps;
    HIPCHK(hipMemcpyAsync(h->d_am_next, h->d_am_base, sizeof(long long) * (size_t)(nch + 1), hipMemcpyDeviceToDevice, h->stream));      // every chain's cursor at its first increment
    HIPCHK(hipGetLastError());
    h->split_am_lo = iter0;
    h->split_am_hi = iter0 + nsteps;
    return PTMI_OK;
}

}  // extern "C"
