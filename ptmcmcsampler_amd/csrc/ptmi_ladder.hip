// ptmi_ladder.hip -- the temperature ladder adapted on the device from every walker's accepted swaps (ptmi_ladder_attach / _update /
// _publish / _read, include/ptmi.h).  nswap [W][n] (n = ntemps_global; column k = pair (k, k + 1), credited to the lower rank) is in
// device memory behind every swap; one update turns the swaps of the window that just ended into new log gaps and a new ladder:
//
//     acc[k] = sum_w nswap[w][k]                                                    uint64, exact
//     A[k]   = (double)(acc[k] - seen[k]) / ((double)W * (double)(k even ? tries_even : tries_odd))      k = 0 .. n - 2
//     h[k]   = g[k] * det_exp(kappa * A[k])
//     s = 0.0; for k ascending: s = s + h[k]        G = 0.0; for k ascending: G = G + g[k]
//     g'[k]  = G * (h[k] / s)
//     c = 0.0; for k = 1 .. n - 2: c = c + g'[k - 1]; T[k] = T[0] * det_exp(c)
//     seen[k] = acc[k]; g = g'                      T[0] and T[n - 1] are never rewritten
//
// (the build has -ffp-contract=off: every operation rounds on its own; det_exp is ptmi_device.h's, the one ptmi_selftest_math op 1 holds
// to the oracle's bit for bit; the division is IEEE's).  Two launches per update, both on the handle's stream:
//   ladder_sum_kernel     the walkers in slabs, one block each: a thread keeps ONE column and walks down the slab's rows, so that a wave
//                         reads consecutive words of nswap (rank fastest); the block's column sums go to part[slab][n].  Integer sums:
//                         any geometry gives the same numbers.
//   ladder_finish_kernel  ONE block: the slabs' sums per column (the same tiling over part), then the rule, 1024 pairs at a time through
//                         LDS -- the element-wise pieces (A, h, g', the exponentials of T) by all threads, the three running sums (G, s,
//                         c) by thread 0 alone in ascending k, out of LDS -- then the publish step.
// Publish (also ptmi_ladder_publish on its own): d_ladder[k] = T[k]; for every local rank r that followed the ladder at attach time
// (d_temps[r] == d_ladder[temp0 + r]: not the hot chain's 1e80) d_temps[r] = T[temp0 + r], d_beta[r] = 1.0 / d_temps[r]; and with the
// evidence stage attached d_dbeta[r] = d_beta[r - 1] - d_beta[r] for r >= 1.  No host synchronisation, no floating-point atomics (no
// atomics at all), graph-capturable.
#include "ptmi_common.h"
#include <math.h>
#include <vector>

struct ptmi_ladder_state {
    double *lad;               // caller-owned [3][n]: planes g, A, T
    u64 *seen;                 // caller-owned [n]
    u64 *d_part;               // [nslab][n] the slabs' column sums, the library's
    int32_t *d_follow;         // [ntemps] 1 where the local rank samples at its ladder entry
    int nslab, rows_per_slab;
};

namespace {

enum { LAD_G = 0, LAD_A = 1, LAD_T = 2 };
constexpr int LAD_BLOCK = 256;

constexpr int LAD_CHUNK = 1024;        // pairs that pass through LDS at a time in the finishing block

// Column sums of rows [row0, row1) of a uint64 matrix [.][n] over one tile of cw = min(n, 256) columns, 256 / cw rows side by side:
// thread tid keeps column tile * cw + tid % cw and walks down rows rr, rr + R, ... (a wave reads consecutive words), the block folds
// the R partial sums of a column through sh[256].  Returned to threads tid < cw (the column is tile * cw + tid; the caller checks it
// against n).  Integer sums: the order does not matter.
__device__ __forceinline__ u64 tile_colsum(const u64 *__restrict__ m, int n, int cw, int tile, int row0, int row1, u64 *sh)
{
    const int tid = (int)threadIdx.x, R = LAD_BLOCK / cw;
    const int c = tid % cw, rr = tid / cw, col = tile * cw + c;
    u64 s = 0;
    if (rr < R && col < n)
        for (int w = row0 + rr; w < row1; w += R) s += m[(size_t)w * (size_t)n + (size_t)col];
    sh[tid] = s;
    __syncthreads();
    u64 t = 0;
    if (tid < cw)
        for (int j = 0; j < R; ++j) t += sh[j * cw + tid];
    __syncthreads();                                           // sh is free again
    return t;
}

__global__ __launch_bounds__(LAD_BLOCK) void ladder_sum_kernel(const u64 *__restrict__ nswap, u64 *__restrict__ part, int W, int n, int cw,
                                                               int rows_per_slab)
{
    __shared__ u64 sh[LAD_BLOCK];
    const int row0 = (int)blockIdx.x * rows_per_slab;
    const u64 t = tile_colsum(nswap, n, cw, (int)blockIdx.y, row0, min(W, row0 + rows_per_slab), sh);
    const int col = (int)blockIdx.y * cw + (int)threadIdx.x;
    if ((int)threadIdx.x < cw && col < n) part[(size_t)blockIdx.x * (size_t)n + (size_t)col] = t;
}

__device__ __forceinline__ void ladder_publish(const double *__restrict__ T, double *__restrict__ d_ladder, double *__restrict__ d_temps,
                                               double *__restrict__ d_beta, double *__restrict__ d_dbeta,
                                               const int32_t *__restrict__ follow, int n, int nt, int temp0)
{
    const int tid = (int)threadIdx.x;
    for (int k = tid; k < n; k += LAD_BLOCK) d_ladder[k] = T[k];
    for (int r = tid; r < nt; r += LAD_BLOCK)
        if (follow[r]) {
            const double t = T[temp0 + r];
            d_temps[r] = t;
            d_beta[r] = 1.0 / t;
        }
    if (d_dbeta) {
        __syncthreads();                                       // every beta of this block is written
        for (int r = 1 + tid; r < nt; r += LAD_BLOCK) d_dbeta[r] = d_beta[r - 1] - d_beta[r];
    }
}

__global__ __launch_bounds__(LAD_BLOCK) void ladder_finish_kernel(const u64 *__restrict__ part, int nslab, double *__restrict__ lad,
                                                                  u64 *__restrict__ seen, double kappa, double den_even, double den_odd,
                                                                  double *__restrict__ d_ladder, double *__restrict__ d_temps,
                                                                  double *__restrict__ d_beta, double *__restrict__ d_dbeta,
                                                                  const int32_t *__restrict__ follow, int n, int nt, int temp0, int cw)
{
    __shared__ u64 sh[LAD_BLOCK];
    __shared__ double bg[LAD_CHUNK], bh[LAD_CHUNK];
    __shared__ double run[3];                                  // the running sums G, s, c: thread 0 alone adds to them, in ascending k
    const int tid = (int)threadIdx.x, n1 = n - 1;
    double *g = lad + (size_t)LAD_G * n, *A = lad + (size_t)LAD_A * n, *T = lad + (size_t)LAD_T * n;
    // the window's acceptance from the slabs' column sums
    for (int tile = 0; tile * cw < n1; ++tile) {
        const u64 acc = tile_colsum(part, n, cw, tile, 0, nslab, sh);
        const int k = tile * cw + tid;
        if (tid < cw && k < n1) {
            A[k] = (double)(acc - seen[k]) / ((k & 1) ? den_odd : den_even);
            seen[k] = acc;
        }
    }
    if (n > 2) {                                               // (two temperatures: no interior rank, A and seen are all there is)
        if (tid == 0) run[0] = run[1] = run[2] = 0.0;
        __syncthreads();                                       // ... and every A[k] of this block is written
        // G = sum g and s = sum h, h[k] = g[k] * det_exp(kappa * A[k]) (kept in plane g from here on): a chunk of pairs goes through
        // LDS, the exponentials by all threads, the two sums by thread 0
        for (int base = 0; base < n1; base += LAD_CHUNK) {
            const int m = min(LAD_CHUNK, n1 - base);
            for (int i = tid; i < m; i += LAD_BLOCK) {
                const double gk = g[base + i], hk = gk * det_exp(kappa * A[base + i]);
                bg[i] = gk;
                bh[i] = hk;
                g[base + i] = hk;
            }
            __syncthreads();
            if (tid == 0) {
                double G = run[0], s = run[1];
                for (int i = 0; i < m; ++i) {
                    G = G + bg[i];
                    s = s + bh[i];
                }
                run[0] = G;
                run[1] = s;
            }
            __syncthreads();
        }
        const double G = run[0], s = run[1], t0 = T[0];
        // g'[k] = G * (h[k] / s) by all threads; c = the running sum of g' by thread 0; T[k + 1] = T[0] * det_exp(c) by all threads
        for (int base = 0; base < n1; base += LAD_CHUNK) {
            const int m = min(LAD_CHUNK, n1 - base);
            for (int i = tid; i < m; i += LAD_BLOCK) {
                const double gn = G * (g[base + i] / s);
                bg[i] = gn;
                g[base + i] = gn;
            }
            __syncthreads();
            if (tid == 0) {
                double c = run[2];
                for (int i = 0; i < m; ++i) {
                    c = c + bg[i];
                    bh[i] = c;
                }
                run[2] = c;
            }
            __syncthreads();
            for (int i = tid; i < m; i += LAD_BLOCK)
                if (base + i + 1 < n1) T[base + i + 1] = t0 * det_exp(bh[i]);      // ranks 1 .. n - 2: the last pair's sum ends at T[n - 1], which stays
            __syncthreads();
        }
    }
    __syncthreads();
    ladder_publish(T, d_ladder, d_temps, d_beta, d_dbeta, follow, n, nt, temp0);
}

__global__ __launch_bounds__(LAD_BLOCK) void ladder_publish_kernel(const double *__restrict__ lad, double *__restrict__ d_ladder,
                                                                   double *__restrict__ d_temps, double *__restrict__ d_beta,
                                                                   double *__restrict__ d_dbeta, const int32_t *__restrict__ follow, int n,
                                                                   int nt, int temp0)
{
    ladder_publish(lad + (size_t)LAD_T * n, d_ladder, d_temps, d_beta, d_dbeta, follow, n, nt, temp0);
}

}  // namespace

void ptmi_ladder_free(ptmi_engine *h)
{
    ptmi_ladder_state *s = h->ladder;
    if (!s) return;
    (void)hipFree(s->d_part);
    (void)hipFree(s->d_follow);
    delete s;
    h->ladder = nullptr;
}

extern "C" {

int ptmi_ladder_attach(ptmi_handle h, double *lad, uint64_t *seen)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (h->ladder) return fail(PTMI_EINVAL, "ptmi_ladder_attach: already attached");
    if (!lad || ((uintptr_t)lad & 7) != 0) return fail(PTMI_EINVAL, "ptmi_ladder_attach: lad must be non-NULL and 8-byte aligned");
    if (!seen || ((uintptr_t)seen & 7) != 0) return fail(PTMI_EINVAL, "ptmi_ladder_attach: seen must be non-NULL and 8-byte aligned");
    const ptmi_config &c = h->cfg;
    if (c.ntemps_global < 2)
        return fail(PTMI_EINVAL, "ptmi_ladder_attach: ntemps_global = %d: a ladder has at least two temperatures", c.ntemps_global);
    if (c.ntemps != c.ntemps_global || c.temp0 != 0)
        return fail(PTMI_EUNSUPPORTED, "ptmi_ladder_attach: ntemps = %d of ntemps_global = %d: a sharded ladder needs a reduction across "
                                       "blocks", c.ntemps, c.ntemps_global);
    if (!h->buf.nswap) return fail(PTMI_EINVAL, "ptmi_ladder_attach: the handle has no nswap buffer");
    const int n = c.ntemps_global, nt = c.ntemps;
    // which local ranks sample at their ladder entry, from the tables as the device holds them
    std::vector<double> lad_h((size_t)n), tmp_h((size_t)nt);
    std::vector<int32_t> follow((size_t)nt);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(lad_h.data(), h->d_ladder, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(tmp_h.data(), h->d_temps, sizeof(double) * (size_t)nt, hipMemcpyDeviceToHost));
    for (int r = 0; r < nt; ++r) follow[(size_t)r] = tmp_h[(size_t)r] == lad_h[(size_t)(c.temp0 + r)] ? 1 : 0;
    ptmi_ladder_state *s = new ptmi_ladder_state();
    s->lad = lad;
    s->seen = (u64 *)seen;
    const int cw = n < LAD_BLOCK ? n : LAD_BLOCK, R = LAD_BLOCK / cw;
    long long rows = 8ll * R, cap = ((long long)c.nwalkers + 1023) / 1024;      // 8 rows per thread, at most 1024 slabs
    if (rows < cap) rows = (cap + R - 1) / R * R;
    s->rows_per_slab = (int)rows;
    s->nslab = (int)(((long long)c.nwalkers + rows - 1) / rows);
    h->ladder = s;
    hipError_t e = hipMalloc((void **)&s->d_part, sizeof(u64) * (size_t)s->nslab * (size_t)n);
    if (e == hipSuccess) e = hipMalloc((void **)&s->d_follow, sizeof(int32_t) * (size_t)nt);
    if (e == hipSuccess) e = hipMemcpy(s->d_follow, follow.data(), sizeof(int32_t) * (size_t)nt, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        ptmi_ladder_free(h);
        return fail(PTMI_EHIP, "ptmi_ladder_attach: %s", hipGetErrorString(e));
    }
    return PTMI_OK;
}

int ptmi_ladder_update(ptmi_handle h, double kappa, int64_t tries_even, int64_t tries_odd)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    const ptmi_ladder_state *s = h->ladder;
    if (!s) return fail(PTMI_EINVAL, "ptmi_ladder_update: no ladder state is attached (ptmi_ladder_attach)");
    const ptmi_config &c = h->cfg;
    const int n = c.ntemps_global;
    if (!isfinite(kappa) || !(kappa >= 0.0 && kappa <= 8.0))
        return fail(PTMI_EINVAL, "ptmi_ladder_update: kappa must be finite and in [0, 8] (got %g)", kappa);
    if (tries_even < 1) return fail(PTMI_EINVAL, "ptmi_ladder_update: tries_even must be >= 1 (got %lld)", (long long)tries_even);
    if (n - 1 >= 2 && tries_odd < 1) return fail(PTMI_EINVAL, "ptmi_ladder_update: tries_odd must be >= 1 (got %lld)", (long long)tries_odd);
    const int cw = n < LAD_BLOCK ? n : LAD_BLOCK;
    const double Wd = (double)c.nwalkers;
    hipLaunchKernelGGL(ladder_sum_kernel, dim3((unsigned)s->nslab, (unsigned)((n + cw - 1) / cw)), dim3(LAD_BLOCK), 0, h->stream,
                       (const u64 *)h->buf.nswap, s->d_part, (int)c.nwalkers, n, cw, s->rows_per_slab);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(ladder_finish_kernel, dim3(1), dim3(LAD_BLOCK), 0, h->stream, (const u64 *)s->d_part, s->nslab, s->lad, s->seen, kappa,
                       Wd * (double)tries_even, Wd * (double)tries_odd, h->d_ladder, h->d_temps, h->d_beta, ptmi_ev_dbeta(h),
                       (const int32_t *)s->d_follow, n, (int)c.ntemps, (int)c.temp0, cw);
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

int ptmi_ladder_publish(ptmi_handle h)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    const ptmi_ladder_state *s = h->ladder;
    if (!s) return fail(PTMI_EINVAL, "ptmi_ladder_publish: no ladder state is attached (ptmi_ladder_attach)");
    const ptmi_config &c = h->cfg;
    hipLaunchKernelGGL(ladder_publish_kernel, dim3(1), dim3(LAD_BLOCK), 0, h->stream, (const double *)s->lad, h->d_ladder, h->d_temps,
                       h->d_beta, ptmi_ev_dbeta(h), (const int32_t *)s->d_follow, (int)c.ntemps_global, (int)c.ntemps, (int)c.temp0);
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

int ptmi_ladder_read(ptmi_handle h, double *ladder, double *temps_mh, double *beta)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (!h->ladder) return fail(PTMI_EINVAL, "ptmi_ladder_read: no ladder state is attached (ptmi_ladder_attach)");
    if (!ladder || !temps_mh || !beta) return fail(PTMI_EINVAL, "ptmi_ladder_read: ladder, temps_mh and beta must be non-NULL");
    const ptmi_config &c = h->cfg;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(ladder, h->d_ladder, sizeof(double) * (size_t)c.ntemps_global, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(temps_mh, h->d_temps, sizeof(double) * (size_t)c.ntemps, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(beta, h->d_beta, sizeof(double) * (size_t)c.ntemps, hipMemcpyDeviceToHost));
    return PTMI_OK;
}

}  // extern "C"
