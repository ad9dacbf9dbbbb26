// ptmi_eig_wide.hip -- the tridiagonal QL eigensolver (eig_mode "ql", ptmi_eig_ql) for 128 < ndim <= 1024: the three-kernel form of
// ptmi_eig.hip (reduce -> the scalar chains of all matrices at once -> apply) with the n x n matrix in a global scratch instead of
// LDS.  The operations and their order are orc_eig_ql's, as in the LDS kernels: same bits.
//  * eig_qlw_reduce_kernel: one block per matrix; the matrix is read and written in place in the scratch z (8 n^2 bytes: it stays
//    in L2), LDS holds vectors of length n only.  Arithmetic as eig_ql_reduce_kernel, operation for operation.
//  * eig_ql_chain_kernel (ptmi_eig.hip, unchanged): {d, e} alone, 2 n doubles of LDS; records the rotations.
//  * eig_qlw_apply_kernel: the record's rotations turn the rows of Z independently of each other: a grid of matrices x row tiles,
//    a wave per tile, the tile transposed in LDS so that the lanes' rows sit side by side.
//  * eig_qlw_redo_kernel: a matrix whose rotations did not fit the record, chain and rows together on Z in global memory.
//  * eig_qlw_finish_kernel: order and signs across the row tiles, Ut as rows, S.
// No kernel waits for another block; every loop is bounded (QL_MAXIT).
#include "ptmi_common.h"
#include "ptmi_eig_ql.h"

constexpr int QLW_NMAX = 1024;
constexpr int QLW_THREADS = 512, QLW_TY = QLW_THREADS / 16, QLW_OCTS = QLW_THREADS / 8;

// Householder reduction and accumulation of the transformations.  LDS: the current row u, the products p / q (then the products g
// of the accumulation), the subdiagonal e, the diagonal d, column i of the accumulation -- 5 n doubles -- and the set of rows that
// took a Householder step (the oracle's d[i] != 0) as a bit array.  A dot product is the work of an oct of lanes: lane c runs chain
// c of QL_DOT8, the butterfly xor 4, xor 2, xor 1 combines them as the oracle does; the rank-two update and the column updates are
// 16-wide tilings of their elements (128 bytes of a row per 16 lanes).
__global__ __launch_bounds__(QLW_THREADS) void eig_qlw_reduce_kernel(const double *cov, int n, QlScratch q)
{
    extern __shared__ __attribute__((aligned(16))) double wsm[];
    __shared__ unsigned hbits[QLW_NMAX / 32];
    double *u = wsm, *pq = u + n, *e = pq + n, *dg = e + n, *col = dg + n;
    const int t = (int)threadIdx.x;
    const int oct = t >> 3, c8 = t & 7, ty = t >> 4, tx = t & 15;
    const double *A = cov + (size_t)blockIdx.x * n * n;
    double *z = q.z + (size_t)blockIdx.x * n * n;
    for (int i = t; i < n * n; i += QLW_THREADS) z[i] = A[i];
    if (t < QLW_NMAX / 32) hbits[t] = 0u;
    __syncthreads();
    for (int i = n - 1; i >= 1; --i) {
        const int l = i - 1;
        double *zi = z + (size_t)i * n;
        for (int k = t; k <= l; k += QLW_THREADS) u[k] = zi[k];
        __syncthreads();
        double h = 0.0;
        if (l > 0) {
            double sc = 0.0;
            for (int k = c8; k <= l; k += 8) { const double v = u[k]; sc = __builtin_fma(v, v, sc); }
            h = jac_oct_sum(sc);
        }
        if (l == 0 || h == 0.0) {                                 // uniform
            if (t == 0) e[i] = u[l];
            __syncthreads();
            continue;
        }
        const double f0 = u[l];
        const double g0 = f0 >= 0.0 ? -det_sqrt(h) : det_sqrt(h);
        h = h - f0 * g0;
        __syncthreads();                                          // every thread has read u[l]
        if (t == 0) { e[i] = g0; u[l] = f0 - g0; zi[l] = f0 - g0; }
        __syncthreads();
        for (int j = oct; j <= l; j += QLW_OCTS) {
            const double *zj = z + (size_t)j * n;
            double sc = 0.0;
            for (int k = c8; k <= l; k += 8) sc = __builtin_fma(k <= j ? zj[k] : z[(size_t)k * n + j], u[k], sc);
            const double g = jac_oct_sum(sc);
            // the two quotients of row j by two lanes of its oct: one division sequence instead of two on the critical path
            const double quo = (c8 == 0 ? g : u[j]) / h;
            if (c8 == 0) pq[j] = quo;
            else if (c8 == 1) z[(size_t)j * n + i] = quo;
        }
        __syncthreads();
        double fc = 0.0;
        for (int k = c8; k <= l; k += 8) fc = __builtin_fma(pq[k], u[k], fc);
        const double f = jac_oct_sum(fc);
        const double hh = f / (h + h);
        __syncthreads();                                          // every thread has its f
        for (int j = t; j <= l; j += QLW_THREADS) pq[j] = pq[j] - hh * u[j];
        __syncthreads();
        for (int j = ty; j <= l; j += QLW_TY) {
            const double uj = u[j], qj = pq[j];
            double *zj = z + (size_t)j * n;
            for (int k = tx; k <= j; k += 16) zj[k] = zj[k] - (uj * pq[k] + qj * u[k]);
        }
        if (t == 0) hbits[i >> 5] |= 1u << (i & 31);
        __syncthreads();
    }
    if (t == 0) e[0] = 0.0;
    for (int i = 0; i < n; ++i) {
        const int l = i - 1;
        double *zi = z + (size_t)i * n;
        if ((hbits[i >> 5] >> (i & 31)) & 1u) {                   // uniform
            for (int k = t; k <= l; k += QLW_THREADS) { u[k] = zi[k]; col[k] = z[(size_t)k * n + i]; }
            __syncthreads();
            // the products g_j of the leading block's columns with row i
            for (int j = oct; j <= l; j += QLW_OCTS) {
                double sc = 0.0;
                for (int k = c8; k <= l; k += 8) sc = __builtin_fma(u[k], z[(size_t)k * n + j], sc);
                const double g = jac_oct_sum(sc);
                if (c8 == 0) pq[j] = g;
            }
            __syncthreads();
            for (int k = ty; k <= l; k += QLW_TY) {
                const double zki = col[k];
                double *zk = z + (size_t)k * n;
                for (int j = tx; j <= l; j += 16) zk[j] = zk[j] - pq[j] * zki;
            }
        }
        __syncthreads();
        if (t == 0) { dg[i] = zi[i]; zi[i] = 1.0; }
        for (int j = t; j <= l; j += QLW_THREADS) { z[(size_t)j * n + i] = 0.0; zi[j] = 0.0; }
        __syncthreads();
    }
    qls_d2 *deo = q.de + (size_t)blockIdx.x * n;
    for (int i = t; i < n; i += QLW_THREADS) deo[i] = qls_d2{dg[i], i + 1 < n ? e[i + 1] : 0.0};
}

// The record's rotations on a tile of R rows of Z, one wave: lane r holds row row0 + r.  The tile is transposed in LDS, column c at
// zt[c (R + 1) ...] (the lanes' rows side by side; the odd stride keeps the transposing copies off one bank).  The rotations of ONE
// iteration (at most n - 1) are staged in LDS, the next iteration's requested into registers before this one's are applied.  Per
// row the operations and their order are eig_ql_apply_kernel's.  The turned tile goes back to z in place (no other block reads it).
constexpr int QLW_STG = QLW_NMAX / 64;                            // staged rotations per lane
__global__ __launch_bounds__(64) void eig_qlw_apply_kernel(int n, int R, QlScratch q)
{
    extern __shared__ __attribute__((aligned(16))) double wsm[];
    const size_t b = blockIdx.y;
    if (q.cnt[2 * b + 1] != 0) return;                            // the record did not hold this matrix's rotations: eig_qlw_redo_kernel
    qls_d2 *stg = reinterpret_cast<qls_d2 *>(wsm);               // [n]: slot j = the iteration's j-th rotation (columns m - 1 - j, m - j)
    double *zt = wsm + 2 * (size_t)n;
    const int lane = (int)threadIdx.x, RP = R + 1;
    const int row0 = (int)blockIdx.x * R, nr = n - row0 < R ? n - row0 : R;
    double *zg = q.z + b * n * n + (size_t)row0 * n;
    for (int r = 0; r < nr; ++r)
        for (int c = lane; c < n; c += 64) zt[(size_t)c * RP + r] = zg[(size_t)r * n + c];
    const int nit = q.cnt[2 * b];
    const int32_t *hdr = q.hdr + b * 2 * (size_t)q.capit;
    const qls_d2 *rot = q.rot + b * (size_t)q.cap;
    int r = 0;
    int l = nit > 0 ? hdr[0] : 0, m = nit > 0 ? hdr[1] : 0;
    int ln = nit > 1 ? hdr[2] : 0, mn = nit > 1 ? hdr[3] : 0;      // the (l, m) of the iteration after: known two iterations ahead
    for (int j = lane; j < m - l; j += 64) stg[j] = rot[j];
    for (int itn = 0; itn < nit; ++itn) {
        const int cntr = m - l;
        __syncthreads();                                            // this iteration's rotations are staged
        r += cntr;
        const int lnn = itn + 2 < nit ? hdr[2 * itn + 4] : 0, mnn = itn + 2 < nit ? hdr[2 * itn + 5] : 0;
        const int cn = itn + 1 < nit ? mn - ln : 0;
        qls_d2 nx[QLW_STG];
#pragma unroll
        for (int jj = 0; jj < QLW_STG; ++jj) nx[jj] = lane + 64 * jj < cn ? rot[r + lane + 64 * jj] : qls_d2{0.0, 0.0};
        if (lane < nr) {
            double zb = zt[(size_t)m * RP + lane];
            double *zp = zt + (size_t)(m - 1) * RP + lane;          // column i of this lane's row, i descending
            int j = 0;
            for (; j + 4 <= cntr; j += 4, zp -= 4 * RP) {          // four rotations a trip: their reads go out together
                const qls_d2 c0 = stg[j], c1 = stg[j + 1], c2 = stg[j + 2], c3 = stg[j + 3];
                const double a0 = zp[0], a1 = zp[-RP], a2 = zp[-2 * RP], a3 = zp[-3 * RP];
                zp[RP] = c0.y * a0 + c0.x * zb;
                zb = c0.x * a0 - c0.y * zb;
                zp[0] = c1.y * a1 + c1.x * zb;
                zb = c1.x * a1 - c1.y * zb;
                zp[-RP] = c2.y * a2 + c2.x * zb;
                zb = c2.x * a2 - c2.y * zb;
                zp[-2 * RP] = c3.y * a3 + c3.x * zb;
                zb = c3.x * a3 - c3.y * zb;
            }
            for (; j < cntr; ++j, zp -= RP) {
                const qls_d2 cs = stg[j];
                const double za = zp[0];
                zp[RP] = cs.y * za + cs.x * zb;
                zb = cs.x * za - cs.y * zb;
            }
            zt[(size_t)l * RP + lane] = zb;
        }
        __syncthreads();                                            // every lane has applied the staged rotations
#pragma unroll
        for (int jj = 0; jj < QLW_STG; ++jj) if (lane + 64 * jj < cn) stg[lane + 64 * jj] = nx[jj];
        l = ln; m = mn;
        ln = lnn; mn = mnn;
    }
    __syncthreads();
    for (int rr = 0; rr < nr; ++rr)
        for (int c = lane; c < n; c += 64) zg[(size_t)rr * n + c] = zt[(size_t)c * RP + rr];
}

// A matrix whose rotations did not fit the record: the chain and the rows together, rows t, t + 64, ... of Z in global memory
// (ql_iterate<true, true>).  One wave per flagged matrix; slow and rare, like the LDS kernels' redo.
__global__ __launch_bounds__(64) void eig_qlw_redo_kernel(int n, QlScratch q)
{
    extern __shared__ __attribute__((aligned(16))) double wsm[];
    const size_t b = blockIdx.x;
    if (q.cnt[2 * b + 1] == 0) return;
    qls_d2 *de = reinterpret_cast<qls_d2 *>(wsm);
    const int t = (int)threadIdx.x;
    for (int i = t; i < n; i += 64) de[i] = q.de[b * n + i];
    asm volatile("" ::: "memory");
    __syncthreads();
    ql_iterate<true, true>(de, n, t, q.z + b * n * n, nullptr, nullptr, 0, 0, nullptr);
    asm volatile("" ::: "memory");
    __syncthreads();
    for (int i = t; i < n; i += 64) q.ev[b * n + i] = de[i].x;
}

// Order and signs as orc_eig_ql, for 32 columns of Z per block: rank by |eigenvalue| descending (ties by ascending column); the
// eigenvector's first component of largest magnitude (lowest row, strict >) becomes positive -- eight threads per column scan
// eight runs of consecutive rows, and the runs are combined in ascending order with the same strict comparison, so the first of
// equals survives; then the columns go out as rows of Ut through a 32 x 32 LDS tile (both sides coalesced).
__global__ __launch_bounds__(256) void eig_qlw_finish_kernel(double *Ut, double *S, int n, int ut_stride, int s_stride, QlScratch q)
{
    extern __shared__ __attribute__((aligned(16))) double wsm[];   // the eigenvalues
    __shared__ double tile[32][33], cmax[8][32], cval[8][32], sgs[32];
    __shared__ int rpart[8][32], rk[32];
    double *ev = wsm;
    const int t = (int)threadIdx.x, tx = t & 31, ty = t >> 5;
    const size_t b = blockIdx.y;
    const int k0 = (int)blockIdx.x * 32, k = k0 + tx;
    const double *z = q.z + b * n * n;
    for (int i = t; i < n; i += 256) ev[i] = q.ev[b * n + i];
    __syncthreads();
    {
        const int chunk = (n + 7) / 8, i0 = ty * chunk, i1 = i0 + chunk < n ? i0 + chunk : n;
        double best = -1.0, bval = 0.0;
        int cnt = 0;
        if (k < n) {
            const double mine = __builtin_fabs(ev[k]);
            for (int j = ty; j < n; j += 8) { const double o = __builtin_fabs(ev[j]); cnt += (o > mine) || (o == mine && j < k); }
            for (int i = i0; i < i1; ++i) {
                const double v = z[(size_t)i * n + k], a = __builtin_fabs(v);
                if (a > best) { best = a; bval = v; }
            }
        }
        cmax[ty][tx] = best; cval[ty][tx] = bval; rpart[ty][tx] = cnt;
    }
    __syncthreads();
    if (ty == 0 && k < n) {
        double best = cmax[0][tx], bval = cval[0][tx];
        int rank = rpart[0][tx];
        for (int g = 1; g < 8; ++g) {
            if (cmax[g][tx] > best) { best = cmax[g][tx]; bval = cval[g][tx]; }
            rank += rpart[g][tx];
        }
        sgs[tx] = bval < 0.0 ? -1.0 : 1.0;
        rk[tx] = rank;
        S[b * s_stride + rank] = __builtin_fabs(ev[k]);
    }
    __syncthreads();
    double *Uo = Ut + b * ut_stride;
    for (int i0 = 0; i0 < n; i0 += 32) {
        for (int rr = ty; rr < 32; rr += 8) tile[rr][tx] = (i0 + rr < n && k < n) ? z[(size_t)(i0 + rr) * n + k] : 0.0;
        __syncthreads();
        for (int cc = ty; cc < 32; cc += 8)
            if (k0 + cc < n && i0 + tx < n) Uo[(size_t)rk[cc] * n + i0 + tx] = sgs[cc] * tile[tx][cc];
        __syncthreads();
    }
}

// Rows per tile of eig_qlw_apply_kernel: the most rows a CU's 160 KB of LDS hold at once, the larger tile on a tie
static int qlw_apply_rows(int n, size_t *lds_out)
{
    int best = 8, best_rows = -1;
    for (int R = 64; R >= 8; R >>= 1) {
        const size_t lds = sizeof(double) * ((size_t)n * (R + 1) + 2 * (size_t)n);
        if (lds > 160 * 1024) continue;
        const int rows = (int)((160 * 1024) / lds) * R;
        if (rows > best_rows) { best_rows = rows; best = R; }
    }
    *lds_out = sizeof(double) * ((size_t)n * (best + 1) + 2 * (size_t)n);
    return best;
}

// nmat symmetric matrices of order 128 < n <= 1024, as eig_ql_run.  The scratch is some 7 n^2 doubles per matrix (z, the record of
// 2 cap doubles, de, ev, the headers): the matrices are factorized in batches that fit QLW_BUDGET_MB, queued one after another on
// the stream; a matrix's result does not depend on its batch.  PTMI_QL_SPLIT = 0 (the test hook that asks for chain and rows
// together, below 128 as one kernel per matrix) gives the record no room here: every matrix that rotates at all is flagged by the
// chain kernel and takes eig_qlw_redo_kernel -- the same bits.
constexpr double QLW_BUDGET_MB = 4096.0;
int eig_ql_wide_run(ptmi_engine *h, int n, int nmat, const double *cov, double *Ut, double *S)
{
    if (n <= 128 || n > QLW_NMAX) return fail(PTMI_EUNSUPPORTED, "the wide QL eigensolver factorizes matrices of order 129 .. 1024 (this one: %d)", n);
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const bool together = ptmi_env("PTMI_QL_SPLIT", 1) == 0;
    const int cap = 3 * n * n, capit = 8 * n;
    const size_t per = sizeof(double) * ((size_t)n * n + 2 * (size_t)n + 2 * (size_t)cap + (size_t)n) + sizeof(int32_t) * (2 * (size_t)capit + 2);
    const double budget = QLW_BUDGET_MB * 1048576.0;
    long long nb = (long long)(budget / (double)per);
    if (nb < 1) nb = 1;
    if (nb > nmat) nb = nmat;
    if (nb > 65535) nb = 65535;                                       // (the grids' second dimension)
    const size_t need = (size_t)nb * per + 6 * 16;
    if (need > h->qlw_scr_bytes) {                                    // (hipFree waits for the work that still uses the old one)
        if (h->d_qlw_scr) { HIPCHK(hipFree(h->d_qlw_scr)); h->d_qlw_scr = nullptr; h->qlw_scr_bytes = 0; }
        HIPCHK(hipMalloc((void **)&h->d_qlw_scr, need));
        h->qlw_scr_bytes = need;
    }
    QlScratch q;
    char *pb = (char *)h->d_qlw_scr;
    q.z = (double *)pb; pb += up16(sizeof(double) * (size_t)nb * n * n);
    q.de = (qls_d2 *)pb; pb += sizeof(double) * 2 * (size_t)nb * n;
    q.rot = (qls_d2 *)pb; pb += sizeof(double) * 2 * (size_t)nb * cap;
    q.ev = (double *)pb; pb += up16(sizeof(double) * (size_t)nb * n);
    q.hdr = (int32_t *)pb; pb += up16(sizeof(int32_t) * 2 * (size_t)nb * capit);
    q.cnt = (int32_t *)pb;
    q.cap = together ? 0 : cap; q.capit = capit;
    size_t lds_apply = 0;
    const int R = qlw_apply_rows(n, &lds_apply);
    if (lds_apply > 64 * 1024)
        HIPCHK(hipFuncSetAttribute((const void *)eig_qlw_apply_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_apply));
    const size_t lds_reduce = sizeof(double) * 5 * (size_t)n, lds_de = sizeof(double) * 2 * (size_t)n;
    for (int m0 = 0; m0 < nmat; m0 += (int)nb) {
        const int cnt = nmat - m0 < (int)nb ? nmat - m0 : (int)nb;
        hipLaunchKernelGGL(eig_qlw_reduce_kernel, dim3(cnt), dim3(QLW_THREADS), lds_reduce, h->stream, cov + (size_t)m0 * n * n, n, q);
        eig_ql_chain_launch(h->stream, n, cnt, q);
        hipLaunchKernelGGL(eig_qlw_apply_kernel, dim3((n + R - 1) / R, cnt), dim3(64), lds_apply, h->stream, n, R, q);
        hipLaunchKernelGGL(eig_qlw_redo_kernel, dim3(cnt), dim3(64), lds_de, h->stream, n, q);
        hipLaunchKernelGGL(eig_qlw_finish_kernel, dim3((n + 31) / 32, cnt), dim3(256), sizeof(double) * (size_t)n, h->stream,
                           Ut + (size_t)m0 * n * n, S + (size_t)m0 * n, n, n * n, n, q);
    }
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}
