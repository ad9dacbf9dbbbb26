// ptmi_eig.hip -- the device eigensolvers of libptmi.so (eig_mode "jacobi", "ql", "sytrd"): every solver's kernels with its entry
// points directly below them.  They reach the engine through the handle's fields only (ptmi_common.h).
#include <math.h>
#include <stdlib.h>

#include <new>
#include <mutex>
#include <vector>

#include "ptmi_common.h"
#include "ptmi_eig_ql.h"

// ---------------------------------------------------------- eigensolver
// Batched symmetric eigensolver for the per-walker covariances (PT:797-803 calls LAPACK's SVD once per epoch; a batch of
// thousands of walkers would queue thousands of host factorizations).  One block per matrix, one-sided (Hestenes) Jacobi
// on the rows of W = V^T A with W and V^T both in LDS: in every round of the circle-method schedule the n/2 disjoint row
// pairs are rotated at once, eight lanes per pair (lane l owns elements l, l+8, ... of both rows, cached in registers
// for the three dot products and the rotation); one barrier per round.  Operation order = oracle/ptmcmc_oracle.c orc_eig_jacobi,
// so the results are bit-identical to it.  Eigenvalues descending, eigenvectors as rows, largest component positive.
constexpr int JAC_THREADS = 512;                            // 8 lanes per row pair, up to 64 pairs (ndim <= 101 uses 51)
constexpr int JAC_L = 8;
constexpr int JAC_MAX_SWEEPS = 30;
__global__ __launch_bounds__(JAC_THREADS) void eig_jacobi_kernel(const double *cov, double *Ut, double *S, int d, int ut_stride, int s_stride)
{
    extern __shared__ __attribute__((aligned(16))) double jsm[];     // W[d][d], V[d][d]: all of the CU's LDS at d = 101
    double *W = jsm, *V = jsm + (size_t)d * d;
    constexpr int NE = 13;                                           // elements of a row per lane: l, l + 8, ... < 104
    const int tid = (int)threadIdx.x;
    const double *A = cov + (size_t)blockIdx.x * d * d;
    for (int i = tid; i < d * d; i += JAC_THREADS) {
        W[i] = A[i];
        V[i] = (i / d == i % d) ? 1.0 : 0.0;
    }
    const int n = d + (d & 1), P = n / 2, rounds = n - 1;
    const int pr = tid / JAC_L, l = tid % JAC_L;
    __syncthreads();
    for (int sweep = 0; sweep < JAC_MAX_SWEEPS; ++sweep) {
        int rotated = 0;
        for (int r = 0; r < rounds; ++r) {
            if (pr < P) {                                            // P <= 51 pairs: eight lanes each
                const int k = pr;
                const int a = k == 0 ? n - 1 : (r + k) % (n - 1);
                const int b = k == 0 ? r : (r - k + (n - 1)) % (n - 1);
                const int p = a < b ? a : b, q = a < b ? b : a;
                const bool real = q < d;                             // the bye of an odd dimension
                double *wp = W + (size_t)p * d, *wq = W + (size_t)(real ? q : p) * d;
                // both rows into registers once (zeros beyond the row: fma(0, 0, s) = s leaves the sums untouched)
                double xp[NE], xq[NE];
#pragma unroll
                for (int j = 0; j < NE; ++j) {
                    const int i = l + JAC_L * j;
                    xp[j] = i < d ? wp[i] : 0.0;
                    xq[j] = i < d ? wq[i] : 0.0;
                }
                double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
                for (int j = 0; j < NE; ++j) {
                    al = __builtin_fma(xp[j], xp[j], al);
                    be = __builtin_fma(xq[j], xq[j], be);
                    ga = __builtin_fma(xp[j], xq[j], ga);
                }
                al = jac_oct_sum(al); be = jac_oct_sum(be); ga = jac_oct_sum(ga);
                if (real && __builtin_fabs(ga) > 0x1.0p-50 * det_sqrt(al * be)) {      // uniform over the pair's lanes
                    const double zeta = (be - al) / (2.0 * ga);
                    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (__builtin_fabs(zeta) + det_sqrt(1.0 + zeta * zeta));
                    const double c = 1.0 / det_sqrt(1.0 + t * t), sn = c * t;
                    double *vp = V + (size_t)p * d, *vq = V + (size_t)q * d;
#pragma unroll
                    for (int j = 0; j < NE; ++j) {
                        const int i = l + JAC_L * j;
                        if (i < d) {
                            const double u = vp[i], v = vq[i];
                            wp[i] = c * xp[j] - sn * xq[j];
                            wq[i] = sn * xp[j] + c * xq[j];
                            vp[i] = c * u - sn * v;
                            vq[i] = sn * u + c * v;
                        }
                    }
                    rotated = 1;
                }
            }
            __syncthreads();
        }
        if (!__syncthreads_or(rotated)) break;
    }
    // norms (eight lanes per row, same summation as above): first in registers, then -- W is dead -- in W[0..d)
    double mynorm[2] = {0.0, 0.0};
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int k = pass * (JAC_THREADS / JAC_L) + pr;
        double al = 0.0;
        if (k < d)
            for (int j = 0; j < NE; ++j) { const int i = l + JAC_L * j; const double x = i < d ? W[(size_t)k * d + i] : 0.0; al = __builtin_fma(x, x, al); }
        mynorm[pass] = det_sqrt(jac_oct_sum(al));
    }
    __syncthreads();                                                 // every row of W has been read: W[0..d) now holds the norms
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int k = pass * (JAC_THREADS / JAC_L) + pr;
        if (k < d && l == 0) W[k] = mynorm[pass];
    }
    __syncthreads();
    const double *nrm = W;
    double *Uo = Ut + (size_t)blockIdx.x * ut_stride, *So = S + (size_t)blockIdx.x * s_stride;
    for (int k = pr; k < d; k += JAC_THREADS / JAC_L) {
        const double mine = nrm[k];
        int rank = 0;
        for (int j = 0; j < d; ++j) rank += (nrm[j] > mine) || (nrm[j] == mine && j < k);
        const double *vk = V + (size_t)k * d;
        int im = 0;
        for (int i = 1; i < d; ++i) if (__builtin_fabs(vk[i]) > __builtin_fabs(vk[im])) im = i;
        const double sg = vk[im] < 0.0 ? -1.0 : 1.0;
        for (int i = l; i < d; i += JAC_L) Uo[(size_t)rank * d + i] = sg * vk[i];
        if (l == 0) So[rank] = mine;
    }
}

int ptmi_eig_jacobi(ptmi_handle h)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    const ptmi_config &c = h->cfg;
    if (!h->buf.cov || !h->buf.Ut || !h->buf.S) return fail(PTMI_EINVAL, "cov / Ut / S buffers missing");
    if (c.ngroups > 1) return fail(PTMI_EUNSUPPORTED, "the device eigensolver factorizes the full covariance (no parameter groups)");
    const int d = c.ndim;
    const size_t lds = sizeof(double) * 2 * (size_t)d * d;
    if (lds > 160 * 1024 || d > 101) return fail(PTMI_EUNSUPPORTED, "the device eigensolver keeps two %d x %d tables in LDS: ndim <= 101", d, d);
    if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)eig_jacobi_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int nmat = c.cov_per_walker ? c.nwalkers : 1;
    hipLaunchKernelGGL(eig_jacobi_kernel, dim3(nmat), dim3(JAC_THREADS), lds, h->stream, (const double *)h->buf.cov, h->buf.Ut, h->buf.S,
                       d, d * d, d);
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

// ----------------------------------------------------------- tridiagonal QL eigensolver (eig_mode "ql")
// The eigendecomposition of PT:797-803 by Householder tridiagonalization with the transformations accumulated, then implicit QL
// iterations on the tridiagonal matrix (oracle: orc_eig_ql -- the kernel does the oracle's operations in the oracle's order, dot products
// as eight interleaved fma chains, so both give the same bits).  eig_jacobi_kernel needs nine sweeps of n^2 / 2
// rotations, each moving two rows of W and two of V through LDS (4.4 ms per 100 x 100 matrix, one matrix per CU), on the nearly
// degenerate spectra an isotropic target adapts to; here the O(n^3) work is two passes over the matrix and the rest is a chain of
// some 7500 plane rotations whose scalars depend on each other (one sqrt and one division each) while the columns they turn do not.
// One block of two waves per matrix, two blocks per CU at ndim = 100 (the matrix, the subdiagonal and one work row: 81.6 KB):
//  * reduction, row i = n-1 .. 1: every thread forms the row's scalars itself (broadcast reads: no barrier for them); thread j owns
//    row j of the products p = A u / h and of the rank-two update;
//  * accumulation, row i = 0 .. n-1: thread j owns column j of the leading block (its product and its update need nothing else);
//  * QL: ONE wave (64 lanes, rows k and k + 64 of the eigenvector matrix each) runs the scalar recurrence in every lane and turns
//    its rows; nothing is synchronised inside this phase.
constexpr int QL_THREADS = 128;
// the oracle's QL_DOT8: eight interleaved fma chains, term k into chain k mod 8 (a dependent f64 operation costs a lone wave some 20
// cycles: one chain of 100 terms is 2000 cycles, eight side by side 300)
template <class FA, class FB>
__device__ __forceinline__ double ql_dot8(int cnt, FA fa, FB fb)
{
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
    int k = 0;
    for (; k + 8 <= cnt; k += 8) {
        s0 = __builtin_fma(fa(k), fb(k), s0);
        s1 = __builtin_fma(fa(k + 1), fb(k + 1), s1);
        s2 = __builtin_fma(fa(k + 2), fb(k + 2), s2);
        s3 = __builtin_fma(fa(k + 3), fb(k + 3), s3);
        s4 = __builtin_fma(fa(k + 4), fb(k + 4), s4);
        s5 = __builtin_fma(fa(k + 5), fb(k + 5), s5);
        s6 = __builtin_fma(fa(k + 6), fb(k + 6), s6);
        s7 = __builtin_fma(fa(k + 7), fb(k + 7), s7);
    }
    if (k < cnt) s0 = __builtin_fma(fa(k), fb(k), s0);
    if (k + 1 < cnt) s1 = __builtin_fma(fa(k + 1), fb(k + 1), s1);
    if (k + 2 < cnt) s2 = __builtin_fma(fa(k + 2), fb(k + 2), s2);
    if (k + 3 < cnt) s3 = __builtin_fma(fa(k + 3), fb(k + 3), s3);
    if (k + 4 < cnt) s4 = __builtin_fma(fa(k + 4), fb(k + 4), s4);
    if (k + 5 < cnt) s5 = __builtin_fma(fa(k + 5), fb(k + 5), s5);
    if (k + 6 < cnt) s6 = __builtin_fma(fa(k + 6), fb(k + 6), s6);
    return ((s0 + s4) + (s2 + s6)) + ((s1 + s5) + (s3 + s7));
}
// (Measured and dropped: the matrix in a global scratch with 3 n doubles of LDS per block, sixteen blocks per CU and all 4096 matrices
// resident at once -- every broadcast read became an L2 round trip: 84 ms per epoch against 41.)
__global__ __launch_bounds__(QL_THREADS) void eig_ql_kernel(const double *cov, double *Ut, double *S, int n, int ut_stride, int s_stride, int32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) double qsm[];
    double *z = qsm, *e = qsm + (((size_t)n * n + 1) & ~(size_t)1), *pq = e + n;     // pq: the products p / h, then q; after the accumulation: the diagonal d
    const int t = (int)threadIdx.x;
    const double *A = cov + (size_t)blockIdx.x * n * n;
#define QZ(i, j) z[(i) * n + (j)]
    for (int i = t; i < n * n; i += QL_THREADS) z[i] = A[i];
#ifdef PTMI_QL_PROFILE
    unsigned long long qt0 = __builtin_readcyclecounter(), qt1, qt2, qt3;
#endif
    unsigned long long hmask[2] = {0ull, 0ull};                   // rows whose reflector exists (the oracle's d[i] != 0), n <= 128
    __syncthreads();
    for (int i = n - 1; i >= 1; --i) {
        const int l = i - 1;
        double h = 0.0;
        if (l > 0) h = ql_dot8(l + 1, [&](int k) { return QZ(i, k); }, [&](int k) { return QZ(i, k); });
        if (l == 0 || h == 0.0) {                                 // uniform
            if (t == 0) e[i] = QZ(i, l);
            __syncthreads();
            continue;
        }
        const double f0 = QZ(i, l);
        const double g0 = f0 >= 0.0 ? -det_sqrt(h) : det_sqrt(h);
        h = h - f0 * g0;
        __syncthreads();                                          // every thread has read Z(i, l)
        if (t == 0) { e[i] = g0; QZ(i, l) = f0 - g0; }
        __syncthreads();
        for (int j = t; j <= l; j += QL_THREADS) {
            QZ(j, i) = QZ(i, j) / h;
            const double g = ql_dot8(l + 1, [&](int k) { return k <= j ? QZ(j, k) : QZ(k, j); }, [&](int k) { return QZ(i, k); });
            pq[j] = g / h;
        }
        __syncthreads();
        const double f = ql_dot8(l + 1, [&](int k) { return pq[k]; }, [&](int k) { return QZ(i, k); });
        const double hh = f / (h + h);
        __syncthreads();                                          // every thread has its f
        for (int j = t; j <= l; j += QL_THREADS) pq[j] = pq[j] - hh * QZ(i, j);
        __syncthreads();
        for (int j = t; j <= l; j += QL_THREADS) {
            const double uj = QZ(i, j), qj = pq[j];
            for (int k = 0; k <= j; ++k) QZ(j, k) = QZ(j, k) - (uj * pq[k] + qj * QZ(i, k));
        }
        hmask[i >> 6] |= 1ull << (i & 63);
        __syncthreads();
    }
    if (t == 0) e[0] = 0.0;
#ifdef PTMI_QL_PROFILE
    qt1 = __builtin_readcyclecounter();
#endif
    // accumulation of the transformations
    for (int i = 0; i < n; ++i) {
        const int l = i - 1;
        if ((hmask[i >> 6] >> (i & 63)) & 1ull) {
            for (int j = t; j <= l; j += QL_THREADS) {
                const double g = ql_dot8(l + 1, [&](int k) { return QZ(i, k); }, [&](int k) { return QZ(k, j); });
                for (int k = 0; k <= l; ++k) QZ(k, j) = QZ(k, j) - g * QZ(k, i);
            }
        }
        __syncthreads();
        if (t == 0) { pq[i] = QZ(i, i); QZ(i, i) = 1.0; }
        for (int j = t; j <= l; j += QL_THREADS) { QZ(j, i) = 0.0; QZ(i, j) = 0.0; }
        __syncthreads();
    }
    // ---- implicit QL: one wave, no barrier; lane `t` turns rows t and t + 64.  The diagonal and the subdiagonal are re-laid as
    // pairs {d[i], e[i]} over the 2 n doubles of e and pq (one 16-byte read and one 16-byte write per rotation); of the two
    // columns a rotation turns, the lower one is the next rotation's upper one and stays in a register.
    typedef double ql_d2 __attribute__((ext_vector_type(2)));
    ql_d2 *de = reinterpret_cast<ql_d2 *>(e);
    int iters = 0, failed = 0;
#ifdef PTMI_QL_PROFILE
    qt2 = __builtin_readcyclecounter();
#endif
    if (t < 64) {
        const int k0 = t, k1 = t + 64;
        const bool r0 = k0 < n, r1 = k1 < n;
        {
            // e[i - 1] = e[i], e[n - 1] = 0, then the pairs: every lane reads its entries before any lane writes
            const int ia = t, ib = t + 64;
            const double da = ia < n ? pq[ia] : 0.0, db = ib < n ? pq[ib] : 0.0;
            const double ea = ia + 1 < n ? e[ia + 1] : 0.0, eb = ib + 1 < n ? e[ib + 1] : 0.0;
            asm volatile("" ::: "memory");
            if (ia < n) de[ia] = ql_d2{da, ea};
            if (ib < n) de[ib] = ql_d2{db, eb};
            asm volatile("" ::: "memory");
        }
#define QD(i) de[i].x
#define QE(i) de[i].y
        double f = 0.0, tst1 = 0.0;
        for (int l = 0; l < n && !failed; ++l) {
            const ql_d2 del = de[l];
            const double t0 = __builtin_fabs(del.x) + __builtin_fabs(del.y);
            if (tst1 < t0) tst1 = t0;
            int m = l;
            while (m < n - 1 && tst1 + __builtin_fabs(QE(m)) != tst1) ++m;
            double dlf = del.x;                                  // d[l] as the iterations leave it
            if (m > l) {
                int it = 0;
                double el;
                do {
                    if (++it > QL_MAXIT) { failed = 1; break; }
                    ++iters;
                    const ql_d2 pl = de[l], pl1 = de[l + 1];
                    const double g = pl.x, e_l = pl.y;
                    const double p0 = (pl1.x - g) / (2.0 * e_l);
                    const double rr0 = det_sqrt(p0 * p0 + 1.0);
                    const double pr = p0 + (p0 >= 0.0 ? rr0 : -rr0);
                    const double dl = e_l / pr, dl1 = e_l * pr;
                    const double h = g - dl;
                    const double el1 = pl1.y;
                    double p = QD(m);
                    asm volatile("" ::: "memory");
                    if (t == 0) { QD(l) = dl; QD(l + 1) = dl1; }
                    for (int i = l + 2 + t; i < n; i += 64) QD(i) = QD(i) - h;
                    asm volatile("" ::: "memory");
                    f = f + h;
                    if (m == l + 1) p = dl1; else if (m >= l + 2) p = p - h;     // d[m] as the updates above leave it
                    double c = 1.0, c2 = 1.0, c3 = 1.0, s = 0.0, s2 = 0.0;
                    ql_d2 nx = de[m - 1];                            // the next rotation's inputs are asked for a rotation ahead
                    double zb0 = r0 ? z[k0 * n + m] : 0.0, zb1 = r1 ? z[k1 * n + m] : 0.0;     // column i + 1 of the lane's rows, carried
                    for (int i = m - 1; i >= l; --i) {
                        c3 = c2; c2 = c; s2 = s;
                        const double di = nx.x, ei = nx.y;
                        if (i > l) nx = de[i - 1];
                        const double za0 = r0 ? z[k0 * n + i] : 0.0, za1 = r1 ? z[k1 * n + i] : 0.0;
                        const double gg = c * ei, hh = c * p;
                        double r, ri;
                        ql_root_and_reciprocal(p * p + ei * ei, r, ri);
                        const double e1 = s * r;
                        s = ei * ri;
                        c = p * ri;
                        p = c * di - s * gg;
                        const double d1 = hh + s * (c * gg + s * di);
                        if (t == 0) de[i + 1] = ql_d2{d1, e1};
                        if (r0) z[k0 * n + i + 1] = s * za0 + c * zb0;
                        if (r1) z[k1 * n + i + 1] = s * za1 + c * zb1;
                        zb0 = c * za0 - s * zb0;
                        zb1 = c * za1 - s * zb1;
                    }
                    if (r0) z[k0 * n + l] = zb0;
                    if (r1) z[k1 * n + l] = zb1;
                    p = -s * s2 * c3 * el1 * e_l / dl1;
                    el = s * p;
                    dlf = c * p;
                    asm volatile("" ::: "memory");
                    if (t == 0) de[l] = ql_d2{dlf, el};
                    asm volatile("" ::: "memory");
                } while (tst1 + __builtin_fabs(el) != tst1);
            }
            asm volatile("" ::: "memory");
            if (t == 0) de[l] = ql_d2{dlf + f, 0.0};
            asm volatile("" ::: "memory");
        }
        if (t == 0 && status) {
            if (failed) atomicOr(status, 1);
        }
    }
    __syncthreads();
#ifdef PTMI_QL_PROFILE
    qt3 = __builtin_readcyclecounter();
    if (t == 0 && (blockIdx.x == 0 || blockIdx.x == 3000)) printf("ql block %d: reduce %llu accumulate %llu ql %llu cycles, %d iterations\n", (int)blockIdx.x, qt1 - qt0, qt2 - qt1, qt3 - qt2, iters);
#endif
    // order and signs as eig_jacobi_kernel / orc_eig_ql
    double *Uo = Ut + (size_t)blockIdx.x * ut_stride, *So = S + (size_t)blockIdx.x * s_stride;
    for (int k = t; k < n; k += QL_THREADS) {
        const double mine = __builtin_fabs(QD(k));
        int rank = 0;
        for (int j = 0; j < n; ++j) { const double o = __builtin_fabs(QD(j)); rank += (o > mine) || (o == mine && j < k); }
        int im = 0;
        for (int i = 1; i < n; ++i) if (__builtin_fabs(QZ(i, k)) > __builtin_fabs(QZ(im, k))) im = i;
        const double sg = QZ(im, k) < 0.0 ? -1.0 : 1.0;
        for (int i = 0; i < n; ++i) Uo[(size_t)rank * n + i] = sg * QZ(i, k);
        So[rank] = mine;
    }
#undef QZ
#undef QD
#undef QE
}

// ---- the same in three kernels, for MANY matrices (per-walker covariances).  The QL phase is a chain of dependent scalar
// operations (some 45 of them per rotation, ~20 cycles each for a lone wave: 900 cycles per rotation, 7.6 of the 10.3 M cycles a
// matrix takes in eig_ql_kernel) and only two matrices fit a CU's LDS: 64 ms of chain per CU and epoch whatever is done to the rest.
// But the chain needs the tridiagonal matrix alone -- 200 doubles, not the eigenvectors: eig_ql_chain_kernel runs the chains of ALL
// matrices at once (a wave each, four per SIMD) and RECORDS the rotations (c, s) with the (l, m) of every iteration;
// eig_ql_apply_kernel then turns the eigenvector rows with them, a thread per row and no scalar work.  Same operations on the
// same values in the same order as orc_eig_ql: same bits.  A matrix whose rotations do not fit the record (3 n^2; nearly degenerate
// 100 x 100 spectra take 0.8 n^2) is flagged and redone by the apply kernel with the chain and the rows together.
// Reduction and accumulation for the three-kernel form, 256 threads: a dot product is the work of an OCT of lanes -- lane c runs chain
// c of QL_DOT8 (terms k = c, c + 8, ...), the butterfly xor 4, xor 2, xor 1 is the oracle's ((s0 + s4) + (s2 + s6)) + ((s1 + s5) +
// (s3 + s7)) in every lane -- 32 products at a time; the rank-two update and the column updates are 16 x 16 tilings of their
// elements.  (A thread per row with the eight chains side by side left the threads of short rows idle and every wave alone on its
// SIMD: 17 000 cycles per row of the reduction.)
#ifndef PTMI_QLR_THREADS
#define PTMI_QLR_THREADS 512
#endif
constexpr int QLR_THREADS = PTMI_QLR_THREADS, QLR_TY = QLR_THREADS / 16;
__global__ __launch_bounds__(QLR_THREADS) void eig_ql_reduce_kernel(const double *cov, int n, QlScratch q)
{
    extern __shared__ __attribute__((aligned(16))) double qsm[];
    double *z = qsm, *e = qsm + (((size_t)n * n + 1) & ~(size_t)1), *pq = e + n;
    const int t = (int)threadIdx.x;
    const int oct = t >> 3, c8 = t & 7, ty = t >> 4, tx = t & 15;
    const double *A = cov + (size_t)blockIdx.x * n * n;
#define QZ(i, j) z[(i) * n + (j)]
    for (int i = t; i < n * n; i += QLR_THREADS) z[i] = A[i];
    unsigned long long hmask[2] = {0ull, 0ull};
    __syncthreads();
    for (int i = n - 1; i >= 1; --i) {
        const int l = i - 1;
        double h = 0.0;
        if (l > 0) {
            double sc = 0.0;
            for (int k = c8; k <= l; k += 8) { const double v = QZ(i, k); sc = __builtin_fma(v, v, sc); }
            h = jac_oct_sum(sc);
        }
        if (l == 0 || h == 0.0) {                                 // uniform
            if (t == 0) e[i] = QZ(i, l);
            __syncthreads();
            continue;
        }
        const double f0 = QZ(i, l);
        const double g0 = f0 >= 0.0 ? -det_sqrt(h) : det_sqrt(h);
        h = h - f0 * g0;
        __syncthreads();                                          // every thread has read Z(i, l)
        if (t == 0) { e[i] = g0; QZ(i, l) = f0 - g0; }
        __syncthreads();
        for (int j = oct; j <= l; j += QLR_THREADS / 8) {
            double sc = 0.0;
            for (int k = c8; k <= l; k += 8) sc = __builtin_fma(k <= j ? QZ(j, k) : QZ(k, j), QZ(i, k), sc);
            const double g = jac_oct_sum(sc);
            // the two quotients of row j by two lanes of its oct: one division sequence instead of two on the critical path
            const double quo = (c8 == 0 ? g : QZ(i, j)) / h;
            if (c8 == 0) pq[j] = quo;
            else if (c8 == 1) QZ(j, i) = quo;
        }
        __syncthreads();
        double fc = 0.0;
        for (int k = c8; k <= l; k += 8) fc = __builtin_fma(pq[k], QZ(i, k), fc);
        const double f = jac_oct_sum(fc);
        const double hh = f / (h + h);
        __syncthreads();                                          // every thread has its f
        for (int j = t; j <= l; j += QLR_THREADS) pq[j] = pq[j] - hh * QZ(i, j);
        __syncthreads();
        for (int j = ty; j <= l; j += QLR_TY) {
            const double uj = QZ(i, j), qj = pq[j];
            for (int k = tx; k <= j; k += 16) QZ(j, k) = QZ(j, k) - (uj * pq[k] + qj * QZ(i, k));
        }
        hmask[i >> 6] |= 1ull << (i & 63);
        __syncthreads();
    }
    if (t == 0) e[0] = 0.0;
    for (int i = 0; i < n; ++i) {
        const int l = i - 1;
        if ((hmask[i >> 6] >> (i & 63)) & 1ull) {                  // uniform
            // the products g_j of the leading block's columns with row i; row i is dead afterwards (zeroed below) and keeps them
            double gj[4] = {0.0, 0.0, 0.0, 0.0};
            int nj = 0;
            for (int j = oct; j <= l; j += QLR_THREADS / 8, ++nj) {
                double sc = 0.0;
                for (int k = c8; k <= l; k += 8) sc = __builtin_fma(QZ(i, k), QZ(k, j), sc);
                gj[nj & 3] = jac_oct_sum(sc);
            }
            __syncthreads();                                      // every product has read row i
            nj = 0;
            for (int j = oct; j <= l; j += QLR_THREADS / 8, ++nj)
                if (c8 == 0) QZ(i, j) = gj[nj & 3];
            __syncthreads();
            for (int k = ty; k <= l; k += QLR_TY) {
                const double zki = QZ(k, i);
                for (int j = tx; j <= l; j += 16) QZ(k, j) = QZ(k, j) - QZ(i, j) * zki;
            }
        }
        __syncthreads();
        if (t == 0) { pq[i] = QZ(i, i); QZ(i, i) = 1.0; }
        for (int j = t; j <= l; j += QLR_THREADS) { QZ(j, i) = 0.0; QZ(i, j) = 0.0; }
        __syncthreads();
    }
#undef QZ
    double *zo = q.z + (size_t)blockIdx.x * n * n;
    for (int i = t; i < n * n; i += QLR_THREADS) zo[i] = z[i];
    qls_d2 *deo = q.de + (size_t)blockIdx.x * n;
    for (int i = t; i < n; i += QLR_THREADS) deo[i] = qls_d2{pq[i], i + 1 < n ? e[i + 1] : 0.0};
}

// (the QL iterations themselves, ql_iterate, are in ptmi_eig_ql.h: the wide unit's redo runs them on rows in global memory)
__global__ __launch_bounds__(64) void eig_ql_chain_kernel(int n, QlScratch q)
{
    extern __shared__ __attribute__((aligned(16))) double qsm[];
    qls_d2 *de = reinterpret_cast<qls_d2 *>(qsm);
    const int t = (int)threadIdx.x;
    const size_t b = blockIdx.x;
    for (int i = t; i < n; i += 64) de[i] = q.de[b * n + i];
    asm volatile("" ::: "memory");
    int over = 0;
    const int iters = ql_iterate<false>(de, n, t, nullptr, q.rot + b * (size_t)q.cap, q.hdr + b * 2 * (size_t)q.capit, q.cap, q.capit, &over);
    asm volatile("" ::: "memory");
    for (int i = t; i < n; i += 64) q.ev[b * n + i] = de[i].x;
    if (t == 0) { q.cnt[2 * b] = iters < 0 ? 0 : iters; q.cnt[2 * b + 1] = (over || iters < 0) ? 1 : 0; }
}

__global__ __launch_bounds__(QL_THREADS) void eig_ql_apply_kernel(double *Ut, double *S, int n, int ut_stride, int s_stride, QlScratch q, int redo_only)
{
    if (redo_only && q.cnt[2 * blockIdx.x + 1] == 0) return;      // eig_ql_apply_reg_kernel has done this matrix

    extern __shared__ __attribute__((aligned(16))) double qsm[];
    double *zt = qsm;                                              // zt[c n + k] = Z(k, c)
    qls_d2 *de = reinterpret_cast<qls_d2 *>(qsm + (((size_t)n * n + 1) & ~(size_t)1));
    const int t = (int)threadIdx.x;
    const size_t b = blockIdx.x;
    const double *zi = q.z + b * n * n;
    for (int i = t; i < n * n; i += QL_THREADS) { const int r = i / n, c = i % n; zt[c * n + r] = zi[i]; }
    const bool redo = q.cnt[2 * b + 1] != 0;                       // the record did not hold this matrix's rotations
    if (redo) {
        for (int i = t; i < n; i += QL_THREADS) de[i] = q.de[b * n + i];
        __syncthreads();
        if (t < 64) ql_iterate<true>(de, n, t, zt, nullptr, nullptr, 0, 0, nullptr);
    } else {
        // A thread per row.  The rotations of ONE iteration (at most n - 1 of them) are staged in LDS -- the pairs' 2 n doubles,
        // free until the eigenvalues go there -- by all threads at once, the next iteration's requested before this one's are
        // applied (a read of the record per rotation sat on every row's chain with its whole memory round trip: 300 cycles per
        // rotation).  Of the two columns a rotation turns, the lower one is the next rotation's upper one and stays in a register.
        const int nit = q.cnt[2 * b];
        const int32_t *hdr = q.hdr + b * 2 * (size_t)q.capit;
        const qls_d2 *rot = q.rot + b * (size_t)q.cap;
        int r = 0;
        int l = nit > 0 ? hdr[0] : 0, m = nit > 0 ? hdr[1] : 0;
        int ln = nit > 1 ? hdr[2] : 0, mn = nit > 1 ? hdr[3] : 0;  // the (l, m) of the iteration after: known two iterations ahead
        qls_d2 mine = (nit > 0 && t < m - l) ? rot[t] : qls_d2{0.0, 0.0};
        for (int itn = 0; itn < nit; ++itn) {
            const int cntr = m - l;
            __syncthreads();                                        // the previous iteration's rotations have been applied
            if (t < cntr) de[t] = mine;
            __syncthreads();
            r += cntr;
            const int lnn = itn + 2 < nit ? hdr[2 * itn + 4] : 0, mnn = itn + 2 < nit ? hdr[2 * itn + 5] : 0;
            if (itn + 1 < nit && t < mn - ln) mine = rot[r + t];
            if (t < n) {
                double zb = zt[m * n + t];
                const double *zp = zt + (size_t)(m - 1) * n + t;    // column i of this thread's row, i descending
                int j = 0;
                for (; j + 4 <= cntr; j += 4, zp -= 4 * n) {       // four rotations a trip: their reads go out together
                    const qls_d2 c0 = de[j], c1 = de[j + 1], c2 = de[j + 2], c3 = de[j + 3];
                    const double a0 = zp[0], a1 = zp[-n], a2 = zp[-2 * n], a3 = zp[-3 * n];
                    const_cast<double *>(zp)[n] = c0.y * a0 + c0.x * zb;
                    zb = c0.x * a0 - c0.y * zb;
                    const_cast<double *>(zp)[0] = c1.y * a1 + c1.x * zb;
                    zb = c1.x * a1 - c1.y * zb;
                    const_cast<double *>(zp)[-n] = c2.y * a2 + c2.x * zb;
                    zb = c2.x * a2 - c2.y * zb;
                    const_cast<double *>(zp)[-2 * n] = c3.y * a3 + c3.x * zb;
                    zb = c3.x * a3 - c3.y * zb;
                }
                for (; j < cntr; ++j, zp -= n) {
                    const qls_d2 cs = de[j];
                    const double za = zp[0];
                    const_cast<double *>(zp)[n] = cs.y * za + cs.x * zb;
                    zb = cs.x * za - cs.y * zb;
                }
                zt[l * n + t] = zb;
            }
            l = ln; m = mn;
            ln = lnn; mn = mnn;
        }
        __syncthreads();
        for (int i = t; i < n; i += QL_THREADS) de[i] = qls_d2{q.ev[b * n + i], 0.0};
    }
    __syncthreads();
    double *Uo = Ut + b * ut_stride, *So = S + b * s_stride;
    for (int k = t; k < n; k += QL_THREADS) {
        const double mine = __builtin_fabs(de[k].x);
        int rank = 0;
        for (int j = 0; j < n; ++j) { const double o = __builtin_fabs(de[j].x); rank += (o > mine) || (o == mine && j < k); }
        const double *col = zt + (size_t)k * n;                    // Z(i, k), i = 0 .. n - 1
        int im = 0;
        for (int i = 1; i < n; ++i) if (__builtin_fabs(col[i]) > __builtin_fabs(col[im])) im = i;
        const double sg = col[im] < 0.0 ? -1.0 : 1.0;
        for (int i = 0; i < n; ++i) Uo[(size_t)rank * n + i] = sg * col[i];
        So[rank] = mine;
    }
}

// The apply step with the eigenvector matrix in REGISTERS (n <= 100): thread t holds row t of Z, z[0 .. n - 1], and a rotation of
// columns (i, i + 1) is six instructions on two registers of every thread -- the record's (c, s) and the iterations' (l, m) are the
// same for all rows: uniform branches, (c, s) an LDS broadcast staged by each wave for itself; no barrier until the end, four matrices (eight waves)
// per CU instead of the two that fit with Z in LDS.  Register indices are compile-time: an iteration's sweep i = m - 1 ... l is the
// unrolled sweep 98 ... 0 entered block by block (QLA_BLK = 8 steps, 2.29 ms against 2.41 with 4; a block outside [l, m) is one uniform branch, a block inside it
// runs without tests).  eig_ql_apply_kernel: 4.15 ms per epoch at 4096 x 100 x 100 (a wave per SIMD, an LDS round trip on every
// row's chain per four rotations).  Matrices whose record overflowed are left to that kernel (redo_only).
#ifndef PTMI_QLA_BLK
#define PTMI_QLA_BLK 8
#endif
constexpr int QLA_N = 100, QLA_BLK = PTMI_QLA_BLK;
template <int LO, int HI, bool CHECK>
__device__ __forceinline__ void qla_steps(double (&z)[QLA_N], const qls_d2 *cs_of_step, int l, int m)
{
#pragma unroll
    for (int i = HI; i >= LO; --i) {
        if (!CHECK || (i >= l && i < m)) {
            const qls_d2 cs = cs_of_step[i];                        // {c, s}: an LDS broadcast at a compile-time offset
            const double za = z[i], zb = z[i + 1];
            z[i + 1] = cs.y * za + cs.x * zb;
            z[i] = cs.x * za - cs.y * zb;
        }
    }
}
template <int BLKI>
__device__ __forceinline__ void qla_sweep(double (&z)[QLA_N], const qls_d2 *cs_of_step, int l, int m)
{
    constexpr int LO = QLA_BLK * BLKI, HI = LO + QLA_BLK - 1 < QLA_N - 2 ? LO + QLA_BLK - 1 : QLA_N - 2;
    if (HI >= l && LO < m) {
        if (LO >= l && HI < m) qla_steps<LO, HI, false>(z, cs_of_step, l, m);
        else qla_steps<LO, HI, true>(z, cs_of_step, l, m);
    }
    if constexpr (BLKI > 0) qla_sweep<BLKI - 1>(z, cs_of_step, l, m);
}
__global__ __launch_bounds__(128, 2) void eig_ql_apply_reg_kernel(double *Ut, double *S, int n, int ut_stride, int s_stride,
                                                                  const double *__restrict__ zin, const double *__restrict__ evin,
                                                                  const qls_d2 *__restrict__ rot_all, const int32_t *__restrict__ hdr_all,
                                                                  const int32_t *__restrict__ cnt, int cap, int capit)
{
    __shared__ double wmax[2][QLA_N], wsv[2][QLA_N], sgs[QLA_N];
    __shared__ int rk[QLA_N];
    // an iteration's rotations, staged by each wave for itself (no barrier): slot i = the rotation of step i; the next iteration's
    // are requested before this one's sweep and stored behind it (a scalar load per block of the sweep waited 600 cycles each)
    __shared__ __attribute__((aligned(16))) qls_d2 stg[2][2][QLA_N];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t b = blockIdx.x;
    if (cnt[2 * b + 1] != 0) return;                                // the record did not hold this matrix's rotations
    const bool rowok = t < n;
    double z[QLA_N];
    {
        const double *zi = zin + b * n * n + (size_t)(rowok ? t : 0) * n;
#pragma unroll
        for (int c = 0; c < QLA_N; ++c) z[c] = c < n ? zi[c] : 0.0;
    }
    const int nit = cnt[2 * b];
    const int32_t *hdr = hdr_all + b * 2 * (size_t)capit;
    const qls_d2 *rot = rot_all + b * (size_t)cap;
    int l = nit > 0 ? hdr[0] : 0, m = nit > 0 ? hdr[1] : 0;
    int ln = nit > 1 ? hdr[2] : 0, mn = nit > 1 ? hdr[3] : 0;      // the (l, m) of the iteration after: known two iterations ahead
    int r = 0;
    {
        const int cn = m - l;
        if (lane < cn) stg[wave][0][m - 1 - lane] = rot[lane];
        if (lane + 64 < cn) stg[wave][0][m - 1 - lane - 64] = rot[lane + 64];
    }
    for (int itn = 0; itn < nit; ++itn) {
        r += m - l;
        const int lnn = itn + 2 < nit ? hdr[2 * itn + 4] : 0, mnn = itn + 2 < nit ? hdr[2 * itn + 5] : 0;
        const int cn = itn + 1 < nit ? mn - ln : 0;
        qls_d2 nx0 = qls_d2{0.0, 0.0}, nx1 = qls_d2{0.0, 0.0};
        if (lane < cn) nx0 = rot[r + lane];
        if (lane + 64 < cn) nx1 = rot[r + lane + 64];
        __builtin_amdgcn_wave_barrier();
        qla_sweep<(QLA_N - 2) / QLA_BLK>(z, stg[wave][itn & 1], l, m);
        __builtin_amdgcn_wave_barrier();
        if (lane < cn) stg[wave][(itn + 1) & 1][mn - 1 - lane] = nx0;
        if (lane + 64 < cn) stg[wave][(itn + 1) & 1][mn - 1 - lane - 64] = nx1;
        l = ln; m = mn;
        ln = lnn; mn = mnn;
    }
    // the sign of every eigenvector: its first component of largest magnitude becomes positive (row ascending, strict >)
#pragma unroll
    for (int k = 0; k < QLA_N; ++k) {
        if (k < n) {
            const double a = rowok ? __builtin_fabs(z[k]) : -1.0;
            double mx = a;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) { const double ot = __shfl_xor(mx, o, 64); mx = ot > mx ? ot : mx; }
            const unsigned long long eq = __ballot(a == mx);
            const int first = __builtin_ctzll(eq);
            const double sv = __shfl(z[k], first, 64);
            if (lane == 0) { wmax[wave][k] = mx; wsv[wave][k] = sv; }
        }
    }
    __syncthreads();
    if (rowok) {
        const int k = t;
        const double sv = wmax[1][k] > wmax[0][k] ? wsv[1][k] : wsv[0][k];
        sgs[k] = sv < 0.0 ? -1.0 : 1.0;
        const double *ev = evin + b * n;
        const double mine = __builtin_fabs(ev[k]);
        int rank = 0;
        for (int j = 0; j < n; ++j) { const double o = __builtin_fabs(ev[j]); rank += (o > mine) || (o == mine && j < k); }
        rk[k] = rank;
        S[b * s_stride + rank] = mine;
    }
    __syncthreads();
    double *Uo = Ut + b * ut_stride;
#pragma unroll
    for (int k = 0; k < QLA_N; ++k) {
        if (k < n && rowok) Uo[(size_t)rk[k] * n + t] = sgs[k] * z[k];
    }
}

void eig_ql_chain_launch(hipStream_t stream, int n, int nmat, const QlScratch &q)
{
    hipLaunchKernelGGL(eig_ql_chain_kernel, dim3(nmat), dim3(64), sizeof(double) * 2 * (size_t)n, stream, n, q);
}

// (the kernels from here to the divide-and-conquer solver's have C names)
extern "C" {

// nmat symmetric matrices of order n, packed [nmat][n][n] -> eigenvectors as rows [nmat][n][n], eigenvalues [nmat][n] (see ptmi_eig_ql)
static int eig_ql_run(ptmi_engine *h, int n, int nmat, const double *cov, double *Ut, double *S)
{
    const ptmi_config &c = h->cfg;
    const int d = n, dmax = c.ndim < 128 ? c.ndim : 128;               // (the scratch below: a matrix beyond 128 goes to the wide kernels)
    if (d > 1024) return fail(PTMI_EUNSUPPORTED, "the QL eigensolver factorizes matrices up to 1024 x 1024 (this one: %d x %d)", d, d);
    if (d > 128) return eig_ql_wide_run(h, d, nmat, cov, Ut, S);     // the matrix in a global scratch (ptmi_eig_wide.hip)
    const size_t lds = sizeof(double) * ((((size_t)d * d + 1) & ~(size_t)1) + 2 * (size_t)d);
    const bool split = ptmi_env("PTMI_QL_SPLIT", nmat >= 64) != 0;    // 1 / 0 forces the three-kernel / the one-kernel form (a test hook)
    if (split) {
        // many matrices: reduce -> the scalar chains of all of them at once -> apply (see eig_ql_chain_kernel)
        const int cap = 3 * d * d, capit = 8 * d;
        if (!h->d_ql_scr) {                                             // sized for the full order (a parameter group's matrices are smaller)
            const int capm = 3 * dmax * dmax, capitm = 8 * dmax;
            const size_t bytes = sizeof(double) * (size_t)nmat * ((size_t)dmax * dmax + 2 * (size_t)dmax + (size_t)dmax + 2 * (size_t)capm) +
                                 sizeof(int32_t) * (size_t)nmat * (2 * (size_t)capitm + 2) + 256;
            HIPCHK(hipMalloc((void **)&h->d_ql_scr, bytes));
        }
        QlScratch q;
        char *pb = (char *)h->d_ql_scr;
        auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
        q.z = (double *)pb; pb += up16(sizeof(double) * (size_t)nmat * d * d);
        q.de = (qls_d2 *)pb; pb += sizeof(double) * 2 * (size_t)nmat * d;
        q.rot = (qls_d2 *)pb; pb += sizeof(double) * 2 * (size_t)nmat * cap;
        q.ev = (double *)pb; pb += up16(sizeof(double) * (size_t)nmat * d);
        q.hdr = (int32_t *)pb; pb += sizeof(int32_t) * 2 * (size_t)nmat * capit;
        q.cnt = (int32_t *)pb;
        q.cap = cap; q.capit = capit;
        if (lds > 64 * 1024) {
            HIPCHK(hipFuncSetAttribute((const void *)eig_ql_reduce_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            HIPCHK(hipFuncSetAttribute((const void *)eig_ql_apply_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        }
        hipLaunchKernelGGL(eig_ql_reduce_kernel, dim3(nmat), dim3(QLR_THREADS), lds, h->stream, cov, d, q);
        eig_ql_chain_launch(h->stream, d, nmat, q);
        const bool regs = d <= QLA_N;
        if (regs)
            hipLaunchKernelGGL(eig_ql_apply_reg_kernel, dim3(nmat), dim3(128), 0, h->stream, Ut, S, d, d * d, d, (const double *)q.z,
                               (const double *)q.ev, (const qls_d2 *)q.rot, (const int32_t *)q.hdr, (const int32_t *)q.cnt, cap, capit);
        hipLaunchKernelGGL(eig_ql_apply_kernel, dim3(nmat), dim3(QL_THREADS), lds, h->stream, Ut, S, d, d * d, d, q, regs ? 1 : 0);
        HIPCHK(hipGetLastError());
        return PTMI_OK;
    }
    if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)eig_ql_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(eig_ql_kernel, dim3(nmat), dim3(QL_THREADS), lds, h->stream, cov, Ut, S, d, d * d, d, (int32_t *)nullptr);
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

// Parameter groups (PT:129-145, 797-803: one SVD per group's block of the covariance): the group's rows and columns, in ascending
// parameter order, packed into an m x m matrix per walker ...
__global__ __launch_bounds__(256) void group_gather_kernel(const double *cov, const double *gmask, int d, int m, double *sub)
{
    __shared__ int idx[1024];
    const double *mk = gmask;                                            // [d] membership of this group
    if (threadIdx.x == 0) {
        int k = 0;
        for (int i = 0; i < d && k < 1024; ++i) if (mk[i] != 0.0) idx[k++] = i;
    }
    __syncthreads();
    const double *cw = cov + (size_t)blockIdx.x * d * d;
    double *sw = sub + (size_t)blockIdx.x * m * m;
    for (int t = (int)threadIdx.x; t < m * m; t += 256) sw[t] = cw[(size_t)idx[t / m] * d + idx[t % m]];
}
// ... and its eigenvectors embedded in the full space, one per row of the group's table (zero outside the group, zero rows beyond
// the group's size), the eigenvalues padded with zeros: the layout propose() reads (Ut[Wc][Ng][d][d], S[Wc][Ng][d])
__global__ __launch_bounds__(256) void group_embed_kernel(const double *usub, const double *ssub, const double *gmask, int d, int m, int ng, int gi,
                                                          double *Ut, double *S)
{
    __shared__ int pos[1024];                                            // position of parameter i inside the group, or -1
    if (threadIdx.x == 0) {
        int k = 0;
        for (int i = 0; i < d; ++i) pos[i] = gmask[i] != 0.0 ? k++ : -1;
    }
    __syncthreads();
    const double *uw = usub + (size_t)blockIdx.x * m * m, *sw = ssub + (size_t)blockIdx.x * m;
    double *Uo = Ut + ((size_t)blockIdx.x * ng + gi) * d * d, *So = S + ((size_t)blockIdx.x * ng + gi) * d;
    for (int t = (int)threadIdx.x; t < d * d; t += 256) {
        const int k = t / d, i = t % d;
        Uo[t] = (k < m && pos[i] >= 0) ? uw[(size_t)k * m + pos[i]] : 0.0;
    }
    for (int k = (int)threadIdx.x; k < d; k += 256) So[k] = k < m ? sw[k] : 0.0;
}

int ptmi_eig_ql(ptmi_handle h)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    const ptmi_config &c = h->cfg;
    if (!h->buf.cov || !h->buf.Ut || !h->buf.S) return fail(PTMI_EINVAL, "cov / Ut / S buffers missing");
    const int d = c.ndim, nmat = c.cov_per_walker ? c.nwalkers : 1;
    if (c.ngroups <= 1) return eig_ql_run(h, d, nmat, (const double *)h->buf.cov, h->buf.Ut, h->buf.S);
    if (d > 1024) return fail(PTMI_EUNSUPPORTED, "the QL eigensolver with parameter groups: ndim <= 1024 (got %d)", d);
    // one factorization per parameter group, as the reference's loop over self.groups (PT:797-803)
    if (!h->d_qlg_scr) HIPCHK(hipMalloc((void **)&h->d_qlg_scr, sizeof(double) * (size_t)nmat * (2 * (size_t)d * d + d)));
    double *sub = (double *)h->d_qlg_scr, *usub = sub + (size_t)nmat * d * d, *ssub = usub + (size_t)nmat * d * d;
    for (int gi = 0; gi < c.ngroups; ++gi) {
        const int m = h->gsize_host[gi];
        const double *mk = h->d_gmask + (size_t)gi * d;
        hipLaunchKernelGGL(group_gather_kernel, dim3(nmat), dim3(256), 0, h->stream, (const double *)h->buf.cov, mk, d, m, sub);
        if (int rc = eig_ql_run(h, m, nmat, (const double *)sub, usub, ssub)) return rc;
        hipLaunchKernelGGL(group_embed_kernel, dim3(nmat), dim3(256), 0, h->stream, (const double *)usub, (const double *)ssub, mk, d, m, c.ngroups, gi,
                           h->buf.Ut, h->buf.S);
    }
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

// ptmi_eig_ql on the caller's stream, from / into the caller's buffers: the engine's eig_lag with per-walker covariances -- the
// factorization of thousands of small matrices (chains of dependent rotations: little of the GPU each) runs BESIDE the step launches of
// the next covariance period instead of between two of them.  One call at a time (the scratch is the handle's).
int ptmi_eig_ql_from(ptmi_handle h, void *stream, const double *cov_in, double *Ut_out, double *S_out)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    const ptmi_config &c = h->cfg;
    const double *cov = cov_in ? cov_in : (const double *)h->buf.cov;
    double *Uo = Ut_out ? Ut_out : h->buf.Ut, *So = S_out ? S_out : h->buf.S;
    if (!cov || !Uo || !So) return fail(PTMI_EINVAL, "cov / Ut / S buffers missing");
    if (c.ngroups > 1) return fail(PTMI_EUNSUPPORTED, "ptmi_eig_ql_from: one parameter group (use ptmi_eig_ql)");
    ptmi_engine view = *h;                                               // eig_ql_run reads the stream, the configuration and the scratch pointer
    if (stream) view.stream = (hipStream_t)stream;
    const int rc = eig_ql_run(&view, c.ndim, c.cov_per_walker ? c.nwalkers : 1, cov, Uo, So);
    h->d_ql_scr = view.d_ql_scr;                                         // (made by the first call)
    h->d_qlw_scr = view.d_qlw_scr;
    h->qlw_scr_bytes = view.qlw_scr_bytes;
    return rc;
}

// ---------------------------------------------------------------- one large matrix: tridiagonalization in one kernel
// eig_mode "sytrd" (ptmi_eig_sytrd; ndim <= 1024, one pooled covariance).  The ROCm library's symmetric eigensolver spends two thirds
// of its time reducing the matrix to tridiagonal form in some 7000 launches of one-block kernels (1000 x 1000: 25 of 35 ms of kernel
// time, 3 us each).  Here that step is ONE kernel: the matrix lives in the LDS of its blocks (block b owns the full columns
// b, b + NB, ...: 64 KB of 160 at 1000 x 1000 over 128 blocks), a Householder step is
//   the owner of column k forms v (its own LDS)                                         -> v to all      [grid barrier]
//   every block: p_j = tau (column j . v) for ITS columns (A symmetric: column j is row j)  -> p to all      [grid barrier]
//   every block: w = p - (tau/2 p.v) v, its columns -= v w_j + w v_j
// -- no reduction across blocks, two barriers per column (a few microseconds each on an atomic counter).  Output in LAPACK's
// dsytrd format (uplo = lower: d, e, tau, the reflectors below the subdiagonal), from which the divide-and-conquer solver for the
// tridiagonal matrix and its back-transformation through the reflectors (dc_solve) take it.
struct SytrdArgs {
    double *A;             // [n][n] column-major = row-major (symmetric in); out: the reflectors
    double *D, *E, *tau;   // [n], [n - 1], [n - 1]
    double *vbuf;          // [2][n + 2]: column m as its owner holds it before the update (by parity of m)
    double *pbuf;          // [2][n]: the products p_j (by parity of m)
    unsigned *bar;
    int n;
};
#ifndef PTMI_SY_THREADS
#define PTMI_SY_THREADS 256
#endif
constexpr int SY_THREADS = PTMI_SY_THREADS, SY_NW = SY_THREADS / 64, SY_CMAX = 16, SY_PT = 1024 / SY_THREADS;       // SY_PT: elements of a vector per thread (n <= 1024)
// exchanged data goes through agent-scope relaxed atomics (write-through stores, loads past the caches of the other XCDs): no
// cache write-back / invalidation beside the barrier's own counter
__device__ __forceinline__ void sy_grid_sync(unsigned *bar, unsigned &target, unsigned nb)
{
    // every thread's exchanged stores must be ACKNOWLEDGED before the counter moves.  __syncthreads alone does not wait for them (a
    // workgroup-scope release needs no vmcnt wait on this part: the CU's L1 is the block's own), and the counter's increment is
    // relaxed: beside an idle GPU the stores happened to land first; beside step launches that saturate the L2 / MALL path (the wide
    // kernels of round 5) another block could pass the barrier and read a vector's old contents -- whole runs differed from
    // repeat to repeat (tools/repeat_check.py).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#ifdef PTMI_SY_NOBAR
    return;
#endif
    if (threadIdx.x == 0) {
        target += nb;
        // RELAXED: a release / acquire at agent scope writes back / invalidates the XCD's whole L2 at every barrier -- under the step
        // kernel running beside this one (its table rows live there): launches of 3.2 ms instead of 2.5.  The exchanged vectors
        // need neither: they are written and read with agent-scope atomics themselves, and __syncthreads has waited for the stores.
        __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifndef PTMI_SY_SLEEP
#define PTMI_SY_SLEEP 8
#endif
        while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) __builtin_amdgcn_s_sleep(PTMI_SY_SLEEP);
    }
    __syncthreads();
}
__device__ __forceinline__ double sy_load(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void sy_store(double *p, double x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// elements lo .. n - 1 of an exchanged vector into LDS: every load of a thread in flight at once
__device__ __forceinline__ void sy_fetch(const double *src, double *dst, int lo, int n)
{
    double tmp[SY_PT];
#pragma unroll
    for (int u = 0; u < SY_PT; ++u) { const int i = lo + (int)threadIdx.x + u * SY_THREADS; tmp[u] = i < n ? sy_load(src + i) : 0.0; }
#pragma unroll
    for (int u = 0; u < SY_PT; ++u) { const int i = lo + (int)threadIdx.x + u * SY_THREADS; if (i < n) dst[i] = tmp[u]; }
}
__device__ __forceinline__ double sy_block_sum(double x, double *red)      // red: [SY_NW] doubles of LDS
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < SY_THREADS / 64; ++w) s += red[w];
    return s;
}
// 256 threads and at most 64 registers: a wave per SIMD that fits beside FOUR waves of the config-4 step kernel (112 registers each);
// with 512 threads of 72 registers the step kernel lost a wave per SIMD on every CU that holds a block of this one (launches 3.1 ms
// against 2.5)
__global__ __launch_bounds__(SY_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void sytrd_lds_kernel(SytrdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double sy[];
    const int n = a.n, nb = (int)gridDim.x, b = (int)blockIdx.x, t = (int)threadIdx.x;
    const int ncol = b < n ? (n - 1 - b) / nb + 1 : 0;               // owned columns b, b + nb, ...
    double *col = sy;                                                // [ncol][n]
    double *v = sy + (size_t)SY_CMAX * n, *w = v + n, *xr = w + n, *red = xr + n;    // [n] each, [1 + SY_CMAX][SY_NW]
    unsigned target = 0;
    for (int c = 0; c < ncol; ++c)
        for (int i = t; i < n; i += SY_THREADS) col[(size_t)c * n + i] = a.A[(size_t)(b + c * nb) * n + i];
    for (int i = t; i < n; i += SY_THREADS) { v[i] = 0.0; w[i] = 0.0; }
    double tau = 0.0;                                                // of the reflector in v (m - 1)
    __syncthreads();
    // Iteration m: the update by reflector m - 1 (in v, known to every block) and the generation of reflector m, with ONE grid
    // barrier: beside its p_j every block would need column m after the update to form the next reflector -- the column's owner
    // sends it as it is BEFORE the update, and every block applies the update to its copy and forms v_m for itself (the same
    // operations on the same values in every block).
    for (int m = 0; m + 1 < n; ++m) {
        const int par = m & 1;
        double *pb = a.pbuf + (size_t)par * n, *rb = a.vbuf + (size_t)par * (n + 2);
        const int c0 = m <= b ? 0 : (m - b + nb - 1) / nb;             // this block's columns j >= m: those from c0 on
        if (m >= 1 && tau != 0.0) {
            // a wave per column (columns wave, wave + SY_NW, ...: SY_CMAX / SY_NW accumulators per lane, reduced inside the wave,
            // no barrier): with every thread on every column the 16 accumulators' 96 shuffle steps, an LDS exchange between the
            // waves and a barrier made this the longest part of a step (9 of 12.5 us)
            constexpr int CW = SY_CMAX / SY_NW;
            const int wv = t >> 6, ln = t & 63;
            double acc[CW];
#pragma unroll
            for (int q = 0; q < CW; ++q) acc[q] = 0.0;
            for (int i = m + ln; i < n; i += 64) {
                const double vi = v[i];
#pragma unroll
                for (int q = 0; q < CW; ++q) {
                    const int c = wv + q * SY_NW;
                    if (c >= c0 && c < ncol) acc[q] = __builtin_fma(col[(size_t)c * n + i], vi, acc[q]);
                }
            }
#pragma unroll
            for (int q = 0; q < CW; ++q) {
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) acc[q] += __shfl_xor(acc[q], o, 64);
                const int c = wv + q * SY_NW;
                if (ln == 0 && c >= c0 && c < ncol) sy_store(pb + b + c * nb, tau * acc[q]);
            }
        }
        if (b == m % nb) {
            const double *x = col + (size_t)(m / nb) * n;
            for (int i = m + 1 + t; i < n; i += SY_THREADS) sy_store(rb + i, x[i]);
        }
        sy_grid_sync(a.bar, target, (unsigned)nb);
        if (m >= 1 && tau != 0.0) {
            // both vectors' loads in flight at once (a round trip to memory each)
            double tx[SY_PT], tp[SY_PT];
#pragma unroll
            for (int u = 0; u < SY_PT; ++u) {
                const int i = m + t + u * SY_THREADS;
                tx[u] = (i > m && i < n) ? sy_load(rb + i) : 0.0;
                tp[u] = i < n ? sy_load(pb + i) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < SY_PT; ++u) {
                const int i = m + t + u * SY_THREADS;
                if (i > m && i < n) xr[i] = tx[u];
                if (i < n) w[i] = tp[u];
            }
            __syncthreads();
            double pv = 0.0;
            for (int i = m + t; i < n; i += SY_THREADS) pv = __builtin_fma(w[i], v[i], pv);
            const double ptv = sy_block_sum(pv, red);
            const double al = -0.5 * tau * ptv;
            for (int i = m + t; i < n; i += SY_THREADS) w[i] = __builtin_fma(al, v[i], w[i]);
            __syncthreads();
            for (int c = c0; c < ncol; ++c) {
                const int j = b + c * nb;
                const double vj = v[j], wj = w[j];
                double *cj = col + (size_t)c * n;
                for (int i = m + t; i < n; i += SY_THREADS) cj[i] -= v[i] * wj + w[i] * vj;
            }
            const double vm = v[m], wm = w[m];
            for (int i = m + 1 + t; i < n; i += SY_THREADS) xr[i] -= v[i] * wm + w[i] * vm;       // column m as its owner now has it
        } else {
            sy_fetch(rb, xr, m + 1, n);
        }
        __syncthreads();
        // reflector m from xr[m + 1 .. n - 1] (dlarfg)
        double ss = 0.0;
        for (int i = m + 2 + t; i < n; i += SY_THREADS) ss = __builtin_fma(xr[i], xr[i], ss);
        const double xn2 = sy_block_sum(ss, red);
        const double alpha = xr[m + 1];
        double beta = alpha, scal = 0.0;
        tau = 0.0;
        if (xn2 != 0.0) {
            const double nrm = det_sqrt(alpha * alpha + xn2);
            beta = alpha >= 0.0 ? -nrm : nrm;
            tau = (beta - alpha) / beta;
            scal = 1.0 / (alpha - beta);
        }
        __syncthreads();                                              // every thread has read alpha
        for (int i = m + 2 + t; i < n; i += SY_THREADS) v[i] = xr[i] * scal;
        if (t == 0) v[m + 1] = 1.0;
        if (b == m % nb) {
            for (int i = m + 2 + t; i < n; i += SY_THREADS) a.A[(size_t)m * n + i] = xr[i] * scal;      // LAPACK's storage of reflector m
            if (t == 0) {
                a.D[m] = col[(size_t)(m / nb) * n + m];
                a.E[m] = beta;
                a.tau[m] = tau;
            }
        }
        __syncthreads();
    }
    if ((n - 1) % nb == b && t == 0) a.D[n - 1] = col[(size_t)((n - 1) / nb) * n + (n - 1)];
}
// eigenvalues ascending (the library's order) -> by decreasing size in absolute value, the eigenvectors (rows of C) along
__global__ __launch_bounds__(256) void eig_sort_rows_kernel(const double *D, const double *Cm, int n, double *Ut, double *S)
{
    __shared__ int rank_s;
    const int k = (int)blockIdx.x;
    if (threadIdx.x == 0) {
        const double mine = __builtin_fabs(D[k]);
        int rank = 0;
        for (int j = 0; j < n; ++j) { const double o = __builtin_fabs(D[j]); rank += (o > mine) || (o == mine && j > k); }
        rank_s = rank;
        S[rank] = mine;
    }
    __syncthreads();
    const int rank = rank_s;
    for (int i = (int)threadIdx.x; i < n; i += 256) Ut[(size_t)rank * n + i] = Cm[(size_t)k * n + i];
}
#include "ptmi_dc.inc.h"

}  // extern "C"

// host side of the divide-and-conquer solver: the tree of a matrix order (all leaves at one depth, so that every level merges every
// block and the two vector buffers alternate), built once per engine
struct DcPlan {
    int n = 0, nlevels = 0, nleaves = 0, nnodes = 0;
    std::vector<int> lvl_off, lvl_cnt, lvl_nmax;       // per level (bottom-up): first node, nodes, largest node
    dc::Node *d_nodes = nullptr;                       // all merges, level by level
    dc::Leaf *d_leaves = nullptr;
    char *scr = nullptr;                               // two vector buffers, U, the per-row arrays
    int *info = nullptr;                               // a convergence word of the plan's own (ptmi_eig_dc_tridiag), in the slack of scr
};
static int dc_plan_get(ptmi_engine *h, int n, DcPlan **out)
{
    if (h->dc_plan) { *out = (DcPlan *)h->dc_plan; return PTMI_OK; }
    DcPlan *P = new (std::nothrow) DcPlan();
    if (!P) return fail(PTMI_EHIP, "out of memory");
    int depth = 0;
    while (((n + (1 << depth) - 1) >> depth) > dc::LEAF) ++depth;
    std::vector<std::vector<dc::Node>> by_depth(depth);
    std::vector<dc::Leaf> leaves;
    struct Rec { static void go(int off, int nn, int dep, int depth, std::vector<std::vector<dc::Node>> &bd, std::vector<dc::Leaf> &lv) {
        if (dep == depth) { lv.push_back({off, nn}); return; }
        const int n1 = nn / 2;
        bd[dep].push_back({off, nn, n1});
        go(off, n1, dep + 1, depth, bd, lv);
        go(off + n1, nn - n1, dep + 1, depth, bd, lv);
    } };
    Rec::go(0, n, 0, depth, by_depth, leaves);
    std::vector<dc::Node> all;
    for (int dep = depth - 1; dep >= 0; --dep) {       // bottom-up
        P->lvl_off.push_back((int)all.size());
        P->lvl_cnt.push_back((int)by_depth[dep].size());
        int mx = 0;
        for (const dc::Node &nd : by_depth[dep]) { all.push_back(nd); mx = nd.n > mx ? nd.n : mx; }
        P->lvl_nmax.push_back(mx);
    }
    P->n = n; P->nlevels = depth; P->nleaves = (int)leaves.size(); P->nnodes = (int)all.size();
    const size_t nn = (size_t)n * n;
    const size_t bytes = sizeof(double) * (3 * nn + 12 * (size_t)n + 2 * all.size() + 64) + sizeof(int) * (6 * (size_t)n + 2 * all.size() + 64);
    hipError_t e = hipMalloc((void **)&P->scr, bytes);
    if (e == hipSuccess && !all.empty()) e = hipMalloc((void **)&P->d_nodes, sizeof(dc::Node) * all.size());
    if (e == hipSuccess) e = hipMalloc((void **)&P->d_leaves, sizeof(dc::Leaf) * leaves.size());
    if (e == hipSuccess && !all.empty()) e = hipMemcpy(P->d_nodes, all.data(), sizeof(dc::Node) * all.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(P->d_leaves, leaves.data(), sizeof(dc::Leaf) * leaves.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(P->scr); (void)hipFree(P->d_nodes); (void)hipFree(P->d_leaves);
        delete P;
        return fail(PTMI_EHIP, "divide-and-conquer scratch: %s", hipGetErrorString(e));
    }
    P->info = (int *)(P->scr + bytes) - 16;
    h->dc_plan = P;
    *out = P;
    return PTMI_OK;
}
void ptmi_dc_plan_free(ptmi_engine *h)
{
    DcPlan *P = (DcPlan *)h->dc_plan;
    if (!P) return;
    (void)hipFree(P->scr); (void)hipFree(P->d_nodes); (void)hipFree(P->d_leaves);
    delete P;
    h->dc_plan = nullptr;
}
// eigenvalues (ascending, *Dres) and eigenvectors (vector-major, *Zres) of the tridiagonal matrix (D, E), back-transformed through the
// reflectors (A, tau) of the reduction (A NULL: the tridiagonal matrix's own vectors); everything queued on st
static int dc_solve(ptmi_engine *h, hipStream_t st, int n, const double *D, const double *E, const double *A, const double *tau,
                    const double **Dres, const double **Zres, int *info /* device: zeroed by the caller; a leaf that did not converge sets it */,
                    const int **cnt = nullptr /* device [2 * nnodes]: k and the number deflated of every merge */)
{
    DcPlan *P = nullptr;
    if (int rc = dc_plan_get(h, n, &P)) return rc;
    const size_t nn = (size_t)n * n;
    double *p = (double *)P->scr;
    double *Qa = p; p += nn;
    double *Qb = p; p += nn;
    dc::Args a;
    memset(&a, 0, sizeof(a));
    a.n = n;
    a.U = p; p += nn;
    a.d = p; p += n;
    a.e = p; p += n;
    double *Da = p; p += n;
    double *Db = p; p += n;
    a.dk = p; p += n; a.zk = p; p += n; a.Ddefl = p; p += n; a.mu = p; p += n; a.lam = p; p += n; a.zh = p; p += n;
    a.rho = p; p += P->nnodes + 8;
    int *q = (int *)p;
    a.keepv = q; q += n; a.deflv = q; q += n; a.org = q; q += n; a.rankk = q; q += n; a.rankd = q; q += n;
    a.cnt = q;
    HIPCHK(hipMemcpyAsync(a.d, D, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    if (n > 1) HIPCHK(hipMemcpyAsync(a.e, E, sizeof(double) * (n - 1), hipMemcpyDeviceToDevice, st));
    if (P->nnodes) hipLaunchKernelGGL(dc::split_kernel, dim3((P->nnodes + 63) / 64), dim3(64), 0, st, (const dc::Node *)P->d_nodes, P->nnodes, a.d, (const double *)a.e);
    HIPCHK(hipMemsetAsync(Qa, 0, sizeof(double) * nn, st));
    hipLaunchKernelGGL(dc::leaf_kernel, dim3(P->nleaves), dim3(64), 0, st, (const dc::Leaf *)P->d_leaves, n, (const double *)a.d, (const double *)a.e, Da, Qa, info);
    double *Qin = Qa, *Qout = Qb, *Din = Da, *Dout = Db;
    for (int lv = 0; lv < P->nlevels; ++lv) {
        const int cnt = P->lvl_cnt[lv], nmax = P->lvl_nmax[lv];
        a.nodes = P->d_nodes + P->lvl_off[lv];
        a.cnt = q + 2 * P->lvl_off[lv];
        a.Qin = Qin; a.Qout = Qout; a.Din = Din; a.Dout = Dout;
        HIPCHK(hipMemsetAsync(Qout, 0, sizeof(double) * nn, st));
        hipLaunchKernelGGL(dc::prep_kernel, dim3(cnt), dim3(dc::PREP_THREADS), 0, st, a);
        hipLaunchKernelGGL(dc::secular_kernel, dim3((nmax + 3) / 4, cnt), dim3(256), 0, st, a);
        hipLaunchKernelGGL(dc::zhat_kernel, dim3((nmax + 3) / 4, cnt), dim3(256), 0, st, a);
        hipLaunchKernelGGL(dc::vectors_kernel, dim3((nmax + 3) / 4, cnt), dim3(256), 0, st, a);
        hipLaunchKernelGGL(dc::rank_kernel, dim3(cnt), dim3(1024), 0, st, a);
        hipLaunchKernelGGL(dc::gemm_kernel, dim3((nmax + 63) / 64, (nmax + 63) / 64, cnt), dim3(256), 0, st, a);
        hipLaunchKernelGGL(dc::copy_deflated_kernel, dim3(nmax, cnt), dim3(256), 0, st, a);
        double *tq = Qin; Qin = Qout; Qout = tq;
        double *td = Din; Din = Dout; Dout = td;
    }
    if (A) hipLaunchKernelGGL(dc::backtransform_kernel, dim3((n + 4 * dc::VPW - 1) / (4 * dc::VPW)), dim3(256), 0, st, A, tau, n, Qin);
    HIPCHK(hipGetLastError());
    if (cnt) *cnt = q;
    *Dres = Din;
    *Zres = Qin;
    return PTMI_OK;
}

int ptmi_eig_sytrd(ptmi_handle h, void *stream, double *Ut_out, double *S_out) { return ptmi_eig_sytrd_from(h, stream, nullptr, Ut_out, S_out); }

int ptmi_eig_sytrd_from(ptmi_handle h, void *stream, const double *cov_in, double *Ut_out, double *S_out)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    const ptmi_config &c = h->cfg;
    if (!cov_in) cov_in = h->buf.cov;
    if (!cov_in) return fail(PTMI_EINVAL, "cov buffer missing");
    if (c.cov_per_walker || c.ngroups > 1) return fail(PTMI_EUNSUPPORTED, "ptmi_eig_sytrd factorizes ONE pooled covariance (no parameter groups)");
    const int n = c.ndim;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    double *Uo = Ut_out ? Ut_out : h->buf.Ut, *So = S_out ? S_out : h->buf.S;
    if (!Uo || !So) return fail(PTMI_EINVAL, "Ut / S buffers missing");
    int dev = 0, ncu = 0;
    HIPCHK(hipGetDevice(&dev));
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    int nb = ncu / 4 > 0 ? ncu / 4 : 1;                             // 64 blocks: the barrier's cost grows with them (21.1 ms at 64, 23.1 at 128, 27.8 at 256)
    while ((n + nb - 1) / nb > SY_CMAX && nb < ncu) nb *= 2;
    if (nb > ncu) nb = ncu;
    if (nb > n) nb = n;
    if (n < 3 || (n + nb - 1) / nb > SY_CMAX) return fail(PTMI_EUNSUPPORTED, "ptmi_eig_sytrd: 3 <= ndim <= %d on this device", SY_CMAX * nb);
    int cpb = (n + nb - 1) / nb;                                    // columns per block
    const size_t lds = sizeof(double) * ((size_t)(SY_CMAX + 3) * n + (size_t)(1 + SY_CMAX) * SY_NW);
    if (lds > 160 * 1024 || n > 1024) return fail(PTMI_EUNSUPPORTED, "ptmi_eig_sytrd: ndim = %d does not fit the LDS", n);
    (void)cpb;
    const size_t nn = (size_t)n * n;
    if (!h->d_sy_scr) HIPCHK(hipMalloc(&h->d_sy_scr, sizeof(double) * (nn + 8 * (size_t)n + 64) + 256));
    double *A = (double *)h->d_sy_scr, *D = A + nn, *E = D + n, *tau = E + n, *vbuf = tau + n, *pbuf = vbuf + 2 * (n + 2);
    unsigned *bar = (unsigned *)(pbuf + 2 * n + 2);
    int *info = (int *)(bar + 4);
    HIPCHK(hipMemcpyAsync(A, cov_in, sizeof(double) * nn, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemsetAsync(bar, 0, 32, st));
    HIPCHK(hipFuncSetAttribute((const void *)sytrd_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    SytrdArgs sa = {A, D, E, tau, vbuf, pbuf, bar, n};
    // The kernel's grid barrier needs all nb blocks resident at once.  One block per CU always fits an otherwise free CU (checked
    // here against the occupancy the runtime computes); beside persistent step kernels the blocks take the CUs' remaining LDS as it
    // is (the step kernel leaves 78 KB, a block needs up to 160: such a block starts when its CU's step block ends, and every step
    // block ends).  What could deadlock is a SECOND factorization of another engine on the same device holding part of the CUs with
    // blocks that spin: factorizations of one device are therefore serialized by an event chain across engines and streams.
    int occ = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)sytrd_lds_kernel, SY_THREADS, lds));
    if (occ < 1 || (long long)occ * ncu < nb)
        return fail(PTMI_EUNSUPPORTED, "ptmi_eig_sytrd: %d blocks of %zu B of LDS cannot be resident at once on %d CUs", nb, lds, ncu);
    {
        static std::mutex mu;
        static hipEvent_t last[64] = {};
        std::lock_guard<std::mutex> lk(mu);
        const int di = dev & 63;
        if (last[di]) HIPCHK(hipStreamWaitEvent(st, last[di], 0));
        else HIPCHK(hipEventCreateWithFlags(&last[di], hipEventDisableTiming));
        hipLaunchKernelGGL(sytrd_lds_kernel, dim3(nb), dim3(SY_THREADS), lds, st, sa);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(last[di], st));
    }
    h->sy_reduced = 1;
    // the tridiagonal matrix's eigenvectors by the engine's own divide-and-conquer kernels, back-transformed through the reflectors
    const double *Dres = nullptr, *Zres = nullptr;
    if (int rc = dc_solve(h, st, n, D, E, A, tau, &Dres, &Zres, info)) return rc;
    hipLaunchKernelGGL(eig_sort_rows_kernel, dim3(n), dim3(256), 0, st, Dres, Zres, n, Uo, So);
    HIPCHK(hipGetLastError());
    // the convergence word (a leaf's QL iteration: dc::leaf_kernel) follows the result to the host on the same stream
    // (ptmi_eig_sytrd_info reads the last one that arrived)
    if (!h->h_sy_info) {
        HIPCHK(hipHostMalloc((void **)&h->h_sy_info, 2 * sizeof(int32_t)));
        h->h_sy_info[0] = 0; h->h_sy_info[1] = 0;
    }
    HIPCHK(hipMemcpyAsync(h->h_sy_info, info, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    return PTMI_OK;
}

int ptmi_eig_sytrd_info(ptmi_handle h, int32_t *info)
{
    if (!h || !info) return fail(PTMI_EINVAL, "NULL argument");
    *info = h->h_sy_info ? h->h_sy_info[0] : 0;
    return PTMI_OK;
}

// the stages on their own (tests/test_eig_dc_gpu.py): the tridiagonal solver on the caller's matrix, and the reduction's output
// a matrix that is ONE leaf (n <= dc::LEAF, no merge): the leaf's eigenvalues come in the order its QL iteration leaves them (the
// merges sort their children's, ptmi_eig_sytrd sorts by size at the end) -- ranked ascending here, ties by position as in rank_kernel
__global__ __launch_bounds__(64) void dc_leaf_sort_kernel(const double *D, const double *Q, int n, double *W, double *Z)
{
    const int t = (int)threadIdx.x;
    if (t >= n) return;
    const double mine = D[t];
    int rank = 0;
    for (int j = 0; j < n; ++j) { const double o = D[j]; rank += (o < mine) || (o == mine && j < t); }
    W[rank] = mine;
    for (int i = 0; i < n; ++i) Z[(size_t)rank * n + i] = Q[(size_t)t * n + i];
}

int ptmi_eig_dc_tridiag(ptmi_handle h, void *stream, const double *d, const double *e, double *W, double *Z, int32_t *cnt)
{
    if (!h || !d || !W || !Z) return fail(PTMI_EINVAL, "NULL argument");
    const int n = h->cfg.ndim;
    if (n < 1 || n > dc::NMAX) return fail(PTMI_EUNSUPPORTED, "ptmi_eig_dc_tridiag: 1 <= ndim <= %d", dc::NMAX);
    if (n > 1 && !e) return fail(PTMI_EINVAL, "NULL argument");
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    DcPlan *P = nullptr;
    if (int rc = dc_plan_get(h, n, &P)) return rc;
    HIPCHK(hipMemsetAsync(P->info, 0, sizeof(int), st));
    const double *Dres = nullptr, *Zres = nullptr;
    const int *counts = nullptr;
    if (int rc = dc_solve(h, st, n, d, e, nullptr, nullptr, &Dres, &Zres, P->info, &counts)) return rc;
    if (P->nlevels == 0) {
        hipLaunchKernelGGL(dc_leaf_sort_kernel, dim3(1), dim3(64), 0, st, Dres, Zres, n, W, Z);
        HIPCHK(hipGetLastError());
    } else {
        HIPCHK(hipMemcpyAsync(W, Dres, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(Z, Zres, sizeof(double) * n * n, hipMemcpyDeviceToDevice, st));
    }
    if (cnt && P->nnodes) HIPCHK(hipMemcpyAsync(cnt, counts, sizeof(int32_t) * 2 * P->nnodes, hipMemcpyDeviceToDevice, st));
    if (!h->h_sy_info) {
        HIPCHK(hipHostMalloc((void **)&h->h_sy_info, 2 * sizeof(int32_t)));
        h->h_sy_info[0] = 0; h->h_sy_info[1] = 0;
    }
    HIPCHK(hipMemcpyAsync(h->h_sy_info, P->info, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    return PTMI_OK;
}

int ptmi_eig_sytrd_reduction(ptmi_handle h, void *stream, double *D, double *E, double *tau, double *A)
{
    if (!h || !D || !E || !tau || !A) return fail(PTMI_EINVAL, "NULL argument");
    if (!h->d_sy_scr || !h->sy_reduced) return fail(PTMI_EINVAL, "ptmi_eig_sytrd_reduction: no ptmi_eig_sytrd has run on this handle");
    const int n = h->cfg.ndim;
    const size_t nn = (size_t)n * n;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    const double *As = (const double *)h->d_sy_scr, *Ds = As + nn, *Es = Ds + n, *ts = Es + n;
    HIPCHK(hipMemcpyAsync(A, As, sizeof(double) * nn, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(D, Ds, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(E, Es, sizeof(double) * (n - 1), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(tau, ts, sizeof(double) * (n - 1), hipMemcpyDeviceToDevice, st));
    return PTMI_OK;
}
