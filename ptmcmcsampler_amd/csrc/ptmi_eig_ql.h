// ptmi_eig_ql.h -- what the two units of the tridiagonal QL eigensolver share (ptmi_eig.hip: the matrix in LDS, ndim <= 128;
// ptmi_eig_wide.hip: the matrix in a global scratch, 128 < ndim <= 1024): the oct butterfly, the rotation's root and reciprocal,
// the scratch of the three-kernel form and the QL iterations themselves.
#pragma once
#include "ptmi_common.h"

// sum over the eight lanes of a pair: xor 4, xor 2, xor 1 (the oracle's ((s0+s4)+(s2+s6)) + ((s1+s5)+(s3+s7)))
__device__ __forceinline__ double jac_oct_sum(double p)
{
    p = p + __shfl_xor(p, 4, 64);
    p = p + dppf64<0x4E>(p);     // xor 2
    p = p + dppf64<0xB1>(p);     // xor 1
    return p;
}

// sqrt(x) and 1 / sqrt(x)'s partner 1 / r of a rotation, for x in the middle of the exponent range: the compiler's own correctly
// rounded sequences (v_rsq_f64 / v_rcp_f64 + the fma refinements of its sqrt and division lowerings) without their range scaling,
// special-value tests and fix-ups -- 17 instead of 29 instructions on the chain that bounds eig_ql_chain_kernel, the same bits
// wherever no scaling would have been applied; anything else takes the plain operations.
__device__ __forceinline__ void ql_root_and_reciprocal(double x, double &r, double &ri)
{
    if (x > 0x1p-600 && x < 0x1p600) {                              // uniform in the chain kernel
        const double y = __builtin_amdgcn_rsq(x);
        double g = x * y, hh = 0.5 * y;
        const double r0 = __builtin_fma(-hh, g, 0.5);
        g = __builtin_fma(g, r0, g);
        hh = __builtin_fma(hh, r0, hh);
        double dd = __builtin_fma(-g, g, x);
        g = __builtin_fma(dd, hh, g);
        dd = __builtin_fma(-g, g, x);
        r = __builtin_fma(dd, hh, g);
        double q = __builtin_amdgcn_rcp(r);
        double e = __builtin_fma(-r, q, 1.0);
        q = __builtin_fma(q, e, q);
        e = __builtin_fma(-r, q, 1.0);
        q = __builtin_fma(q, e, q);
        e = __builtin_fma(-r, q, 1.0);
        ri = __builtin_fma(e, q, q);
    } else {
        r = det_sqrt(x);
        ri = 1.0 / r;
    }
}

constexpr int QL_MAXIT = 60;

typedef double qls_d2 __attribute__((ext_vector_type(2)));
struct QlScratch {
    double *z;          // [nmat][n][n]  the accumulated transformations, row-major
    qls_d2 *de;         // [nmat][n]     {d[i], e[i]} (subdiagonal shifted: e[i] couples i and i + 1)
    double *ev;         // [nmat][n]     the eigenvalues the chains end with
    qls_d2 *rot;        // [nmat][cap]   the rotations, in the order they are applied
    int32_t *hdr;       // [nmat][2 capit]  l, m of every QL iteration
    int32_t *cnt;       // [nmat][2]     iterations recorded, overflow flag
    int cap, capit;
};

// the QL iterations on {d, e} pairs in LDS (one wave; every lane runs the scalar recurrence).  ROWS: the lane also turns rows of
// the eigenvector matrix -- rows t and t + 64 of zt, the matrix TRANSPOSED in LDS (column c at zt[c n ...], so that the lanes' rows
// sit side by side), or, with GLOBAL, rows t, t + 64, t + 128, ... of the row-major matrix zt in global memory (the wide unit's
// redo: slow and rare); else the rotations and the iterations' (l, m) are recorded.  Returns the iterations (negative: an eigenvalue
// did not converge).
template <bool ROWS, bool GLOBAL = false>
__device__ __forceinline__ int ql_iterate(qls_d2 *de, int n, int t, double *zt, qls_d2 *rot, int32_t *hdr, int cap, int capit, int *overflow)
{
    const int k0 = t, k1 = t + 64;
    const bool r0 = ROWS && !GLOBAL && k0 < n, r1 = ROWS && !GLOBAL && k1 < n;
    int iters = 0, nrot = 0;
    bool over = false, failed = false;
    double f = 0.0, tst1 = 0.0;
    for (int l = 0; l < n && !failed; ++l) {
        const qls_d2 del = de[l];
        const double t0 = __builtin_fabs(del.x) + __builtin_fabs(del.y);
        if (tst1 < t0) tst1 = t0;
        int m = l;
        while (m < n - 1 && tst1 + __builtin_fabs(de[m].y) != tst1) ++m;
        double dlf = del.x;
        if (m > l) {
            int it = 0;
            double el;
            do {
                if (++it > QL_MAXIT) { failed = true; break; }
                if (!ROWS) {
                    if (iters >= capit || nrot + (m - l) > cap) over = true;
                    if (!over && t == 0) { hdr[2 * iters] = l; hdr[2 * iters + 1] = m; }
                }
                ++iters;
                const qls_d2 pl = de[l], pl1 = de[l + 1];
                const double g = pl.x, e_l = pl.y;
                const double p0 = (pl1.x - g) / (2.0 * e_l);
                const double rr0 = det_sqrt(p0 * p0 + 1.0);
                const double pr = p0 + (p0 >= 0.0 ? rr0 : -rr0);
                const double dl = e_l / pr, dl1 = e_l * pr;
                const double h = g - dl;
                const double el1 = pl1.y;
                double p = de[m].x;
                asm volatile("" ::: "memory");
                if (t == 0) { de[l].x = dl; de[l + 1].x = dl1; }
                for (int i = l + 2 + t; i < n; i += 64) de[i].x = de[i].x - h;
                asm volatile("" ::: "memory");
                f = f + h;
                if (m == l + 1) p = dl1; else if (m >= l + 2) p = p - h;
                double c = 1.0, c2 = 1.0, c3 = 1.0, s = 0.0, s2 = 0.0;
                qls_d2 nx = de[m - 1];
                double zb0 = r0 ? zt[m * n + k0] : 0.0, zb1 = r1 ? zt[m * n + k1] : 0.0;
                for (int i = m - 1; i >= l; --i) {
                    c3 = c2; c2 = c; s2 = s;
                    const double di = nx.x, ei = nx.y;
                    if (i > l) nx = de[i - 1];
                    double za0 = 0.0, za1 = 0.0;
                    if (ROWS && !GLOBAL) { za0 = r0 ? zt[i * n + k0] : 0.0; za1 = r1 ? zt[i * n + k1] : 0.0; }
                    const double gg = c * ei, hh = c * p;
                    double r, ri;
                    ql_root_and_reciprocal(p * p + ei * ei, r, ri);
                    const double e1 = s * r;
                    s = ei * ri;
                    c = p * ri;
                    p = c * di - s * gg;
                    const double d1 = hh + s * (c * gg + s * di);
                    if (t == 0) de[i + 1] = qls_d2{d1, e1};
                    if (ROWS && GLOBAL) {
                        for (int k = t; k < n; k += 64) {
                            double *zk = zt + (size_t)k * n + i;
                            const double za = zk[0], zb = zk[1];
                            zk[1] = s * za + c * zb;
                            zk[0] = c * za - s * zb;
                        }
                    } else if (ROWS) {
                        if (r0) zt[(i + 1) * n + k0] = s * za0 + c * zb0;
                        if (r1) zt[(i + 1) * n + k1] = s * za1 + c * zb1;
                        zb0 = c * za0 - s * zb0;
                        zb1 = c * za1 - s * zb1;
                    } else if (!over && t == 0) {
                        rot[nrot + (m - 1 - i)] = qls_d2{c, s};
                    }
                }
                if (ROWS && !GLOBAL) {
                    if (r0) zt[l * n + k0] = zb0;
                    if (r1) zt[l * n + k1] = zb1;
                }
                nrot += m - l;
                p = -s * s2 * c3 * el1 * e_l / dl1;
                el = s * p;
                dlf = c * p;
                asm volatile("" ::: "memory");
                if (t == 0) de[l] = qls_d2{dlf, el};
                asm volatile("" ::: "memory");
            } while (tst1 + __builtin_fabs(el) != tst1);
        }
        asm volatile("" ::: "memory");
        if (t == 0) de[l] = qls_d2{dlf + f, 0.0};
        asm volatile("" ::: "memory");
    }
    if (overflow) *overflow = over ? 1 : 0;
    return failed ? -iters - 1 : iters;
}

// eig_ql_chain_kernel (ptmi_eig.hip) for `nmat` matrices of order n on `stream`: the chains need {d, e} alone, at any order
void eig_ql_chain_launch(hipStream_t stream, int n, int nmat, const QlScratch &q);
// ptmi_eig_ql's kernels for 128 < n <= 1024 (ptmi_eig_wide.hip); arguments as eig_ql_run
int eig_ql_wide_run(ptmi_engine *h, int n, int nmat, const double *cov, double *Ut, double *S);
