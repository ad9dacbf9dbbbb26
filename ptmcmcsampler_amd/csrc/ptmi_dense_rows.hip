// ptmi_dense_rows.hip -- the built-in dense Gaussian (PTMI_LOGL_DENSE) and the built-in priors over n rows [n][ndim] anywhere in device
// memory: ptmi_rows_logl / ptmi_rows_logl_grad / ptmi_rows_logp (include/ptmi.h).  The split path's likelihood stage for handles whose
// table does not fit LDS (ndim > 104), served at every ndim the shapes take (1 .. 2048).
//
// The oracle defines the value and the gradient as k-ascending fma chains (oracle/ptmcmc_oracle.c eval_logl, eval_logl_grad):
//     r = x - mu;  v_i = sum_k Tl[k][i] r_k;  logl = -lane_dot(r, v, d, G);      g_i = -sum_k Pt[k][i] r_k
// every v_i / g_i ONE accumulator that starts at +0.0 and takes k = 0 .. d-1 in turn, lane_dot = lane l of G folds elements l, l + G, ..
// by fma, then the xor butterfly G/2 .. 1.  v_mfma_f64_16x16x4_f64 is bit for bit such a chain (tools/mfma_probe.hip), so the product
// runs on the matrix cores: a wave owns RT row tiles of 16 rows and walks the output columns in groups of NT tiles of 16, ascending.
// Per k-step of 4 it loads NT table values (lane (c, g): T[k0 + g][16 j + c]; the table is shared by every wave of the launch and
// stays in L2 / MALL) and RT residuals (lane (c, g): x[row c][k0 + g] - mu[k0 + g]) and issues RT x NT matrix instructions; the
// operands of step k0 + 4 are requested before the instructions of step k0.  The result layout (col = lane & 15 = the row of the tile,
// row = (lane >> 4) + 4 reg = the output column) puts elements 16 j + g + 4 reg of row c into lane (c, g): its partial of lane_dot
// is partial (16 j + g + 4 reg) % G, so a lane keeps 1 / 4 / 16 partials per row for G = 4 / 16 / 64, folds a finished group of
// columns into them in ascending order and drops it: V never goes to memory.  The butterfly's stages 32 .. 4 are register adds
// inside the lane, stages 2 and 1 two cross-lane moves.
//
// Padding: k-steps past ndim multiply a table operand of 1.0 by a residual of -0.0: x + (-0.0) = x for every x, -0.0 and NaN included,
// so the pad leaves every accumulator's bits alone (a +0.0 would turn an accumulator of -0.0 into +0.0).  Columns past ndim read
// column ndim - 1 and are never folded or stored.
//
// The value's table Tl is zero above its diagonal (Tl[k][i] = 0 for k < i).  The oracle multiplies through those zeros: with finite
// residuals each such step adds +-0 to an accumulator that is still +0.0 and leaves +0.0, so the steps k < 16 j0 of a column group
// and the tiles of a group that are still entirely above the diagonal are skipped -- half the value's work.  A residual of inf or
// NaN makes 0 * r = NaN there, so a wave whose rows hold one (a wave-uniform test of all its residuals, one extra pass over the rows)
// walks the whole table.  The gradient's table Pt is full.
#include "ptmi_common.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

// RT row tiles (of 16 rows) per wave, NT column tiles (of 16) per group -- NT a multiple of 4, so that tile t of a group is partial
// block t % 4 at G = 64.  Chosen per launch (launch_dense): the bits do not depend on them.  Measured (value kernel, ms):
//   (RT, NT)      105-d x 65536   200-d x 65536   416-d x 65536   1000-d x 16384
//   (2, 4)            0.050           0.112           0.400           0.967        (1000-d: 128 blocks, half the CUs idle)
//   (2, 8)            0.071           0.135           0.388           0.797
//   (4, 4)            0.050           0.113           0.352           1.560
//   (1, 8)            0.070           0.148           0.466           0.606
// so: wide groups where the rows' re-reads per group dominate (ndim > 512), one row tile per wave while the launch has fewer than
// 32768 rows (blocks for every CU first).

// One pass of a wave over a table T[d][d] (row k, column i): acc-chains for columns [16 j0, 16 (j0 + NT)) of its rows, k from kbeg.
// LOWER: tiles still entirely above the diagonal at a step are left out (see above).
template <bool LOWER, int RT, int NT>
__device__ __forceinline__ void col_group(const double *T, const double *mu, const double *const (&xp)[RT], int d, int ntile, int j0, int kbeg,
                                          int c, int g, d4 (&acc)[RT][NT])
{
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[rt][t] = d4{0.0, 0.0, 0.0, 0.0};
    int col[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int i = 16 * (j0 + t) + c;
        col[t] = i < d ? i : d - 1;
    }
    double ta[NT], tn[NT], ra[RT], rn[RT];
    auto fetch = [&](int k0, double (&tv)[NT], double (&rv)[RT]) {
        const int k = k0 + g;
        const bool in = k < d;
        const int kk = in ? k : d - 1;
        const double m = mu[kk];
        const double *row = T + (size_t)kk * d;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const double v = row[col[t]];
            tv[t] = in ? v : 1.0;
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const double v = xp[rt][kk] - m;
            rv[rt] = in ? v : -0.0;
        }
    };
    fetch(kbeg, ta, ra);
#pragma unroll 1
    for (int k0 = kbeg; k0 < d; k0 += 4) {
        fetch(k0 + 4 < d ? k0 + 4 : k0, tn, rn);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (j0 + t >= ntile) continue;                               // wave-uniform
            if (LOWER && 16 * (j0 + t) > k0 + 3) continue;               // wave-uniform: the tile is above the diagonal
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ta[t], ra[rt], acc[rt][t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) ta[t] = tn[t];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) ra[rt] = rn[rt];
    }
}

// G: the handle's lanes per chain (the order of lane_dot).  GRAD: also g = -(R Pt) to grad[n][d].
template <int G, bool GRAD, int RT, int NT>
__global__ __launch_bounds__(256) void dense_rows_kernel(const double *rows, long long n, int d, const double *par, double *out, double *grad)
{
    static_assert(NT % 4 == 0 && RT >= 1, "column groups of a multiple of four tiles");
    constexpr int WROWS = 16 * RT;                                        // rows per wave
    constexpr int TT = G == 64 ? 4 : 1, RR = G >= 16 ? 4 : 1;             // partials of lane_dot a lane keeps per row: [tile % 4][reg]
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int c = lane & 15, g = lane >> 4;
    const long long row0 = ((long long)blockIdx.x * 4 + wave) * WROWS;
    if (row0 >= n) return;                                               // (whole waves; the kernel has no block-wide barrier)
    const double *mu = par, *Pt = par + d, *Tl = par + d + (size_t)d * d;
    const int ntile = (d + 15) / 16;
    const double *xp[RT];
    long long rowi[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        rowi[rt] = row0 + 16 * rt + c;
        xp[rt] = rows + (size_t)(rowi[rt] < n ? rowi[rt] : n - 1) * d;   // rows past the end: the last row's values, never stored
    }
    // are all residuals of this wave's rows finite?  (lane (c, g) looks at elements g, g + 4, .. of its rows)
    bool fin = true;
    for (int k = g; k < d; k += 4) {
        const double m = mu[k];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const double r = xp[rt][k] - m;
            fin = fin && (r - r == 0.0);
        }
    }
    const bool skip = __all(fin);
    double p[RT][TT][RR];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
#pragma unroll
            for (int rr = 0; rr < RR; ++rr) p[rt][tt][rr] = 0.0;
    d4 acc[RT][NT];
#pragma unroll 1
    for (int j0 = 0; j0 < ntile; j0 += NT) {
        if (skip) col_group<true, RT, NT>(Tl, mu, xp, d, ntile, j0, 16 * j0, c, g, acc);
        else col_group<false, RT, NT>(Tl, mu, xp, d, ntile, j0, 0, c, g, acc);
        // lane_dot's strided fma chains: element i = 16 (j0 + t) + g + 4 reg goes to partial i % G, in ascending i
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * (j0 + t) + g + 4 * r;
                if (i < d) {
                    const double m = mu[i];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        double &q = p[rt][G == 64 ? (t & 3) : 0][G >= 16 ? r : 0];
                        q = __builtin_fma(xp[rt][i] - m, acc[rt][t][r], q);
                    }
                }
            }
        if (GRAD) {
            col_group<false, RT, NT>(Pt, mu, xp, d, ntile, j0, 0, c, g, acc);
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * (j0 + t) + g + 4 * r;
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
                        if (i < d && rowi[rt] < n) grad[(size_t)rowi[rt] * d + i] = -acc[rt][t][r];
                }
        }
    }
    // the xor butterfly G/2 .. 1 over the partials l = 16 tt + 4 rr + g: stages 32, 16 (tt), 8, 4 (rr) inside the lane, 2 and 1 across
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        double s[RR];
#pragma unroll
        for (int rr = 0; rr < RR; ++rr) {
            if (TT == 4) s[rr] = (p[rt][0][rr] + p[rt][TT / 2][rr]) + (p[rt][TT / 4][rr] + p[rt][TT / 4 + TT / 2][rr]);
            else s[rr] = p[rt][0][rr];
        }
        double v = RR == 4 ? (s[0] + s[RR / 2]) + (s[RR / 4] + s[RR / 4 + RR / 2]) : s[0];
        v = v + __shfl_xor(v, 32, 64);
        v = v + __shfl_xor(v, 16, 64);
        if (g == 0 && rowi[rt] < n) out[rowi[rt]] = -v;
    }
}

// g = -x: the isotropic Gaussian's gradient (eval_logl_grad, LOGL_ISO)
__global__ __launch_bounds__(256) void neg_kernel(const double *x, long long total, double *g)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) g[i] = -x[i];
}

// The built-in priors (oracle: eval_logp; the reference's tests/test_simple.py:36-41): flat 0; box -inf unless lo <= x <= hi in every
// element, the comparison written as the oracle writes it, so that a NaN element gives -inf.  16 lanes per row.
__global__ __launch_bounds__(256) void rows_logp_kernel(const double *rows, long long n, int d, int box, const double *par, double *lp)
{
    const int l = (int)(threadIdx.x & 15);
    const long long row = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    int out = 0;
    if (box && row < n) {
        const double *x = rows + (size_t)row * d, *lo = par, *hi = par + d;
        for (int i = l; i < d; i += 16)
            if (!(lo[i] <= x[i]) || !(hi[i] >= x[i])) out = 1;
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) out |= __shfl_xor(out, m, 64);
    if (l == 0 && row < n) lp[row] = out ? -__builtin_inf() : 0.0;
}

template <int G, bool GRAD, int RT, int NT>
void launch_one(ptmi_engine *h, const double *rows, long long n, double *out, double *grad)
{
    const long long brows = 4 * 16 * RT;                                  // rows per block of four waves
    hipLaunchKernelGGL((dense_rows_kernel<G, GRAD, RT, NT>), dim3((unsigned)((n + brows - 1) / brows)), dim3(256), 0, h->stream, rows, n,
                       h->cfg.ndim, h->d_loglpar, out, grad);
}

template <int G, bool GRAD>
int launch_shape(ptmi_engine *h, const double *rows, long long n, double *out, double *grad)
{
    const bool two = n >= 32768;                                          // two row tiles per wave once there are blocks for every CU
    if constexpr (G == 64) {
        if (h->cfg.ndim > 512) {
            if (two) launch_one<G, GRAD, 2, 8>(h, rows, n, out, grad);
            else launch_one<G, GRAD, 1, 8>(h, rows, n, out, grad);
            return PTMI_OK;
        }
    }
    if (two) launch_one<G, GRAD, 2, 4>(h, rows, n, out, grad);
    else launch_one<G, GRAD, 1, 4>(h, rows, n, out, grad);
    return PTMI_OK;
}

template <bool GRAD>
int launch_dense(ptmi_engine *h, const double *rows, long long n, double *out, double *grad)
{
    if (h->G == 4) return launch_shape<4, GRAD>(h, rows, n, out, grad);
    if (h->G == 16) return launch_shape<16, GRAD>(h, rows, n, out, grad);
    if (h->G == 64) return launch_shape<64, GRAD>(h, rows, n, out, grad);
    return ptmi_fail(PTMI_EINVAL, "dense rows: unknown shape (%d lanes per chain)", h->G);
}

}  // namespace

// ptmi_rows_logl / ptmi_rows_logl_grad for PTMI_LOGL_DENSE (grad == nullptr: the value alone)
int ptmi_rows_dense(ptmi_engine *h, const double *rows, long long n, double *out, double *grad)
{
    return grad ? launch_dense<true>(h, rows, n, out, grad) : launch_dense<false>(h, rows, n, out, nullptr);
}

// the gradient of PTMI_LOGL_ISO for ptmi_rows_logl_grad
int ptmi_rows_neg(ptmi_engine *h, const double *rows, long long n, double *grad)
{
    const long long total = n * h->cfg.ndim;
    hipLaunchKernelGGL(neg_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, rows, total, grad);
    return PTMI_OK;
}

// ptmi_rows_logp
int ptmi_rows_prior(ptmi_engine *h, const double *rows, long long n, double *lp)
{
    hipLaunchKernelGGL(rows_logp_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, h->stream, rows, n, h->cfg.ndim,
                       h->cfg.logp_kind == PTMI_LOGP_BOX ? 1 : 0, h->d_logppar, lp);
    return PTMI_OK;
}
