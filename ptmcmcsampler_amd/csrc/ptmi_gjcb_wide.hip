// ptmi_gjcb_wide.hip -- HMC on the split path with batched gradient callbacks at 512 < ndim <= 2048 (ptmi_gj_begin / ptmi_gj_step of
// ptmi_gjcb.hip, which keeps the stage's sequencing, the work area and the listing).  The arithmetic is the one of gj_begin_kernel /
// gj_step_kernel there at G = 64 lanes per chain, operation for operation (the oracle: hmc_call of oracle/ptmcmc_oracle.c); what changes
// is where it runs:
//
//   the whitening products  out[i] = sum_k T[k][i] v[k]  over the listed chains are n rows times one full d x d table, every out[i] ONE
//   accumulator that starts at +0.0 and takes k = 0 .. d-1 in turn: bit for bit what v_mfma_f64_16x16x4_f64 computes (tools/mfma_probe.hip,
//   ptmi_dense_rows.hip's header).  gjw_product_kernel is the walk of ptmi_dense_rows.hip's col_group<false, RT, NT> -- a wave owns RT
//   tiles of 16 listed chains and goes through the output columns in groups of NT tiles of 16, ascending; per k-step of 4 it loads NT
//   table values and RT operands, the operands of step k0 + 4 requested before the instructions of step k0 -- with the stage's
//   operands in front (a chain's proposal row or whitened position through the round's list; g = beta dlnl + dlp formed as
//   gj_step_kernel forms it) and a plain store behind (to the listed chain's row of the work area, or to its proposal when its call
//   has ended).  K-steps past ndim multiply a table operand of 1.0 by an input of -0.0 (leaves -0.0, NaN and inf accumulators alone),
//   columns past ndim read column ndim - 1 and are never stored.  Diagonal tables stay d multiplications T[i][i] v[i].
//
//   the step (gjw_step_kernel) is one wave per listed chain, lane gl owning elements gl + 64 e; the chain's vectors stay in the work
//   area and the wave streams over its slots e in ascending order (the dot products' fma partials take the slots in that order, then
//   group_sum<64>), so the kernel holds no per-slot registers and serves every ndim.
//
// A round is: gradient product (into xs), step, backward product, listing (gj_count_kernel / gj_fill_kernel for the list and its
// count, gjw_rows_kernel for the rows); ptmi_gj_begin lists the HMC picks before its forward and backward products (ptmi_gjcb.hip:
// wide_begin / wide_round).
#include "ptmi_gjcb.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

enum { OP_ROW = 0, OP_GRAD = 1, OP_GRAD_PRIOR = 2 };   // the product's operand: in[list[j]][k]; beta dlnl[j][k] + 0.0; beta dlnl[j][k] + dlp[j][k]

struct ProdArgs {
    const double *T;                 // the table [d][d] (row k, column i)
    int d;
    long long n;                     // listed chains, or ...
    const long long *nptr;           // ... where the listing left their count (ptmi_gj_begin)
    const int32_t *list;             // the listed chains' slots
    const double *in;                // OP_ROW: [nch][d]
    const double *dlnl, *dlp;        // OP_GRAD*: the callback's gradients of row j
    const double *beta;
    const int32_t *temp_of;
    double *out;                     // [nch][d]: row list[j]
    double *out_done;                // backward product of a round: the row of a chain whose call has ended (ist: not listed again) ...
    const int32_t *ist;              // ... goes here (its proposal)
};

template <int OP>
struct Operand {
    const double *x, *gp;
    double beta;
    __device__ __forceinline__ double operator()(int k) const
    {
        if (OP == OP_ROW) return x[k];
        const double gl_ = x[k], g2 = OP == OP_GRAD_PRIOR ? gp[k] : 0.0;
        return beta * gl_ + g2;                                          // NJ:82-86: multiply, then add (the built-in priors: + 0.0)
    }
};

template <int OP>
__device__ __forceinline__ void row_setup(const ProdArgs &a, long long row, long long n, Operand<OP> &o, double *&out, bool &ok)
{
    ok = row < n;
    const long long r = ok ? row : n - 1;                                // rows past the end: the last row's values, never stored
    const long long ch = a.list[r];
    if (OP == OP_ROW) {
        o.x = a.in + (size_t)ch * a.d; o.gp = nullptr; o.beta = 0.0;
    } else {
        o.x = a.dlnl + (size_t)r * a.d;
        o.gp = OP == OP_GRAD_PRIOR ? a.dlp + (size_t)r * a.d : nullptr;
        o.beta = a.beta[a.temp_of[ch]];
    }
    double *base = (a.out_done && a.ist[(size_t)ch * 4 + ST_ACT] == 0) ? a.out_done : a.out;
    out = base + (size_t)ch * a.d;
}

// One pass of a wave over the table: acc-chains for columns [16 j0, 16 (j0 + NT)) of its RT x 16 rows, k = 0 .. d-1
template <int OP, int RT, int NT>
__device__ __forceinline__ void col_group(const double *T, const Operand<OP> (&xp)[RT], int d, int ntile, int j0, int c, int g, d4 (&acc)[RT][NT])
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
        const double *row = T + (size_t)kk * d;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const double v = row[col[t]];
            tv[t] = in ? v : 1.0;
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const double v = xp[rt](kk);
            rv[rt] = in ? v : -0.0;
        }
    };
    fetch(0, ta, ra);
#pragma unroll 1
    for (int k0 = 0; k0 < d; k0 += 4) {
        fetch(k0 + 4 < d ? k0 + 4 : k0, tn, rn);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (j0 + t >= ntile) continue;                               // wave-uniform
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ta[t], ra[rt], acc[rt][t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) ta[t] = tn[t];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) ra[rt] = rn[rt];
    }
}

template <int OP, int RT, int NT>
__global__ __launch_bounds__(256) void gjw_product_kernel(const ProdArgs a)
{
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int c = lane & 15, g = lane >> 4;
    const long long n = a.nptr ? *a.nptr : a.n;
    const long long row0 = ((long long)blockIdx.x * 4 + wave) * (16 * RT);
    if (row0 >= n) return;                                               // (whole waves; the kernel has no block-wide barrier)
    const int d = a.d, ntile = (d + 15) / 16;
    Operand<OP> xp[RT];
    double *op[RT];
    bool ok[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) row_setup<OP>(a, row0 + 16 * rt + c, n, xp[rt], op[rt], ok[rt]);
    d4 acc[RT][NT];
#pragma unroll 1
    for (int j0 = 0; j0 < ntile; j0 += NT) {
        col_group<OP, RT, NT>(a.T, xp, d, ntile, j0, c, g, acc);
        // the result layout: element 16 (j0 + t) + g + 4 reg of row c
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * (j0 + t) + g + 4 * r;
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
                    if (i < d && ok[rt]) op[rt][i] = acc[rt][t][r];
            }
    }
}

// diagonal tables: out[i] = T[i][i] v[i], 64 lanes per listed chain
template <int OP>
__global__ __launch_bounds__(256) void gjw_diag_kernel(const ProdArgs a)
{
    const long long n = a.nptr ? *a.nptr : a.n;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    Operand<OP> x;
    double *out;
    bool ok;
    row_setup<OP>(a, row, n, x, out, ok);
    const int d = a.d;
    for (int i = (int)(threadIdx.x & 63); i < d; i += 64) out[i] = a.T[(size_t)i * d + i] * x(i);
}

__global__ __launch_bounds__(256) void gjw_mark_kernel(const double *qaux, long long nch, int32_t *ist)
{
    const long long ch = (long long)blockIdx.x * 256 + threadIdx.x;
    if (ch >= nch) return;
    const double jt = qaux[(size_t)ch * 4 + 1];
    const bool on = jt == (double)PTMI_J_HMC;
    *reinterpret_cast<int4 *>(ist + (size_t)ch * 4) = int4{on ? 1 : 0, 0, 0, 0};
}

// One round of a listed chain (row j of the callback's values; its whitened gradient waits in xs).  First round: logp0, the momenta,
// joint0 and nsteps, then the first half kick and drift; later rounds: the second half kick, joint1 and the guard; then either the
// next half kick and drift (listed again) or the end of the call (qxy, the jump state; the backward product writes the proposal).
// gj_step_kernel's HMC branch with the chain's vectors in the work area instead of register slots.
__global__ __launch_bounds__(256) void gjw_step_kernel(const GjArgs a)
{
    const int gl = (int)(threadIdx.x & 63), d = a.d;
    const long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= a.n) return;                                                // (whole waves; no block-wide barrier)
    const long long ch = (long long)a.w.list[j];
    const int t = a.temp_of[ch];
    const double beta = a.beta[t];
    const int w = (int)(ch / a.nt);
    const u32 sid = (u32)((u64)(a.walker0 + w) * (u32)a.ntg) + (u32)(a.temp0 + t);
    const int4 st = *reinterpret_cast<const int4 *>(a.w.ist + (size_t)ch * 4);
    double *q = a.w.q + (size_t)ch * d, *p = a.w.p + (size_t)ch * d;
    const double *gw = a.w.xs + (size_t)ch * d;                          // the gradient in the whitened coordinates (NJ:87-88)
    const double logp = beta * a.lnl[j] + (a.lp ? a.lp[j] : 0.0);
    const double he = 0.5 * a.eps;
    double joint0, joint1, part = 0.0;
    int left = st.z, nleap = st.w;
    bool done;
    if (st.y == 0) {
        // GradJump::momenta, block 0 (NJ:92-94): directions k and k + 64 share one Box-Muller
#pragma unroll 1
        for (int k = gl; k < d; k += 128) {
            u64 e0, e1;
            philox_words(a.seed, (u64)a.it, sid, SLOT_GJ + (u32)k, e0, e1);
            const double rr = det_sqrt(-2.0 * det_log(w2uniform_open(e0)));
            double sn, cs;
            det_sincos2pi(w2uniform(e1), sn, cs);
            const double pc = rr * cs;
            p[k] = pc;
            part = __builtin_fma(pc, pc, part);
            if (k + 64 < d) {
                const double ps = rr * sn;
                p[k + 64] = ps;
                part = __builtin_fma(ps, ps, part);
            }
        }
        joint0 = logp - 0.5 * group_sum<64>(part);                       // NJ:276 (loghamiltonian NJ:133-147)
        u64 w0, w1;
        philox_words(a.seed, (u64)a.it, sid, SLOT_GJS + 0u, w0, w1);     // NJ:279 randint(nminsteps, nmaxsteps): the call's first scalar draw
        left = a.hmc_min + (int)w2index(w0, (u64)(a.hmc_max - a.hmc_min));
        joint1 = joint0;
        done = left == 0;
    } else {
        joint0 = a.w.joint0[ch];
#pragma unroll 1
        for (int i = gl; i < d; i += 64) {
            const double pv = p[i] + he * gw[i];                         // NJ:166-167: the second half kick
            p[i] = pv;
            part = __builtin_fma(pv, pv, part);
        }
        joint1 = logp - 0.5 * group_sum<64>(part);
        nleap += 1;
        left -= 1;
        done = (joint1 - 1000.0 < joint0) || left == 0;                  // NJ:284-286
    }
    if (!done) {                                                         // NJ:160-163: half kick, drift
#pragma unroll 1
        for (int i = gl; i < d; i += 64) {
            const double rh = p[i] + he * gw[i];
            p[i] = rh;
            q[i] = q[i] + a.eps * rh;
        }
    }
    if (gl == 0) {
        *reinterpret_cast<int4 *>(a.w.ist + (size_t)ch * 4) = int4{done ? 0 : 1, 1, left, nleap};
        if (!done) a.w.joint0[ch] = joint0;
        else {
            a.qaux[(size_t)ch * 4] = joint1 - joint0;                    // qxy (NJ:290)
            double *s = a.gj + ((size_t)w * a.nt + t) * GJ_NSTATE;
            s[GJ_HITER] += 1.0;
            s[GJ_NLEAP] += (double)nleap;
        }
    }
}

// The listing's copy: row j of the callback's input = xs of listed chain list[j], one wave per row (gj_fill_kernel's own copy runs
// in its one block per 1024 chains: 16 blocks for 16384 chains of 1000 parameters).  The count is the one the listing just wrote.
__global__ __launch_bounds__(256) void gjw_rows_kernel(const double *xs, const int32_t *list, const long long *n, int d, double *rows)
{
    const long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= *n) return;
    const double *src = xs + (size_t)list[j] * d;
    double *dst = rows + (size_t)j * d;
    for (int i = (int)(threadIdx.x & 63); i < d; i += 64) dst[i] = src[i];
}

template <int OP, int RT>
void launch_product(ptmi_engine *h, const ProdArgs &p, long long bound)
{
    const long long brows = 4 * 16 * RT;                                  // rows per block of four waves
    hipLaunchKernelGGL((gjw_product_kernel<OP, RT, 8>), dim3((unsigned)((bound + brows - 1) / brows)), dim3(256), 0, h->stream, p);
}

template <int OP>
void launch_op(ptmi_engine *h, const ProdArgs &p, long long bound, long long expect)
{
    if (h->gj_diag) {
        hipLaunchKernelGGL((gjw_diag_kernel<OP>), dim3((unsigned)((bound + 3) / 4)), dim3(256), 0, h->stream, p);
        return;
    }
    // the launch shape as ptmi_dense_rows.hip's launch_shape picks it beyond 512-d: column groups of 8 tiles, two row tiles per wave
    // once there are blocks for every CU (the bits do not depend on the shape)
    if (expect >= 32768) launch_product<OP, 2>(h, p, bound);
    else launch_product<OP, 1>(h, p, bound);
}

}  // namespace

int ptmi_gjw_mark(ptmi_engine *h, const GjArgs &a)
{
    hipLaunchKernelGGL(gjw_mark_kernel, dim3((unsigned)((a.nch + 255) / 256)), dim3(256), 0, h->stream, (const double *)a.qaux, a.nch, a.w.ist);
    return PTMI_OK;
}

int ptmi_gjw_product(ptmi_engine *h, const GjArgs &a, int which, bool begin)
{
    const ptmi_config &c = h->cfg;
    ProdArgs p;
    memset(&p, 0, sizeof(p));
    p.T = a.tab + (size_t)which * a.d * a.d;
    p.d = a.d;
    p.list = a.w.list;
    p.beta = a.beta; p.temp_of = a.temp_of;
    long long bound, expect;
    if (begin) {                                                         // the count is still on the device: a grid for every chain
        p.nptr = a.w.n;
        bound = a.nch;
        const long long cyc = (long long)c.w_host + c.w_scam + c.w_am + c.w_de + c.w_hmc;
        expect = a.nch * c.w_hmc / (cyc > 0 ? cyc : 1);
    } else {
        p.n = a.n;
        bound = expect = a.n;
    }
    if (bound <= 0) return PTMI_OK;
    if (which == TG) {
        p.dlnl = a.dlnl; p.dlp = a.dlp;
        p.out = a.w.xs;
        if (a.dlp) launch_op<OP_GRAD_PRIOR>(h, p, bound, expect);
        else launch_op<OP_GRAD>(h, p, bound, expect);
        return PTMI_OK;
    }
    if (which == TF) {                                                   // forward (NJ:273): the pick's proposal row is its state x
        p.in = a.Q; p.out = a.w.q;
    } else {                                                             // backward: the next row (NJ:78), or the proposal (NJ:288)
        p.in = a.w.q; p.out = a.w.xs;
        if (!begin) { p.out_done = a.Q; p.ist = a.w.ist; }
    }
    launch_op<OP_ROW>(h, p, bound, expect);
    return PTMI_OK;
}

int ptmi_gjw_rows(ptmi_engine *h, const GjArgs &a, double *rows, long long bound)
{
    if (bound <= 0) return PTMI_OK;
    hipLaunchKernelGGL(gjw_rows_kernel, dim3((unsigned)((bound + 3) / 4)), dim3(256), 0, h->stream, (const double *)a.w.xs,
                       (const int32_t *)a.w.list, (const long long *)a.w.n, a.d, rows);
    return PTMI_OK;
}

int ptmi_gjw_step(ptmi_engine *h, const GjArgs &a)
{
    if (a.n <= 0) return PTMI_OK;
    hipLaunchKernelGGL(gjw_step_kernel, dim3((unsigned)((a.n + 3) / 4)), dim3(256), 0, h->stream, a);
    return PTMI_OK;
}
