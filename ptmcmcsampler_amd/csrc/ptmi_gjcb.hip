// ptmi_gjcb.hip -- HMC on the split path with the caller's batched gradient callbacks (ptmi_gj_work_bytes / ptmi_gj_begin /
// ptmi_gj_step, include/ptmi.h).  HMCJump.__call__ of the reference (NJ:238-291, NJ = PTMCMCSampler/nutsjump.py; whitening NJ:51-54,
// 71-90; leapfrog NJ:149-169) for the chains whose pick of an iteration is HMC, cut into ROUNDS at the points where the reference calls
// its gradient: func_grad_white(q0), then once per leapfrog.  Between two rounds the caller evaluates logL, logp and their gradients on
// the listed rows; the chains' whitened position q and momentum p wait in the caller's work area.
//
// The arithmetic is GradJump::hmc of ptmi_gj.inc.h operation for operation (the oracle: hmc_call of oracle/ptmcmc_oracle.c) in the same
// lane layout -- G = ptmi_lanes_for_grad(ndim) lanes per chain, lane gl holding elements gl + G e -- so the dot products (strided fma
// partials, then the xor butterfly group_sum<G>), the momenta pairing (k, k + G) and the whitening products (per output element an fma
// chain over k ascending; d products for diagonal tables) give the fused kernels' bits.  The rows of a whitening product meet in LDS
// (the block's chains' input vectors), the tables are read from LDS where two fit beside them and through L2 otherwise.
//
// A round is three launches: the step (gj_step_kernel: every listed chain), then the listing (gj_count_kernel, gj_fill_kernel: the
// chains still moving in ascending chain slot -- block counts, then each block's offset from the counts before it and a ballot scan
// inside: no atomics, the order is the slots' order), then the count read back by the host.
#include "ptmi_common.h"

namespace {

constexpr int EMAX = 8;              // slots per lane: ptmi_lanes_for_grad keeps ndim <= 8 G
constexpr int VB = 2048;             // doubles of the block's vector staging area: (256 / G) chains x 8 G elements
constexpr int LB = 1024;             // chains per block of the listing kernels
enum { ST_ACT = 0, ST_STAGE = 1, ST_LEFT = 2, ST_NLEAP = 3 };   // int32 scalars of a chain in the work area

// The work area (ptmi_gj_work_bytes): q, p, xs [nch][d] doubles (whitened position and momentum; the row a listed chain hands to the
// callback), joint0 [nch], ist [nch][4] int32 (listed, stage, leapfrogs left, leapfrogs taken), list [nch] int32 (the round's chains),
// bcnt [nblk] int32 (the listing's block counts), n (int64: the round's count).
struct Work {
    double *q, *p, *xs, *joint0;
    int32_t *ist, *list, *bcnt;
    long long *n;
};
inline size_t al16(size_t b) { return (b + 15) & ~(size_t)15; }
inline size_t work_layout(long long nch, int d, char *base, Work *w)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += al16(bytes); return p; };
    const size_t nblk = (size_t)((nch + LB - 1) / LB);
    Work t;
    t.q = (double *)take(sizeof(double) * (size_t)nch * d);
    t.p = (double *)take(sizeof(double) * (size_t)nch * d);
    t.xs = (double *)take(sizeof(double) * (size_t)nch * d);
    t.joint0 = (double *)take(sizeof(double) * (size_t)nch);
    t.ist = (int32_t *)take(sizeof(int32_t) * 4 * (size_t)nch);
    t.list = (int32_t *)take(sizeof(int32_t) * (size_t)nch);
    t.bcnt = (int32_t *)take(sizeof(int32_t) * nblk);
    t.n = (long long *)take(sizeof(long long));
    if (w) *w = t;
    return off;
}

struct GjArgs {
    Work w;
    const double *tab;               // [3][d][d] whitening tables (GJT_*: 0 backward, 1 forward, 2 gradient)
    int diag;                        // the tables are diagonal (ptmi_create): a product is d multiplications
    int d, nt, W, ntg, temp0, walker0;
    long long nch, n;                // chains; the round's listed chains (gj_step_kernel)
    u64 seed;
    long long it;
    int hmc_min, hmc_max;
    double eps;
    double *Q;                       // the current proposal buffer
    double *qaux, *gj;
    const int32_t *temp_of;
    const double *beta;
    const double *lnl, *dlnl, *lp, *dlp;   // the callback's values of the round before (lp / dlp may be NULL: a flat prior)
};
enum { TB = 0, TF = 1, TG = 2 };

// Table t of the two a kernel uses: in LDS (staged at the kernel's start: slot 0 and 1 of `tl`) or the global copy.
template <bool TL>
__device__ __forceinline__ const double *table(const GjArgs &a, const double *tl, int t, int slot)
{
    return TL ? tl + (size_t)slot * a.d * a.d : a.tab + (size_t)t * a.d * a.d;
}

// out[i] = sum_k T[k][i] v[k], k ascending, one fma per term (GradJump::tab_vec); diagonal tables: T[i][i] v[i].  Every thread of the
// block calls it (the chain's input vector goes through LDS: vb = the chain's d doubles there).
template <int G>
__device__ __forceinline__ void tab_vec(const GjArgs &a, const double *T, const double (&v)[EMAX], double (&out)[EMAX], double *vb, int gl,
                                        bool on)
{
    const int d = a.d;
    if (a.diag) {
#pragma unroll
        for (int e = 0; e < EMAX; ++e) {
            const int i = gl + G * e;
            out[e] = i < d ? T[(size_t)i * d + i] * v[e] : 0.0;
        }
        return;
    }
    __syncthreads();                                     // the area's previous readers are done
#pragma unroll
    for (int e = 0; e < EMAX; ++e) {
        const int i = gl + G * e;
        if (i < d) vb[i] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EMAX; ++e) {
        const int i = gl + G * e;
        double acc = 0.0;
        if (on && i < d)
            for (int k = 0; k < d; ++k) acc = __builtin_fma(T[(size_t)k * d + i], vb[k], acc);
        out[e] = i < d ? acc : 0.0;
    }
}

// lane_dot of the oracle: strided fma partials over the lane's slots (pads are zeros), then the xor butterfly of the chain's G lanes
template <int G>
__device__ __forceinline__ double dot(const double (&x)[EMAX])
{
    double p = 0.0;
#pragma unroll
    for (int e = 0; e < EMAX; ++e) p = __builtin_fma(x[e], x[e], p);
    return group_sum<G>(p);
}

template <bool TL>
__device__ __forceinline__ void stage_tables(const GjArgs &a, double *tl, int t0, int t1)
{
    if (!TL) return;
    const int dd = a.d * a.d;
    for (int j = (int)threadIdx.x; j < dd; j += 256) {
        tl[j] = a.tab[(size_t)t0 * dd + j];
        tl[dd + j] = a.tab[(size_t)t1 * dd + j];
    }
    __syncthreads();
}

// ptmi_gj_begin: every chain whose pick is HMC (qaux[.][1], written by the proposal launch; its proposal row is its state x):
// q = forward(x), its row for the first round = backward(q)
template <int G, bool TL>
__global__ __launch_bounds__(256) void gj_begin_kernel(const GjArgs a)
{
    __shared__ double vbuf[VB];
    extern __shared__ __attribute__((aligned(16))) double tl[];
    constexpr int CPB = 256 / G;
    const int tid = (int)threadIdx.x, cl = tid / G, gl = tid % G, d = a.d;
    const long long ch = (long long)blockIdx.x * CPB + cl;
    const bool live = ch < a.nch;
    const bool on = live && a.qaux[(size_t)ch * 4 + 1] == (double)PTMI_J_HMC;
    stage_tables<TL>(a, tl, TF, TB);
    double x[EMAX], q[EMAX], xs[EMAX];
#pragma unroll
    for (int e = 0; e < EMAX; ++e) {
        const int i = gl + G * e;
        x[e] = on && i < d ? a.Q[(size_t)ch * d + i] : 0.0;
    }
    double *vb = vbuf + cl * (8 * G);
    tab_vec<G>(a, table<TL>(a, tl, TF, 0), x, q, vb, gl, on);         // forward (NJ:273)
    tab_vec<G>(a, table<TL>(a, tl, TB, 1), q, xs, vb, gl, on);        // backward: what func_grad_white(q0) evaluates (NJ:78)
    if (on) {
#pragma unroll
        for (int e = 0; e < EMAX; ++e) {
            const int i = gl + G * e;
            if (i < d) {
                a.w.q[(size_t)ch * d + i] = q[e];
                a.w.xs[(size_t)ch * d + i] = xs[e];
            }
        }
    }
    if (live && gl == 0) {
        int32_t *s = a.w.ist + (size_t)ch * 4;
        *reinterpret_cast<int4 *>(s) = int4{on ? 1 : 0, 0, 0, 0};
    }
}

// One round: the callback's values of listed chain j = row j.  First round of a chain: logp0 and the whitened gradient, the momenta,
// joint0 and nsteps, then the first half kick and drift; later rounds: the second half kick, joint1 and the guard; then either the next
// half kick and drift (listed again) or the end of the call (the proposal, qxy, the jump state).
template <int G, bool TL>
__global__ __launch_bounds__(256) void gj_step_kernel(const GjArgs a)
{
    __shared__ double vbuf[VB];
    extern __shared__ __attribute__((aligned(16))) double tl[];
    constexpr int CPB = 256 / G;
    const int tid = (int)threadIdx.x, cl = tid / G, gl = tid % G, d = a.d;
    const long long j = (long long)blockIdx.x * CPB + cl;
    const bool live = j < a.n;
    const long long ch = live ? (long long)a.w.list[j] : 0;
    stage_tables<TL>(a, tl, TG, TB);
    const int t = a.temp_of[ch];
    const double beta = a.beta[t];
    const int w = (int)(ch / a.nt);
    const u32 sid = (u32)((u64)(a.walker0 + w) * (u32)a.ntg) + (u32)(a.temp0 + t);
    const int4 st = *reinterpret_cast<const int4 *>(a.w.ist + (size_t)ch * 4);
    double g[EMAX], gw[EMAX], q[EMAX], p[EMAX];
#pragma unroll
    for (int e = 0; e < EMAX; ++e) {
        const int i = gl + G * e;
        const bool in = live && i < d;
        const double gl_ = in ? a.dlnl[(size_t)j * d + i] : 0.0;
        const double gp = (in && a.dlp) ? a.dlp[(size_t)j * d + i] : 0.0;
        g[e] = in ? beta * gl_ + gp : 0.0;                            // NJ:82-86: beta * dlnL + dlnp (the built-in priors: + 0.0)
        q[e] = in ? a.w.q[(size_t)ch * d + i] : 0.0;
        p[e] = (in && st.y) ? a.w.p[(size_t)ch * d + i] : 0.0;
    }
    double *vb = vbuf + cl * (8 * G);
    tab_vec<G>(a, table<TL>(a, tl, TG, 0), g, gw, vb, gl, live);      // the gradient in the whitened coordinates (NJ:87-88)
    const double logp = live ? beta * a.lnl[j] + (a.lp ? a.lp[j] : 0.0) : 0.0;
    const double he = 0.5 * a.eps;
    double joint0 = 0.0, joint1 = 0.0;
    int left = st.z, nleap = st.w;
    bool done;
    if (st.y == 0) {
        // GradJump::momenta, block 0 (NJ:92-94): directions k and k + G share one Box-Muller
#pragma unroll
        for (int e = 0; e < EMAX; e += 2) {
            const int k = gl + G * e;
            if (live && k < d) {
                u64 e0, e1;
                philox_words(a.seed, (u64)a.it, sid, SLOT_GJ + (u32)k, e0, e1);
                const double rr = det_sqrt(-2.0 * det_log(w2uniform_open(e0)));
                double sn, cs;
                det_sincos2pi(w2uniform(e1), sn, cs);
                p[e] = rr * cs;
                if (e + 1 < EMAX && k + G < d) p[e + 1] = rr * sn;
            }
        }
        joint0 = logp - 0.5 * dot<G>(p);                               // NJ:276 (loghamiltonian NJ:133-147)
        u64 w0, w1;
        philox_words(a.seed, (u64)a.it, sid, SLOT_GJS + 0u, w0, w1);   // NJ:279 randint(nminsteps, nmaxsteps): the call's first scalar draw
        left = a.hmc_min + (int)w2index(w0, (u64)(a.hmc_max - a.hmc_min));
        joint1 = joint0;
        done = left == 0;
    } else {
        joint0 = a.w.joint0[ch];
#pragma unroll
        for (int e = 0; e < EMAX; ++e) p[e] = p[e] + he * gw[e];          // NJ:166-167: the second half kick
        joint1 = logp - 0.5 * dot<G>(p);
        nleap += 1;
        left -= 1;
        done = (joint1 - 1000.0 < joint0) || left == 0;                  // NJ:284-286
    }
    if (!done) {                                                         // NJ:160-163: half kick, drift
#pragma unroll
        for (int e = 0; e < EMAX; ++e) {
            const double rh = p[e] + he * gw[e];
            p[e] = rh;
            q[e] = q[e] + a.eps * rh;
        }
    }
    double xs[EMAX];
    tab_vec<G>(a, table<TL>(a, tl, TB, 1), q, xs, vb, gl, live);        // backward: the next row, or the proposal (NJ:288)
    if (!live) return;
#pragma unroll
    for (int e = 0; e < EMAX; ++e) {
        const int i = gl + G * e;
        if (i >= d) continue;
        if (done) {
            a.Q[(size_t)ch * d + i] = xs[e];
        } else {
            a.w.q[(size_t)ch * d + i] = q[e];
            a.w.p[(size_t)ch * d + i] = p[e];
            a.w.xs[(size_t)ch * d + i] = xs[e];
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

// The listing: block b counts the listed chains of slots [b LB, (b + 1) LB) ...
__global__ __launch_bounds__(LB) void gj_count_kernel(const int32_t *ist, long long nch, int32_t *bcnt)
{
    const long long ch = (long long)blockIdx.x * LB + threadIdx.x;
    const int c = __syncthreads_count(ch < nch && ist[(size_t)ch * 4 + ST_ACT] != 0);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = c;
}
// ... and writes them, in slot order, to list[] and their rows to rows[] from its offset (the counts of the blocks before it): a
// block's chains take consecutive entries, so its rows are one contiguous span.  The last block writes the total.
__global__ __launch_bounds__(LB) void gj_fill_kernel(const int32_t *ist, long long nch, const int32_t *bcnt, const double *xs, int d,
                                                     int32_t *list, double *rows, long long *n)
{
    __shared__ long long part[LB / 64];
    __shared__ int wtot[LB / 64];
    __shared__ int32_t lch[LB];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    long long s = 0;
    for (int b = tid; b < (int)blockIdx.x; b += LB) s += bcnt[b];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) part[wv] = s;
    const long long ch = (long long)blockIdx.x * LB + tid;
    const bool act = ch < nch && ist[(size_t)ch * 4 + ST_ACT] != 0;
    const u64 mask = __ballot(act);
    if (lane == 0) wtot[wv] = __popcll(mask);
    __syncthreads();
    long long base = 0;
    int off = 0, m = 0;
    for (int k = 0; k < LB / 64; ++k) {
        base += part[k];
        if (k < wv) off += wtot[k];
        m += wtot[k];
    }
    const int r = off + __popcll(mask & ((1ull << lane) - 1ull));
    if (act) {
        list[base + r] = (int32_t)ch;
        lch[r] = (int32_t)ch;
    }
    __syncthreads();
    double *dst = rows + (size_t)base * d;
    for (long long k = tid; k < (long long)m * d; k += LB) {
        const int c = (int)(k / d), i = (int)(k - (long long)c * d);
        dst[k] = xs[(size_t)lch[c] * d + i];
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) *n = base + m;
}


// tables in LDS when two fit beside the staging area in the default 64 KB (ndim <= 55); diagonal tables are read where they are
bool tables_in_lds(const ptmi_engine *h) { return !h->gj_diag && 2.0 * 8.0 * h->cfg.ndim * h->cfg.ndim + 8.0 * VB <= 65536.0; }

template <int G, bool TL>
void launch_g(ptmi_engine *h, const GjArgs &a, bool begin, unsigned grid)
{
    const size_t lds = TL ? sizeof(double) * 2 * (size_t)a.d * a.d : 0;
    if (begin) hipLaunchKernelGGL((gj_begin_kernel<G, TL>), dim3(grid), dim3(256), lds, h->stream, a);
    else hipLaunchKernelGGL((gj_step_kernel<G, TL>), dim3(grid), dim3(256), lds, h->stream, a);
}
template <int G>
void launch_t(ptmi_engine *h, const GjArgs &a, bool begin, unsigned grid)
{
    if (tables_in_lds(h)) launch_g<G, true>(h, a, begin, grid);
    else launch_g<G, false>(h, a, begin, grid);
}

GjArgs make_gj_args(ptmi_engine *h, void *work)
{
    const ptmi_config &c = h->cfg;
    GjArgs a;
    memset(&a, 0, sizeof(a));
    a.nch = (long long)c.nwalkers * c.ntemps;
    work_layout(a.nch, c.ndim, (char *)work, &a.w);
    a.tab = h->d_gj_tab; a.diag = h->gj_diag;
    a.d = c.ndim; a.nt = c.ntemps; a.W = c.nwalkers; a.ntg = c.ntemps_global; a.temp0 = c.temp0; a.walker0 = c.walker0;
    a.seed = c.seed; a.it = h->gj_iter; a.hmc_min = c.hmc_min; a.hmc_max = c.hmc_max; a.eps = c.hmc_eps;
    a.Q = (h->q_cur && h->buf.Q2) ? h->buf.Q2 : h->buf.Q;
    a.qaux = h->buf.qaux; a.gj = h->buf.gj; a.temp_of = h->buf.temp_of; a.beta = h->d_beta;
    return a;
}

int launch(ptmi_engine *h, const GjArgs &a, bool begin)
{
    const long long cnt = begin ? a.nch : a.n;
    const int G = h->G;
    const unsigned grid = (unsigned)((cnt + 256 / G - 1) / (256 / G));
    if (grid == 0) return PTMI_OK;
    if (G == 4) launch_t<4>(h, a, begin, grid);
    else if (G == 16) launch_t<16>(h, a, begin, grid);
    else if (G == 64) launch_t<64>(h, a, begin, grid);
    else return fail(PTMI_EUNSUPPORTED, "gradient stage: no kernel for %d lanes per chain", G);
    return PTMI_OK;
}

// the listing of the round and its count on the host (the round's one synchronisation)
int list_round(ptmi_engine *h, const GjArgs &a, double *rows, int64_t *n)
{
    const unsigned nblk = (unsigned)((a.nch + LB - 1) / LB);
    hipLaunchKernelGGL(gj_count_kernel, dim3(nblk), dim3(LB), 0, h->stream, (const int32_t *)a.w.ist, a.nch, a.w.bcnt);
    hipLaunchKernelGGL(gj_fill_kernel, dim3(nblk), dim3(LB), 0, h->stream, (const int32_t *)a.w.ist, a.nch, (const int32_t *)a.w.bcnt,
                       (const double *)a.w.xs, a.d, a.w.list, rows, a.w.n);
    HIPCHK(hipGetLastError());
    if (!h->h_gj_n) HIPCHK(hipHostMalloc((void **)&h->h_gj_n, sizeof(long long)));
    HIPCHK(hipMemcpyAsync(h->h_gj_n, a.w.n, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *n = (int64_t)*h->h_gj_n;
    h->gj_n = *n;
    h->gj_phase = *n > 0 ? PTMI_GJ_ROUNDS : PTMI_GJ_DONE;
    return PTMI_OK;
}

}  // namespace

// Does the handle's split path serve HMC through callbacks?  (0 = yes, else the refusal's code with the message set.)
int ptmi_gj_split_check(const ptmi_engine *h)
{
    const ptmi_config &c = h->cfg;
    if (c.w_nuts > 0) return fail(PTMI_EUNSUPPORTED, "the split path does not serve NUTS (w_nuts=%d): batched gradient callbacks run HMC only", c.w_nuts);
    if (c.w_hmc > 0 && !ptmi_split_rows_ok(h))
        return fail(PTMI_EUNSUPPORTED, "HMC on the split path runs on the row kernels only (PTMI_SPLIT_ROWS=0 or a handle without room for the AM increments)");
    return PTMI_OK;
}

extern "C" {

int ptmi_gj_work_bytes(ptmi_handle h, size_t *bytes)
{
    if (!h || !bytes) return fail(PTMI_EINVAL, "NULL argument");
    *bytes = work_layout((long long)h->cfg.nwalkers * h->cfg.ntemps, h->cfg.ndim, nullptr, nullptr);
    return PTMI_OK;
}

int ptmi_gj_begin(ptmi_handle h, int64_t iter, void *work, double *rows, int64_t *n)
{
    if (!h || !work || !rows || !n) return fail(PTMI_EINVAL, "NULL argument");
    if (h->cfg.w_hmc <= 0 || !h->d_gj_tab) return fail(PTMI_EINVAL, "ptmi_gj_begin: the handle has no HMC in its cycle (w_hmc)");
    if (int rc = ptmi_gj_split_check(h)) return rc;
    if (h->dev_iter) return fail(PTMI_EUNSUPPORTED, "ptmi_gj_begin: the gradient stage reads its count on the host: not in ptmi_device_iter mode");
    if (h->gj_phase != PTMI_GJ_PENDING || h->gj_iter != (long long)iter)
        return fail(PTMI_EINVAL, "ptmi_gj_begin(%lld): no proposals of that iteration wait for their gradient stage (%s)", (long long)iter,
                    h->gj_phase == PTMI_GJ_PENDING ? "the proposals are another iteration's" : "call it once, after ptmi_propose / ptmi_accept_propose");
    if (((uintptr_t)work & 15) != 0) return fail(PTMI_EINVAL, "ptmi_gj_begin: the work area must be 16-byte aligned");
    h->gj_work = work;
    GjArgs a = make_gj_args(h, work);
    if (int rc = launch(h, a, true)) return rc;
    return list_round(h, a, rows, n);
}

int ptmi_gj_step(ptmi_handle h, void *work, const double *lnl, const double *dlnl, const double *lp, const double *dlp, double *rows,
                 int64_t *n)
{
    if (!h || !work || !lnl || !dlnl || !rows || !n) return fail(PTMI_EINVAL, "NULL argument");
    if ((lp == nullptr) != (dlp == nullptr)) return fail(PTMI_EINVAL, "ptmi_gj_step: lp and dlp are both given or both NULL (a flat prior)");
    if (h->gj_phase != PTMI_GJ_ROUNDS) return fail(PTMI_EINVAL, "ptmi_gj_step: no gradient round is open (ptmi_gj_begin first; the stage ends when n comes back 0)");
    if (work != h->gj_work) return fail(PTMI_EINVAL, "ptmi_gj_step: not the work area ptmi_gj_begin was given");
    GjArgs a = make_gj_args(h, work);
    a.n = h->gj_n;
    a.lnl = lnl; a.dlnl = dlnl; a.lp = lp; a.dlp = dlp;
    if (int rc = launch(h, a, false)) return rc;
    return list_round(h, a, rows, n);
}

}  // extern "C"
