// ptmi_gjcb.hip -- HMC and NUTS on the split path with the caller's batched gradient callbacks (ptmi_gj_work_bytes / ptmi_gj_begin /
// ptmi_gj_step, include/ptmi.h).  HMCJump.__call__ of the reference (NJ:238-291, NJ = PTMCMCSampler/nutsjump.py; whitening NJ:51-54,
// 71-90; leapfrog NJ:149-169) for the chains whose pick of an iteration is HMC, cut into ROUNDS at the points where the reference calls
// its gradient: func_grad_white(q0), then once per leapfrog.  Between two rounds the caller evaluates logL, logp and their gradients on
// the listed rows; the chains' whitened position q and momentum p wait in the caller's work area.
//
// NUTS (NUTSJump.__call__, NJ:654-840) is the same cut made in GradJump::nuts / build_tree / find_reasonable_epsilon: a per-chain state
// machine that stops at every leapfrog's gradient and resumes in the next round.  A round finishes the leapfrog whose gradient came in
// (the second half kick), then runs the call's control flow -- the step-size search, the doublings, a leaf's merges with the pending left
// subtrees, the stop criteria, the dual averaging -- until it needs the next gradient (half kick, drift, listed again) or the call ends
// (backward(sample) into the proposal).  Between rounds the call's vectors, scalars, draw counters and the stack of pending left subtrees
// wait in the work area (nuts_round below).
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
//
// 512 < ndim <= 2048 (HMC only): the same calls and work area with the kernels of ptmi_gjcb_wide.hip -- the whitening products on the
// matrix cores, one wave per listed chain in the step -- in the order wide_begin / wide_round below give them.
#include "ptmi_gjcb.h"

namespace {

constexpr int EMAX = 8;              // slots per lane: ptmi_lanes_for_grad keeps ndim <= 8 G for the kernels of this unit
constexpr int VB = 2048;             // doubles of the block's vector staging area: (256 / G) chains x 8 G elements
constexpr int LB = GJ_LB;            // chains per block of the listing kernels
// (the work area, its scalars' names and the kernels' arguments: ptmi_gjcb.h)
// what the gradient of a NUTS chain's round belongs to: the call's initial point, the search's first leapfrog (eps = 1), a turn of its
// halving loop, a turn of its doubling-or-halving loop, a leaf of the tree
enum { PH_FIRST = 0, PH_FRE1 = 1, PH_HALVE = 2, PH_DOUBLE = 3, PH_LEAF = 4 };

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

// ptmi_gj_begin: every chain whose pick is HMC or NUTS (qaux[.][1], written by the proposal launch; its proposal row is its state x):
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
    const double jt = live ? a.qaux[(size_t)ch * 4 + 1] : -1.0;
    const bool on = jt == (double)PTMI_J_HMC || jt == (double)PTMI_J_NUTS;
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

// two-vector dot of the oracle's lane_dot: strided fma partials, then the butterfly (GradJump::dot)
template <int G>
__device__ __forceinline__ double dot2(const double (&x)[EMAX], const double (&y)[EMAX])
{
    double p = 0.0;
#pragma unroll
    for (int e = 0; e < EMAX; ++e) p = __builtin_fma(x[e], y[e], p);
    return group_sum<G>(p);
}

// A NUTS chain's round (every lane of the chain runs it with the same scalars; no block-wide operation inside).  In: the position q and
// half-kicked momentum p of the leapfrog whose gradient gw (whitened) and value logp came in -- on the call's first round q = q0 and no
// leapfrog.  Out: true when the call ended (q = the sample, to be taken backward into the proposal), else q, p of the next leapfrog's
// drift (its gradient is the next round's).  GradJump::nuts / build_tree / find_reasonable_epsilon operation for operation.
template <int G>
struct NutsChain {
    const GjArgs &a;
    const long long ch;
    const int gl, d;
    const long long it;
    const u32 sid;
    int nm, ns;

    __device__ __forceinline__ double *vec(int slot) const { return a.w.nv + ((size_t)slot * a.nch + ch) * d; }
    __device__ __forceinline__ void vload(int slot, double (&v)[EMAX]) const
    {
        const double *s = vec(slot);
#pragma unroll
        for (int e = 0; e < EMAX; ++e) {
            const int i = gl + G * e;
            v[e] = i < d ? s[i] : 0.0;
        }
    }
    __device__ __forceinline__ void vstore(int slot, const double (&v)[EMAX]) const
    {
        double *s = vec(slot);
#pragma unroll
        for (int e = 0; e < EMAX; ++e) {
            const int i = gl + G * e;
            if (i < d) s[i] = v[e];
        }
    }
    __device__ __forceinline__ double *lscal(int h) const { return a.w.nst + ((size_t)ch * a.levels + h) * 4; }

    __device__ __forceinline__ void momenta(double (&r)[EMAX])           // GradJump::momenta (NJ:92-94)
    {
        const u32 block = (u32)nm++;
#pragma unroll
        for (int e = 0; e < EMAX; ++e) r[e] = 0.0;
#pragma unroll
        for (int e = 0; e < EMAX; e += 2) {
            const int k = gl + G * e;
            if (k < d) {
                u64 e0, e1;
                philox_words(a.seed, (u64)it, sid, SLOT_GJ + 4096u * block + (u32)k, e0, e1);
                const double rr = det_sqrt(-2.0 * det_log(w2uniform_open(e0)));
                double sn, cs;
                det_sincos2pi(w2uniform(e1), sn, cs);
                r[e] = rr * cs;
                if (e + 1 < EMAX && k + G < d) r[e + 1] = rr * sn;
            }
        }
    }
    __device__ __forceinline__ u64 scalar_word()
    {
        u64 w0, w1;
        philox_words(a.seed, (u64)it, sid, SLOT_GJS + (u32)ns++, w0, w1);
        return w0;
    }
    __device__ __forceinline__ double uniform() { return w2uniform(scalar_word()); }
    __device__ __forceinline__ double exponential() { return -det_log(w2uniform_open(scalar_word())); }
    __device__ __forceinline__ double joint_of(double logl, const double (&r)[EMAX]) const { return logl - 0.5 * dot2<G>(r, r); }
    __device__ __forceinline__ bool keep_going(const double (&tm)[EMAX], const double (&tp)[EMAX], const double (&rm)[EMAX],
                                               const double (&rp)[EMAX]) const                  // NJ:465-493
    {
        double dt[EMAX];
#pragma unroll
        for (int e = 0; e < EMAX; ++e) dt[e] = tp[e] - tm[e];
        const double x = dot2<G>(dt, rm), y = dot2<G>(dt, rp);
        return (x >= 0.0) & (y >= 0.0);
    }
    __device__ __forceinline__ bool any_inf(const double (&v)[EMAX]) const
    {
        bool fin = true;
#pragma unroll
        for (int e = 0; e < EMAX; ++e) fin = fin && !__builtin_isinf(v[e]);
        return !group_all<G>(fin);
    }
};

enum { PC_HALVE_TEST, PC_DOUBLE_TEST, PC_CALL_START, PC_DOUBLING, PC_LEAF, PC_TREE_DONE, PC_END };

template <int G>
__device__ bool nuts_round(const GjArgs &a, long long ch, int gl, u32 sid, double *stg, bool first, double logp, const double (&gw)[EMAX],
                           double (&q)[EMAX], double (&p)[EMAX])
{
    NutsChain<G> c{a, ch, gl, a.d, a.it, sid, 0, 0};
    double *nd = a.w.nd + (size_t)ch * ND_NSC;
    int32_t *ni = a.w.ni + (size_t)ch * NI_NSC;
    int phase = ni[NI_PHASE], nleap = ni[NI_NLEAP], j = ni[NI_J], dir = ni[NI_DIR], loop = ni[NI_LOOP], up = ni[NI_UP], ginf = ni[NI_GINF];
    u32 pend = (u32)ni[NI_PEND];
    c.nm = ni[NI_NM]; c.ns = ni[NI_NS];
    double leps = nd[ND_LEPS], logp0 = nd[ND_LOGP0], fj0 = nd[ND_FJ0], fk = nd[ND_FK], feps = nd[ND_FEPS], joint = nd[ND_JOINT],
           logu = nd[ND_LOGU], lnprob = nd[ND_LNPROB], nn = nd[ND_N];
    double st[GJ_NSTATE];
#pragma unroll
    for (int k = 0; k < GJ_NSTATE; ++k) st[k] = stg[k];
    if (first) {
        phase = PH_FIRST; nleap = 0; c.nm = 0; c.ns = 0;
    }
    // the leapfrog whose gradient came in: the second half kick (GradJump::leapfrog, NJ:166-167)
    double tg[EMAX], rg[EMAX], gg[EMAX];
    double lpp = logp;
    if (!first) {
        const double he = 0.5 * leps;
#pragma unroll
        for (int e = 0; e < EMAX; ++e) { tg[e] = q[e]; rg[e] = p[e] + he * gw[e]; gg[e] = gw[e]; }
        nleap += 1;
    }
    // what the next leapfrog starts from (theta, r, grad and its step), when the call goes on
    double lt[EMAX], lr[EMAX], lg[EMAX];
    // the subtree of the leaf (GradJump::Tree without cand_g)
    double far_t[EMAX], far_r[EMAX], cand_t[EMAX];
    double cur_logp = 0.0, cur_alpha = 0.0;
    long long cur_n = 0, cur_nalpha = 0;
    int cur_s = 0;
    double alpha = 0.0;
    long long nalpha = 1;
    bool done = false, leap = false;
    int pc;
    if (first) {
        // NJ:654-669: q0 = forward(x) came in with its gradient
        st[GJ_NITER] += 1.0;
        logp0 = logp;
        c.vstore(NV_Q0, q);
        c.vstore(NV_G0, gw);
        if (st[GJ_HAVE_EPS] == 0.0) {                                    // find_reasonable_epsilon: its first leapfrog at eps = 1
            double r0[EMAX];
            c.momenta(r0);
            c.vstore(NV_R0, r0);
            fj0 = c.joint_of(logp0, r0);
#pragma unroll
            for (int e = 0; e < EMAX; ++e) { lt[e] = q[e]; lr[e] = r0[e]; lg[e] = gw[e]; }
            leps = 1.0;
            phase = PH_FRE1;
            leap = true;
            pc = PC_END;
        } else {
            pc = PC_CALL_START;
        }
    } else if (phase == PH_FRE1) {
        ginf = c.any_inf(gg);                                            // not refreshed in the loop (NJ:449-452)
        fk = 1.0;
        loop = 0;
        pc = PC_HALVE_TEST;
    } else if (phase == PH_HALVE) {
        loop += 1;
        pc = PC_HALVE_TEST;
    } else if (phase == PH_DOUBLE) {
        loop += 1;
        pc = PC_DOUBLE_TEST;
    } else {
        pc = PC_LEAF;
    }
    double ap = 0.0;
    while (!leap && !done) {
        if (pc == PC_HALVE_TEST) {                                       // NJ:449-452, bounded at 100 turns
            if (loop < 100 && (__builtin_isinf(lpp) || ginf)) {
                fk *= 0.5;
                c.vload(NV_Q0, lt); c.vload(NV_R0, lr); c.vload(NV_G0, lg);
                leps = 1.0 * fk;
                phase = PH_HALVE;
                leap = true;
                continue;
            }
            feps = 0.5 * fk * 1.0;
            ap = det_exp(c.joint_of(lpp, rg) - fj0);
            up = ap > 0.5;
            loop = 0;
            pc = PC_DOUBLE_TEST;
            continue;
        }
        if (pc == PC_DOUBLE_TEST) {                                      // NJ:454-462, bounded at 100 turns
            if (phase == PH_DOUBLE) ap = det_exp(c.joint_of(lpp, rg) - fj0);
            if (loop < 100 && ((up ? ap : 1.0 / ap) > (up ? 0.5 : 2.0))) {
                feps = feps * (up ? 2.0 : 0.5);
                c.vload(NV_Q0, lt); c.vload(NV_R0, lr); c.vload(NV_G0, lg);
                leps = feps;
                phase = PH_DOUBLE;
                leap = true;
                continue;
            }
            st[GJ_EPS] = feps;
            st[GJ_MU] = det_log(10.0 * st[GJ_EPS]);
            st[GJ_HAVE_EPS] = 1.0;
            pc = PC_CALL_START;
            continue;
        }
        if (pc == PC_CALL_START) {                                       // NJ:671-700: momenta, joint, slice, the trajectory's ends
            double q0[EMAX], g0[EMAX], r0[EMAX];
            c.vload(NV_Q0, q0); c.vload(NV_G0, g0);
            c.momenta(r0);
            joint = c.joint_of(logp0, r0);
            logu = joint - c.exponential();
            lnprob = logp0;
            c.vstore(NV_SAMPLE, q0);
            c.vstore(NV_TM, q0); c.vstore(NV_RM, r0); c.vstore(NV_GM, g0);
            c.vstore(NV_TP, q0); c.vstore(NV_RP, r0); c.vstore(NV_GP, g0);
            j = 0;
            nn = 1.0;
            pc = PC_DOUBLING;
            continue;
        }
        if (pc == PC_DOUBLING) {                                         // NJ:716-730: a direction, the first leaf from that end
            dir = 2 * (int)(c.uniform() < 0.5) - 1;
            const int eb = dir == -1 ? NV_TM : NV_TP;
            c.vload(eb, lt); c.vload(eb + 1, lr); c.vload(eb + 2, lg);
            pend = 0;
            leps = (double)dir * st[GJ_EPS];
            phase = PH_LEAF;
            leap = true;
            continue;
        }
        if (pc == PC_LEAF) {                                             // build_tree: the leaf (NJ:506-530), then its merges
            const double jl = c.joint_of(lpp, rg);
            cur_n = logu < jl;
            cur_s = (logu - 1000.0) < jl;
#pragma unroll
            for (int e = 0; e < EMAX; ++e) { far_t[e] = tg[e]; far_r[e] = rg[e]; cand_t[e] = tg[e]; }
            cur_logp = lpp;
            const double ex = det_exp(jl - joint);
            cur_alpha = ex < 1.0 ? ex : 1.0;                             // Python's min(1.0, e): 1.0 when e is NaN
            cur_nalpha = 1;
            int h = 0;
            for (;;) {
                const int top_h = pend ? (int)__builtin_ctz(pend) : -1;
                if (top_h == h) {                                        // cur is the right sibling of the stack top
                    pend &= pend - 1u;
                    const double *ls = c.lscal(h);
                    const double t_logp = ls[0], t_n = ls[1], t_alpha = ls[2], t_nalpha = ls[3];
                    const long long tn = (long long)t_n;
                    const long long tot = tn + cur_n;
                    const double den = (double)tot > 1.0 ? (double)tot : 1.0;
                    const bool take_u = c.uniform() < (double)cur_n / den;
                    const int lb = NV_TOP + NL_VECS * h;
                    if (!take_u) {
                        c.vload(lb + NL_CAND_T, cand_t);
                        cur_logp = t_logp;
                    }
                    c.vload(lb + NL_FAR_T, far_t);
                    c.vload(lb + NL_FAR_R, far_r);
                    cur_n = tot;
                    const bool go = dir == 1 ? c.keep_going(far_t, tg, far_r, rg) : c.keep_going(tg, far_t, rg, far_r);
                    cur_s = cur_s && go;                                 // the popped tree has s = 1
                    cur_alpha = t_alpha + cur_alpha;
                    cur_nalpha = (long long)t_nalpha + cur_nalpha;
                    h += 1;
                    continue;
                }
                if (h == j) { pc = PC_TREE_DONE; break; }
                if (cur_s == 0) {
                    if (pend == 0) { pc = PC_TREE_DONE; break; }
                    h = top_h;
                    continue;
                }
                const int lb = NV_TOP + NL_VECS * h;                     // push: wait for the right sibling
                c.vstore(lb + NL_FAR_T, far_t);
                c.vstore(lb + NL_FAR_R, far_r);
                c.vstore(lb + NL_CAND_T, cand_t);
                if (gl == 0) {
                    double *ls = c.lscal(h);
                    ls[0] = cur_logp; ls[1] = (double)cur_n; ls[2] = cur_alpha; ls[3] = (double)cur_nalpha;
                }
                pend |= 1u << h;
#pragma unroll
                for (int e = 0; e < EMAX; ++e) { lt[e] = tg[e]; lr[e] = rg[e]; lg[e] = gg[e]; }
                leap = true;                                             // the next leaf, same direction and step
                break;
            }
            continue;
        }
        if (pc == PC_TREE_DONE) {                                        // NJ:731-802: the subtree's end, candidate, stop criterion
            const int eb = dir == -1 ? NV_TM : NV_TP, ob = dir == -1 ? NV_TP : NV_TM;
            c.vstore(eb, tg); c.vstore(eb + 1, rg); c.vstore(eb + 2, gg);
            if (cur_s == 1) {
                const double ratio = (double)cur_n / nn;
                if (c.uniform() < (1.0 < ratio ? 1.0 : ratio)) { c.vstore(NV_SAMPLE, cand_t); lnprob = cur_logp; }
            }
            nn = (double)((long long)nn + cur_n);
            double to[EMAX], ro[EMAX];
            c.vload(ob, to); c.vload(ob + 1, ro);
            const bool go = dir == -1 ? c.keep_going(tg, to, rg, ro) : c.keep_going(to, tg, ro, rg);
            const bool s = cur_s && go;
            alpha = cur_alpha;
            nalpha = cur_nalpha;
            j += 1;
            pc = (s && !(j > a.nuts_maxdepth)) ? PC_DOUBLING : PC_END;   // cap (not in the reference)
            continue;
        }
        // PC_END: dual averaging (NJ:805-816): gamma = 0.05, t0 = 10, kappa = 0.75
        const double it_call = st[GJ_NITER];
        double eta = 1.0 / (it_call + 10.0);
        st[GJ_HBAR] = (1.0 - eta) * st[GJ_HBAR] + eta * (a.nuts_delta - alpha / (double)nalpha);
        if (a.it <= (long long)a.gj_nburn) {
            st[GJ_EPS] = det_exp(st[GJ_MU] - det_sqrt(it_call) / 0.05 * st[GJ_HBAR]);
            eta = det_exp(-0.75 * det_log(it_call));
            st[GJ_EPSBAR] = det_exp((1.0 - eta) * det_log(st[GJ_EPSBAR]) + eta * det_log(st[GJ_EPS]));
        } else {
            st[GJ_EPS] = st[GJ_EPSBAR];
        }
        st[GJ_NLEAP] += (double)nleap;
        c.vload(NV_SAMPLE, q);
        done = true;
    }
    if (leap) {                                                          // GradJump::leapfrog up to the gradient: half kick, drift
        const double he = 0.5 * leps;
#pragma unroll
        for (int e = 0; e < EMAX; ++e) {
            const double rh = lr[e] + he * lg[e];
            p[e] = rh;
            q[e] = lt[e] + leps * rh;
        }
    }
    if (gl == 0) {
        ni[NI_PHASE] = phase; ni[NI_NM] = c.nm; ni[NI_NS] = c.ns; ni[NI_NLEAP] = nleap; ni[NI_J] = j; ni[NI_DIR] = dir;
        ni[NI_PEND] = (int32_t)pend; ni[NI_LOOP] = loop; ni[NI_UP] = up; ni[NI_GINF] = ginf;
        nd[ND_LEPS] = leps; nd[ND_LOGP0] = logp0; nd[ND_FJ0] = fj0; nd[ND_FK] = fk; nd[ND_FEPS] = feps; nd[ND_JOINT] = joint;
        nd[ND_LOGU] = logu; nd[ND_LNPROB] = lnprob; nd[ND_N] = nn;
#pragma unroll
        for (int k = 0; k < GJ_NSTATE; ++k) stg[k] = st[k];
        if (done) a.qaux[(size_t)ch * 4] = logp0 - lnprob;                // undoes the outer Hastings ratio (NJ:838)
    }
    return done;
}

// One round: the callback's values of listed chain j = row j.  First round of a chain: logp0 and the whitened gradient, the momenta,
// joint0 and nsteps, then the first half kick and drift; later rounds: the second half kick, joint1 and the guard; then either the next
// half kick and drift (listed again) or the end of the call (the proposal, qxy, the jump state).  NUTS: a NUTS chain's round is
// nuts_round's (handles with w_nuts > 0 run the kernel with NUTS = true; HMC-only handles the one without the branch).
template <int G, bool TL, bool NUTS>
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
    const bool nuts = NUTS && live && a.qaux[(size_t)ch * 4 + 1] == (double)PTMI_J_NUTS;
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
    if (nuts) {
        done = nuts_round<G>(a, ch, gl, sid, a.gj + ((size_t)w * a.nt + t) * GJ_NSTATE, st.y == 0, logp, gw, q, p);
    } else if (st.y == 0) {
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
    if (!nuts && !done) {                                                // NJ:160-163: half kick, drift
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
    if (gl == 0 && nuts) {                                               // (nuts_round wrote the call's state, qxy and the jump state)
        *reinterpret_cast<int4 *>(a.w.ist + (size_t)ch * 4) = int4{done ? 0 : 1, 1, 0, 0};
    } else if (gl == 0) {
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
    else if (a.levels > 0) hipLaunchKernelGGL((gj_step_kernel<G, TL, true>), dim3(grid), dim3(256), lds, h->stream, a);
    else hipLaunchKernelGGL((gj_step_kernel<G, TL, false>), dim3(grid), dim3(256), lds, h->stream, a);
}
template <int G>
void launch_t(ptmi_engine *h, const GjArgs &a, bool begin, unsigned grid)
{
    if (tables_in_lds(h)) launch_g<G, true>(h, a, begin, grid);
    else launch_g<G, false>(h, a, begin, grid);
}

// stack heights of the work area: the NUTS trees' 0..nuts_maxdepth, none for an HMC-only handle (today's layout)
int nuts_levels(const ptmi_config &c) { return c.w_nuts > 0 ? c.nuts_maxdepth + 1 : 0; }

GjArgs make_gj_args(ptmi_engine *h, void *work)
{
    const ptmi_config &c = h->cfg;
    GjArgs a;
    memset(&a, 0, sizeof(a));
    a.nch = (long long)c.nwalkers * c.ntemps;
    a.levels = nuts_levels(c);
    a.nuts_maxdepth = c.nuts_maxdepth; a.gj_nburn = c.gj_nburn; a.nuts_delta = c.nuts_delta;
    work_layout(a.nch, c.ndim, a.levels, (char *)work, &a.w);
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

// the listing's kernels: the chains still moving into list[] (and their count into the work area); copy: their rows of xs into rows[]
void list_kernels(ptmi_engine *h, const GjArgs &a, double *rows, bool copy)
{
    const unsigned nblk = (unsigned)((a.nch + LB - 1) / LB);
    hipLaunchKernelGGL(gj_count_kernel, dim3(nblk), dim3(LB), 0, h->stream, (const int32_t *)a.w.ist, a.nch, a.w.bcnt);
    hipLaunchKernelGGL(gj_fill_kernel, dim3(nblk), dim3(LB), 0, h->stream, (const int32_t *)a.w.ist, a.nch, (const int32_t *)a.w.bcnt,
                       (const double *)a.w.xs, copy ? a.d : 0, a.w.list, rows, a.w.n);
}

// the listing of the round and its count on the host (the round's one synchronisation)
int list_round(ptmi_engine *h, const GjArgs &a, double *rows, int64_t *n, long long bound)
{
    if (a.d > PTMI_GJ_REG_MAX) {                                           // wide rows: a wave per row copies them (ptmi_gjcb_wide.hip)
        list_kernels(h, a, rows, false);
        if (int rc = ptmi_gjw_rows(h, a, rows, bound)) return rc;
    } else {
        list_kernels(h, a, rows, true);
    }
    HIPCHK(hipGetLastError());
    if (!h->h_gj_n) HIPCHK(hipHostMalloc((void **)&h->h_gj_n, sizeof(long long)));
    HIPCHK(hipMemcpyAsync(h->h_gj_n, a.w.n, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *n = (int64_t)*h->h_gj_n;
    h->gj_n = *n;
    h->gj_phase = *n > 0 ? PTMI_GJ_ROUNDS : PTMI_GJ_DONE;
    return PTMI_OK;
}

// 512 < ndim <= 2048 (ptmi_gjcb_wide.hip).  begin: the HMC picks are listed FIRST, so that the row tiles of the forward and backward
// products hold picks only (their count stays on the device: the grid covers every chain and the blocks past the count leave); a round:
// the gradient product (into xs, free since the listing copied it out), the step, the backward product, the listing.
int wide_begin(ptmi_engine *h, const GjArgs &a, double *rows)
{
    if (int rc = ptmi_gjw_mark(h, a)) return rc;
    list_kernels(h, a, rows, false);
    if (int rc = ptmi_gjw_product(h, a, TF, true)) return rc;
    return ptmi_gjw_product(h, a, TB, true);
}
int wide_round(ptmi_engine *h, const GjArgs &a)
{
    if (int rc = ptmi_gjw_product(h, a, TG, false)) return rc;
    if (int rc = ptmi_gjw_step(h, a)) return rc;
    return ptmi_gjw_product(h, a, TB, false);
}

}  // namespace

// Does the handle's split path serve its gradient jumps (HMC, NUTS) through callbacks?  (0 = yes, else the refusal's code with the
// message set.)
int ptmi_gj_split_check(const ptmi_engine *h)
{
    const ptmi_config &c = h->cfg;
    if (c.w_nuts + c.w_hmc > 0 && !ptmi_split_rows_ok(h))
        return fail(PTMI_EUNSUPPORTED, "gradient jumps (HMC, NUTS) on the split path run on the row kernels only (PTMI_SPLIT_ROWS=0 or a handle without room "
                                       "for the AM increments)");
    return PTMI_OK;
}

extern "C" {

int ptmi_gj_work_bytes(ptmi_handle h, size_t *bytes)
{
    if (!h || !bytes) return fail(PTMI_EINVAL, "NULL argument");
    *bytes = work_layout((long long)h->cfg.nwalkers * h->cfg.ntemps, h->cfg.ndim, nuts_levels(h->cfg), nullptr, nullptr);
    return PTMI_OK;
}

int ptmi_gj_begin(ptmi_handle h, int64_t iter, void *work, double *rows, int64_t *n)
{
    if (!h || !work || !rows || !n) return fail(PTMI_EINVAL, "NULL argument");
    if (h->cfg.w_nuts + h->cfg.w_hmc <= 0 || !h->d_gj_tab)
        return fail(PTMI_EINVAL, "ptmi_gj_begin: the handle has no gradient jumps in its cycle (w_nuts + w_hmc)");
    if (int rc = ptmi_gj_split_check(h)) return rc;
    if (h->dev_iter) return fail(PTMI_EUNSUPPORTED, "ptmi_gj_begin: the gradient stage reads its count on the host: not in ptmi_device_iter mode");
    if (h->gj_phase != PTMI_GJ_PENDING || h->gj_iter != (long long)iter)
        return fail(PTMI_EINVAL, "ptmi_gj_begin(%lld): no proposals of that iteration wait for their gradient stage (%s)", (long long)iter,
                    h->gj_phase == PTMI_GJ_PENDING ? "the proposals are another iteration's" : "call it once, after ptmi_propose / ptmi_accept_propose");
    if (((uintptr_t)work & 15) != 0) return fail(PTMI_EINVAL, "ptmi_gj_begin: the work area must be 16-byte aligned");
    h->gj_work = work;
    GjArgs a = make_gj_args(h, work);
    if (int rc = a.d > PTMI_GJ_REG_MAX ? wide_begin(h, a, rows) : launch(h, a, true)) return rc;
    return list_round(h, a, rows, n, a.nch);
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
    if (int rc = a.d > PTMI_GJ_REG_MAX ? wide_round(h, a) : launch(h, a, false)) return rc;
    return list_round(h, a, rows, n, a.n);                               // (a round lists no more chains than the one before)
}

}  // extern "C"
