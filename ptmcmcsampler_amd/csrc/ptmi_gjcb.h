// ptmi_gjcb.h -- what the two units of the callback path's gradient stage share (ptmi_gjcb.hip: ndim <= 512, HMC and NUTS;
// ptmi_gjcb_wide.hip: 512 < ndim <= 2048, HMC): the caller's work area, the kernels' arguments, the wide unit's launches.
#pragma once
#include "ptmi_common.h"

constexpr int GJ_LB = 1024;          // chains per block of the listing kernels
enum { ST_ACT = 0, ST_STAGE = 1, ST_LEFT = 2, ST_NLEAP = 3 };   // int32 scalars of a chain in the work area

// NUTS chains (handles with w_nuts > 0): vector slots of a call [slot][nch][d] -- the initial point, its gradient and the step-size
// search's momenta, the sample, the two ends (t, r, g) -- then per stack height h the pending left subtree's far end (t, r) and candidate t
// (its candidate gradient, which the fused kernels carry, is never read: not kept) ...
enum { NV_Q0 = 0, NV_G0 = 1, NV_R0 = 2, NV_SAMPLE = 3, NV_TM = 4, NV_RM = 5, NV_GM = 6, NV_TP = 7, NV_RP = 8, NV_GP = 9, NV_TOP = 10 };
enum { NL_FAR_T = 0, NL_FAR_R = 1, NL_CAND_T = 2, NL_VECS = 3 };
// ... the call's doubles [nch][ND_N] (the pending leapfrog's step, logp0, the search's joint of (q0, r0), its k and eps, the call's joint,
// logu, lnprob, n) and int32 [nch][NI_N] (phase, draws, leapfrogs, tree height j, direction, pending heights, the search's loop turn and
// flags), and the stack's scalars [nch][levels][4] (logp, n, alpha, nalpha)
enum { ND_LEPS = 0, ND_LOGP0 = 1, ND_FJ0 = 2, ND_FK = 3, ND_FEPS = 4, ND_JOINT = 5, ND_LOGU = 6, ND_LNPROB = 7, ND_N = 8, ND_NSC = 9 };
enum { NI_PHASE = 0, NI_NM = 1, NI_NS = 2, NI_NLEAP = 3, NI_J = 4, NI_DIR = 5, NI_PEND = 6, NI_LOOP = 7, NI_UP = 8, NI_GINF = 9, NI_NSC = 10 };

// The work area (ptmi_gj_work_bytes): q, p, xs [nch][d] doubles (whitened position and momentum; the row a listed chain hands to the
// callback), joint0 [nch], ist [nch][4] int32 (listed, stage, leapfrogs left, leapfrogs taken), list [nch] int32 (the round's chains),
// bcnt [nblk] int32 (the listing's block counts), n (int64: the round's count); with NUTS (levels = nuts_maxdepth + 1 > 0) then nv
// [NV_TOP + 3 levels][nch][d], nd [nch][ND_NSC], ni [nch][NI_NSC], nst [nch][levels][4].
struct Work {
    double *q, *p, *xs, *joint0;
    int32_t *ist, *list, *bcnt;
    long long *n;
    double *nv, *nd, *nst;
    int32_t *ni;
};
inline size_t al16(size_t b) { return (b + 15) & ~(size_t)15; }
inline size_t work_layout(long long nch, int d, int levels, char *base, Work *w)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += al16(bytes); return p; };
    const size_t nblk = (size_t)((nch + GJ_LB - 1) / GJ_LB);
    Work t;
    t.q = (double *)take(sizeof(double) * (size_t)nch * d);
    t.p = (double *)take(sizeof(double) * (size_t)nch * d);
    t.xs = (double *)take(sizeof(double) * (size_t)nch * d);
    t.joint0 = (double *)take(sizeof(double) * (size_t)nch);
    t.ist = (int32_t *)take(sizeof(int32_t) * 4 * (size_t)nch);
    t.list = (int32_t *)take(sizeof(int32_t) * (size_t)nch);
    t.bcnt = (int32_t *)take(sizeof(int32_t) * nblk);
    t.n = (long long *)take(sizeof(long long));
    t.nv = t.nd = t.nst = nullptr;
    t.ni = nullptr;
    if (levels > 0) {
        t.nv = (double *)take(sizeof(double) * (size_t)(NV_TOP + NL_VECS * levels) * nch * d);
        t.nd = (double *)take(sizeof(double) * (size_t)ND_NSC * nch);
        t.ni = (int32_t *)take(sizeof(int32_t) * (size_t)NI_NSC * nch);
        t.nst = (double *)take(sizeof(double) * 4 * (size_t)levels * nch);
    }
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
    int levels, nuts_maxdepth, gj_nburn;   // NUTS: stack heights of the work area (0: an HMC-only handle), the cap, nburn of dual averaging
    double nuts_delta;
    double *Q;                       // the current proposal buffer
    double *qaux, *gj;
    const int32_t *temp_of;
    const double *beta;
    const double *lnl, *dlnl, *lp, *dlp;   // the callback's values of the round before (lp / dlp may be NULL: a flat prior)
};
enum { TB = 0, TF = 1, TG = 2 };

// ptmi_gjcb_wide.hip (512 < ndim <= 2048, HMC): the launches ptmi_gj_begin / ptmi_gj_step put around the listing
// every chain's ist = (its pick is HMC, 0, 0, 0)
int ptmi_gjw_mark(ptmi_engine *h, const GjArgs &a);
// the whitening product of table `which` over the listed chains.  begin: TF (Q -> q) and TB (q -> xs) over the list the listing has just
// written, its count read from the work area on the device; a round: TG (beta dlnl + dlp of row j -> xs of chain list[j]) and TB (q ->
// xs of the chains still moving, -> the proposal of those whose call ended) over the a.n chains of the round
int ptmi_gjw_product(ptmi_engine *h, const GjArgs &a, int which, bool begin);
// the listed chains' rows of xs into rows[] (at most `bound` of them; the count is the listing's, in the work area)
int ptmi_gjw_rows(ptmi_engine *h, const GjArgs &a, double *rows, long long bound);
// a round's step: one wave per listed chain
int ptmi_gjw_step(ptmi_engine *h, const GjArgs &a);
