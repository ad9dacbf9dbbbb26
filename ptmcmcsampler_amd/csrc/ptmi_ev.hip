// ptmi_ev.hip -- the ladder's summaries for the log-evidence, accumulated on the device (ptmi_ev_attach / ptmi_ev_update, include/ptmi.h).
// lnL [W][T] of every chain is in device memory behind every launch; once per sampled swap epoch ptmi_ev_update folds the lnL of every
// (walker, LOCAL RANK) cell into floating-point moments per temperature -- what thermodynamic integration (the mean and variance of lnL at
// every beta) and the stepping-stone estimator (the mean of exp(dbeta * lnL) at every beta) need, for every walker on its own, so that the
// walkers' scatter gives the standard error.  One thread per cell, rank fastest:
//
//     l = lnL[w][slot_of[w][r]];   a = dbeta[r] * l
//     !isfinite(l)            -> skipped += 1, nothing else
//     first sample of a cell  -> c = l; s1 = 0; s2 = 0; m = a; es = 1
//     else                    -> t = l - c; s1 += t; s2 += t * t
//                                a <= m: es += det_exp(a - m)        else: es = es * det_exp(m - a) + 1; m = a
//     taken += 1
//
// (the build has -ffp-contract=off: every operation rounds on its own; det_exp is ptmi_device.h's, the one ptmi_selftest_math op 1 holds
// to the oracle's bit for bit).  c, the cell's first sample, is the shift that keeps s2 meaningful where |lnL| is much larger than its
// spread; (m, es) is a running log-sum-exp: sum exp(a) = exp(m) * es with m the largest a so far.  Every cell is a sequential recurrence in
// time, one thread owns it in every call: no atomics, the result does not depend on the grid, and a host restatement of the rule
// reproduces it to the last bit.
//
// Layout: acc double [5][W][T] (planes c, s1, s2, m, es), cnt uint64 [2][W][T] (taken, skipped), both PLANE-major: thread i = w * T + r
// touches word i of every plane, so a wave's accesses are 64 consecutive words each.  The kernel reads slot_of and lnL of the handle and
// nothing else of it; 130 bytes per cell and call.
#include "ptmi_common.h"
#include <math.h>

struct ptmi_ev_state {
    double *acc;               // caller-owned [5][W][T]
    u64 *cnt;                  // caller-owned [2][W][T]
    double *d_dbeta;           // [T], the library's copy
};

namespace {

enum { EV_C = 0, EV_S1 = 1, EV_S2 = 2, EV_M = 3, EV_ES = 4 };

__global__ __launch_bounds__(256) void ev_update_kernel(const double *__restrict__ lnL, const int32_t *__restrict__ slot_of,
                                                        const double *__restrict__ dbeta, double *__restrict__ acc, u64 *__restrict__ cnt,
                                                        u32 nt, u32 ncell)
{
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= ncell) return;                                    // the grid's tail
    const u32 w = i / nt, r = i - w * nt;
    const u32 slot = (u32)slot_of[i];
    // (a slot outside the ladder is nothing the library writes: such a cell reads nothing and counts as skipped)
    const double l = slot < nt ? lnL[(size_t)w * nt + slot] : __builtin_nan("");
    if (!(fabs(l) < __builtin_inf())) {                        // -inf, +inf, NaN
        cnt[(size_t)ncell + i] += 1ull;
        return;
    }
    const double a = dbeta[r] * l;
    const u64 n = cnt[i];
    double *pc = acc + i, *ps1 = pc + (size_t)EV_S1 * ncell, *ps2 = pc + (size_t)EV_S2 * ncell, *pm = pc + (size_t)EV_M * ncell,
           *pes = pc + (size_t)EV_ES * ncell;
    if (n == 0) {
        *pc = l; *ps1 = 0.0; *ps2 = 0.0; *pm = a; *pes = 1.0;
    } else {
        const double t = l - *pc, m = *pm, es = *pes;
        *ps1 = *ps1 + t;
        *ps2 = *ps2 + t * t;
        const bool below = a <= m;
        const double e = det_exp(below ? a - m : m - a);      // one exponential for either branch
        *pes = below ? es + e : es * e + 1.0;
        if (!below) *pm = a;
    }
    cnt[i] = n + 1ull;
}

}  // namespace

void ptmi_ev_free(ptmi_engine *h)
{
    ptmi_ev_state *s = h->ev;
    if (!s) return;
    (void)hipFree(s->d_dbeta);
    delete s;
    h->ev = nullptr;
}

double *ptmi_ev_dbeta(ptmi_engine *h) { return h->ev ? h->ev->d_dbeta : nullptr; }

extern "C" {

int ptmi_ev_attach(ptmi_handle h, double *acc, uint64_t *cnt, const double *dbeta)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (h->ev) return fail(PTMI_EINVAL, "ptmi_ev_attach: already attached");
    if (!acc || ((uintptr_t)acc & 7) != 0) return fail(PTMI_EINVAL, "ptmi_ev_attach: acc must be non-NULL and 8-byte aligned");
    if (!cnt || ((uintptr_t)cnt & 7) != 0) return fail(PTMI_EINVAL, "ptmi_ev_attach: cnt must be non-NULL and 8-byte aligned");
    if (!dbeta) return fail(PTMI_EINVAL, "ptmi_ev_attach: dbeta is NULL");
    const ptmi_config &c = h->cfg;
    for (int r = 0; r < c.ntemps; ++r)
        if (!isfinite(dbeta[r]) || !(dbeta[r] >= 0.0))
            return fail(PTMI_EINVAL, "ptmi_ev_attach: dbeta[%d] must be finite and >= 0 (got %g)", r, dbeta[r]);
    if ((long long)c.nwalkers * c.ntemps >= (1ll << 31))
        return fail(PTMI_EUNSUPPORTED, "ptmi_ev_attach: %lld cells (32-bit cell index: below 2^31)", (long long)c.nwalkers * c.ntemps);
    ptmi_ev_state *s = new ptmi_ev_state();
    s->acc = acc;
    s->cnt = (u64 *)cnt;
    h->ev = s;
    const size_t bytes = sizeof(double) * (size_t)c.ntemps;
    hipError_t e = hipMalloc((void **)&s->d_dbeta, bytes);
    if (e == hipSuccess) e = hipMemcpy(s->d_dbeta, dbeta, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        ptmi_ev_free(h);
        return fail(PTMI_EHIP, "ptmi_ev_attach: %s", hipGetErrorString(e));
    }
    return PTMI_OK;
}

int ptmi_ev_update(ptmi_handle h)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    const ptmi_ev_state *s = h->ev;
    if (!s) return fail(PTMI_EINVAL, "ptmi_ev_update: no accumulators are attached (ptmi_ev_attach)");
    const ptmi_config &c = h->cfg;
    const u32 ncell = (u32)c.nwalkers * (u32)c.ntemps;
    hipLaunchKernelGGL(ev_update_kernel, dim3((ncell + 255u) / 256u), dim3(256), 0, h->stream, (const double *)h->buf.lnL,
                       (const int32_t *)h->buf.slot_of, (const double *)s->d_dbeta, s->acc, s->cnt, (u32)c.ntemps, ncell);
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

}  // extern "C"
