// ptmi_best.hip -- the best-fit row of EVERY cold chain, tracked on the device (ptmi_best_attach / ptmi_best_update, include/ptmi.h):
// per walker the row with the largest lnprob = beta0 * lnL + lp (plane 0, MAP) and the row with the largest lnL (plane 1, ML) over
// ALL iterations, where ptmi_samples.hip keeps the best of a few dozen snapshots.  The AM ring (ptmi_buffers.AM, [W][cov_update][ndim])
// holds the rank-0 row of every walker for every iteration of the current covariance period, AMaux its lnL and lp -- of every
// iteration, stored or not.  Going through the iterations in ascending order a candidate replaces the held best iff its score is not
// NaN and (nothing is held or score > held): the strict IEEE comparison, so the earliest iteration with the maximum wins, 0.0 and
// -0.0 tie, a NaN never wins, and the state does not depend on how a run is cut into calls.
//
// best_rows_kernel: one wave per walker, four per 256-thread block.  Scan: lane l takes iterations klo + l, klo + l + 64, ... and
// loads the 16 bytes of (lnL, lp) at once -- a wave-instruction reads 1 KB of consecutive memory, four of them in flight per turn of
// the unrolled loop -- keeping its best (score, k) of both planes, k = 0 for "none".  Reduce: a butterfly of __shfl_xor per plane
// under the order (score descending by >, then k ascending; "none" loses to anything), total on non-NaN scores, so the wave's winner
// is the sequential rule's.  Compare and copy: the held best is read once per wave; only where a plane improved the wave walks back
// through AMflag 64 words per step to the stored row (ptmi_am_expand's rule, as samples_gather_kernel), copies it with the
// permutation of the exact 4-lane shape's row format on the stores, and writes (score, lnL, lp) and the iteration.  Rows, lnL and lp
// move as 64-bit words.  The planes share nothing: a walker whose planes pick the same iteration copies the row twice.  No atomics,
// no LDS; the ring is only read.
#include "ptmi_common.h"
#define PTMI_RING_RANGE_ONLY       // this reader weighs no rows: no copy of hist_weight_kernel
#include "ptmi_ring_weight.h"      // ring_range
#include <math.h>

struct ptmi_best_state {
    double *rows;              // caller-owned [2][W][ndim], parameter order
    double *val;               // caller-owned [2][W][3]: score, lnL, lp
    int64_t *iters;            // caller-owned [2][W], -1 = nothing held
    double beta0;
};

namespace {

static_assert((AMROW_NEW | AMROW_KEY) == 3ull, "the flag bits sit in the low 32 bits of the word");

struct BestArgs {
    const u64 *AM;             // [W][cu][d] in the ring's row format
    const double2 *AMaux;      // [W][cu] of (lnL, lp)
    const AmFlag *flag;        // [W][cu], or nullptr: every row is stored
    u64 *rows, *val;
    long long *iters;
    double beta0;
    long long base;            // the iteration the ring's period starts behind
    int W, d, epl, cu, klo, khi;   // iterations base + klo .. base + khi, 1 <= klo <= khi <= cu
};

// iteration base + k, k in 1 .. cu, sits in ring row k % cu
__device__ __forceinline__ int ring_row(int k, int cu) { return k == cu ? 0 : k; }

// a lane's running best of one plane; k == 0: none yet.  Candidates come in ascending k: the strict > keeps the earliest maximum
__device__ __forceinline__ void keep(double &s, int &k, double cs, int ck)
{
    if (cs == cs && (k == 0 || cs > s)) { s = cs; k = ck; }
}

// the better of two lanes' bests: score descending by >, then k ascending; none loses to anything
__device__ __forceinline__ void wave_best(double &s, int &k)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double os = __shfl_xor(s, off);
        const int ok = __shfl_xor(k, off);
        if (ok != 0 && (k == 0 || os > s || (os == s && ok < k))) { s = os; k = ok; }
    }
}

__global__ __launch_bounds__(256) void best_rows_kernel(const BestArgs a)
{
    const int wv = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (wv >= a.W) return;                                         // wave-uniform
    const int lane = threadIdx.x & 63;
    const size_t w = (size_t)wv;
    const int cu = a.cu, d = a.d, khi = a.khi;
    const double beta0 = a.beta0;
    const double2 *ax = a.AMaux + w * cu;

    // scan
    double s[2] = {0.0, 0.0};
    int kb[2] = {0, 0};
    int k = a.klo + lane;
    for (; khi - k >= 192; k += 256) {                             // four loads in flight
        double2 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ax[ring_row(k + 64 * j, cu)];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            keep(s[0], kb[0], beta0 * v[j].x + v[j].y, k + 64 * j);   // the product is rounded, then the sum (-ffp-contract=off)
            keep(s[1], kb[1], v[j].x, k + 64 * j);
        }
    }
    for (; k <= khi; k += 64) {
        const double2 v = ax[ring_row(k, cu)];
        keep(s[0], kb[0], beta0 * v.x + v.y, k);
        keep(s[1], kb[1], v.x, k);
    }

    // reduce, compare, copy
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        wave_best(s[p], kb[p]);
        const size_t cell = (size_t)p * a.W + w;
        const long long held_it = a.iters[cell];                   // one address per wave
        const double held = __longlong_as_double((long long)a.val[cell * 3]);
        const bool better = kb[p] != 0 && (held_it < 0 || s[p] > held);
        if (__ballot(better) == 0) continue;                       // every lane holds the wave's winner: all or none
        const int kw = __builtin_amdgcn_readfirstlane(kb[p]);
        int r = kw;                                                // the stored row iteration kw stands for
        if (a.flag) {
            const unsigned *fw = reinterpret_cast<const unsigned *>(a.flag + w * cu);      // the low half of every word holds NEW and KEY
            for (;;) {
                const int kk = r - lane;
                const bool hit = kk >= 1 && (fw[2 * (size_t)ring_row(kk, cu)] & 3u) != 0;
                const unsigned long long m = __ballot(hit);
                if (m) { r -= __ffsll(m) - 1; break; }
                r -= 64;
                if (r < 1) { r = 1; break; }                       // (ring row 1 of a period is a KEY row: not reached)
            }
        }
        const u64 *src = a.AM + (w * cu + ring_row(r, cu)) * d;
        u64 *dst = a.rows + cell * d;
        for (int q = lane; q < d; q += 64) dst[am_inv(q, a.epl)] = src[q];
        const u64 *own = reinterpret_cast<const u64 *>(ax + ring_row(kw, cu));              // lnL and lp of iteration kw itself
        if (lane == 0) {
            a.val[cell * 3] = (u64)__double_as_longlong(s[p]);
            a.iters[cell] = a.base + kw;
        } else if (lane < 3) {
            a.val[cell * 3 + lane] = own[lane - 1];
        }
    }
}

}  // namespace

void ptmi_best_free(ptmi_engine *h)
{
    delete h->best;
    h->best = nullptr;
}

extern "C" {

int ptmi_best_attach(ptmi_handle h, double *rows, double *val, int64_t *iters, double beta0)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (h->best) return fail(PTMI_EINVAL, "ptmi_best_attach: already attached");
    if (!rows || ((uintptr_t)rows & 7) != 0) return fail(PTMI_EINVAL, "ptmi_best_attach: rows must be non-NULL and 8-byte aligned");
    if (!val || ((uintptr_t)val & 7) != 0) return fail(PTMI_EINVAL, "ptmi_best_attach: val must be non-NULL and 8-byte aligned");
    if (!iters || ((uintptr_t)iters & 7) != 0) return fail(PTMI_EINVAL, "ptmi_best_attach: iters must be non-NULL and 8-byte aligned");
    if (!h->buf.AMaux) return fail(PTMI_EINVAL, "ptmi_best_attach: needs a handle with AMaux (lnL and lp beside the ring's rows)");
    if (!isfinite(beta0) || !(beta0 > 0.0)) return fail(PTMI_EINVAL, "ptmi_best_attach: beta0 must be finite and positive (got %g)", beta0);
    ptmi_best_state *s = new ptmi_best_state();
    s->rows = rows;
    s->val = val;
    s->iters = iters;
    s->beta0 = beta0;
    h->best = s;
    return PTMI_OK;
}

int ptmi_best_update(ptmi_handle h, int64_t iter_lo, int64_t iter_hi)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    const ptmi_best_state *s = h->best;
    if (!s) return fail(PTMI_EINVAL, "ptmi_best_update: nothing is attached (ptmi_best_attach)");
    long long base;
    if (int r = ring_range(h, "ptmi_best_update", iter_lo, iter_hi, &base)) return r == RING_IDLE ? PTMI_OK : r;
    if (!h->buf.AMaux || ((uintptr_t)h->buf.AMaux & 15) != 0)
        return fail(PTMI_EINVAL, "ptmi_best_update: the handle has no AMaux buffer, or one that is not 16-byte aligned");
    const ptmi_config &c = h->cfg;
    BestArgs a;
    a.AM = (const u64 *)h->buf.AM; a.AMaux = (const double2 *)h->buf.AMaux; a.flag = (const AmFlag *)h->buf.AMflag;
    a.rows = (u64 *)s->rows; a.val = (u64 *)s->val; a.iters = (long long *)s->iters;
    a.beta0 = s->beta0; a.base = base;
    a.W = c.nwalkers; a.d = c.ndim; a.epl = am_row_epl(h->G, h->EPL); a.cu = c.cov_update;
    a.klo = (int)(iter_lo - base); a.khi = (int)(iter_hi - base);
    hipLaunchKernelGGL(best_rows_kernel, dim3((unsigned)((c.nwalkers + 3) / 4)), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

}  // extern "C"
