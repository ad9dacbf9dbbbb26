// ptmi_diag.hip -- the streaming sums behind the convergence diagnostics of EVERY cold chain (Gelman-Rubin R-hat, batch-means
// autocorrelation time / ESS; ptmi_diag_attach / ptmi_diag_update, include/ptmi.h; the estimates: ptmcmcsampler_amd/diagnostics.py).  The
// AM ring (ptmi_buffers.AM, [W][cov_update][ndim]) holds the rank-0 row of every walker for every iteration of the current covariance
// period; ptmi_update_cov and ptmi_hist_update read it once per period, this unit is a third reader.  One independent stream per
// (walker w, parameter j), in iteration order, every operation rounded on its own (the build has -ffp-contract=off: no fma):
//
//     if n == 0: c = x                       the stream's shift: its first counted sample
//     y = x - c
//     S1 += y;  S2 += y * y;  A += y;  n += 1
//     if n % b0 == 0:                        a level-0 batch is complete
//         k = n / b0;  t = A;  A = 0
//         for l = 0 .. L - 1:
//             Q[l] += t * t                  sum of squared batch sums at level l (batch length b0 << l)
//             if l == L - 1: break
//             if (k >> l) & 1: H[l] = t; break      first half of a pair: wait for its partner
//             t = H[l] + t                   the pair is a level l + 1 batch
//
// n and k are the same for every stream, so they are the CALLER's (n_done comes in with every call): the state is 2 L + 3 planes of
// [W][ndim] doubles in PARAMETER order -- c, S1, S2, A, Q[0 .. L - 1], H[0 .. L - 2] -- in one caller-owned buffer.  A stream is serial in
// time and touches nobody else's state: the sums do not depend on the launch geometry, on how a period is cut into calls, or on the ring
// mode (a row that was not stored repeats the last stored row before it and is added once per iteration), and a NumPy restatement
// reproduces them to the last bit.
//
// diag_rows_kernel: one thread per stream, thread g = w * ndim + p takes position p of walker w's ring rows (am_pos: position p holds
// parameter am_inv(p); undone where the state is loaded and stored), so a wave instruction reads 64 consecutive doubles of a row -- or the
// end of one walker's row and the start of the next walker's, whose flags then differ lane by lane.  UNR iterations are in flight per
// thread: the rows that were stored -- a row that was not stored is never requested -- then the serial sums; their flags (the low half
// of the 8-byte word of every walker and iteration, one address per walker: a broadcast) were requested a chunk earlier.  The count and
// the cascade's branches are wave-uniform (scalar registers); Q / H stay in vector registers because the loop over l is unrolled with
// uniform guards (an array indexed by a run-time l would go to scratch).
#include "ptmi_common.h"
#define PTMI_RING_RANGE_ONLY       // this reader weighs no rows: no copy of hist_weight_kernel
#include "ptmi_ring_weight.h"      // ring_range

struct ptmi_diag_state {
    double *acc;               // caller-owned [2 * nlevels + 3][W][ndim]
    int nlevels, batch0;
};

namespace {

constexpr int UNR = 8;                 // iterations in flight per thread
constexpr int LMAX = 16;               // levels at most

// iteration base + k, k in 1 .. cu, sits in ring row k % cu; of its flag word the low half is read, which holds NEW and KEY
static_assert((AMROW_NEW | AMROW_KEY) == 3ull, "the flag bits sit in the low 32 bits of the word");
__device__ __forceinline__ unsigned flag_word(const AmFlag *fw, int k, int cu) { return reinterpret_cast<const unsigned *>(fw)[2 * (k == cu ? 0 : k)]; }
__device__ __forceinline__ bool stored_at(const AmFlag *fw, int k, int cu) { return (flag_word(fw, k, cu) & 3u) != 0; }

struct DiagArgs {
    const double *AM;
    const AmFlag *flag;        // [W][cov_update], or nullptr: every row is stored
    double *acc;
    long long nstreams;        // W * ndim
    long long k_done;          // n_done / batch0: level-0 batches complete before the call
    int rem;                   // n_done % batch0: samples in the batch under way
    int first;                 // n_done == 0: the first sample of the call is the shift
    int d, epl, cu, klo, khi, L, b0;
};

__global__ __launch_bounds__(256) void diag_rows_kernel(const DiagArgs a)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.nstreams) return;
    const int L = a.L, cu = a.cu;
    const long long w = g / a.d;
    const int p = (int)(g - w * a.d);
    double *st = a.acc + (size_t)w * a.d + am_inv(p, a.epl);
    const size_t plane = (size_t)a.nstreams;
    const double *src = a.AM + (size_t)w * cu * a.d + p;
    const AmFlag *fw = a.flag ? a.flag + (size_t)w * cu : nullptr;

    double c = st[0], S1 = st[plane], S2 = st[2 * plane], A = st[3 * plane];
    double Q[LMAX], H[LMAX - 1];
#pragma unroll
    for (int l = 0; l < LMAX; ++l) Q[l] = l < L ? st[(size_t)(4 + l) * plane] : 0.0;
#pragma unroll
    for (int l = 0; l < LMAX - 1; ++l) H[l] = l < L - 1 ? st[(size_t)(4 + L + l) * plane] : 0.0;

    // the row iteration klo stands for: itself where it was stored, else the stored row its run hangs on (ring row 1 of a period is a KEY row)
    double x;
    {
        int s = a.klo;
        if (fw) while (s > 1 && !stored_at(fw, s, cu)) --s;
        x = src[(size_t)(s == cu ? 0 : s) * a.d];
    }
    long long k = a.k_done;
    int rem = a.rem;
    if (a.first) c = x;
    // The flag words run one chunk ahead of the rows, so a chunk's row loads wait for nothing but the chunk before.  They are loaded
    // without a branch (an iteration beyond iter_hi reads iter_hi's word again) and tested only where they are used: the eight loads
    // go out together, one wait for all of them.
    unsigned fl[UNR];
#pragma unroll
    for (int j = 0; j < UNR; ++j) fl[j] = (unsigned)AMROW_KEY;
    if (fw) {
#pragma unroll
        for (int j = 0; j < UNR; ++j) fl[j] = flag_word(fw, min(a.klo + j, a.khi), cu);
    }
    for (int k0 = a.klo; k0 <= a.khi; k0 += UNR) {
        double v[UNR];
        bool ld[UNR];
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const int kk = k0 + j;
            ld[j] = kk <= a.khi && kk != a.klo && (fl[j] & 3u) != 0;
        }
        if (fw) {
#pragma unroll
            for (int j = 0; j < UNR; ++j) fl[j] = flag_word(fw, min(k0 + UNR + j, a.khi), cu);
        }
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const int kk = k0 + j;
            v[j] = 0.0;
            if (ld[j]) v[j] = src[(size_t)(kk == cu ? 0 : kk) * a.d];
        }
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            if (k0 + j > a.khi) break;                         // uniform
            if (ld[j]) x = v[j];
            const double y = x - c;
            S1 += y;
            S2 += y * y;
            A += y;
            if (++rem == a.b0) {                               // uniform: a level-0 batch is complete
                rem = 0;
                ++k;
                double t = A;
                A = 0.0;
#pragma unroll
                for (int l = 0; l < LMAX; ++l) {
                    if (l >= L) break;
                    Q[l] += t * t;
                    if (l == L - 1) break;
                    if ((k >> l) & 1) { H[l] = t; break; }
                    t = H[l] + t;
                }
            }
        }
    }
    st[0] = c; st[plane] = S1; st[2 * plane] = S2; st[3 * plane] = A;
#pragma unroll
    for (int l = 0; l < LMAX; ++l)
        if (l < L) st[(size_t)(4 + l) * plane] = Q[l];
#pragma unroll
    for (int l = 0; l < LMAX - 1; ++l)
        if (l < L - 1) st[(size_t)(4 + L + l) * plane] = H[l];
}

}  // namespace

void ptmi_diag_free(ptmi_engine *h)
{
    delete h->diag;
    h->diag = nullptr;
}

extern "C" {

int ptmi_diag_attach(ptmi_handle h, double *acc, int32_t nlevels, int32_t batch0)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (h->diag) return fail(PTMI_EINVAL, "ptmi_diag_attach: already attached");
    if (nlevels < 1 || nlevels > LMAX) return fail(PTMI_EINVAL, "ptmi_diag_attach: 1 <= nlevels <= %d (got %d)", LMAX, (int)nlevels);
    if (batch0 < 1) return fail(PTMI_EINVAL, "ptmi_diag_attach: batch0 >= 1 (got %d)", (int)batch0);
    if (!acc || ((uintptr_t)acc & 7) != 0) return fail(PTMI_EINVAL, "ptmi_diag_attach: acc must be non-NULL and 8-byte aligned");
    ptmi_diag_state *s = new ptmi_diag_state();
    s->acc = acc;
    s->nlevels = (int)nlevels;
    s->batch0 = (int)batch0;
    h->diag = s;
    return PTMI_OK;
}

int ptmi_diag_update(ptmi_handle h, int64_t iter_lo, int64_t iter_hi, int64_t n_done)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    const ptmi_diag_state *s = h->diag;
    if (!s) return fail(PTMI_EINVAL, "ptmi_diag_update: no accumulators are attached (ptmi_diag_attach)");
    const ptmi_config &c = h->cfg;
    long long base;
    if (int r = ring_range(h, "ptmi_diag_update", iter_lo, iter_hi, &base)) return r == RING_IDLE ? PTMI_OK : r;
    if (n_done < 0) return fail(PTMI_EINVAL, "ptmi_diag_update: n_done >= 0 (got %lld)", (long long)n_done);
    DiagArgs a;
    a.AM = h->buf.AM; a.flag = (const AmFlag *)h->buf.AMflag; a.acc = s->acc;
    a.nstreams = (long long)c.nwalkers * c.ndim;
    a.k_done = (long long)n_done / s->batch0; a.rem = (int)((long long)n_done % s->batch0); a.first = n_done == 0;
    a.d = c.ndim; a.epl = am_row_epl(h->G, h->EPL); a.cu = c.cov_update;
    a.klo = (int)(iter_lo - base); a.khi = (int)(iter_hi - base); a.L = s->nlevels; a.b0 = s->batch0;
    const long long nblocks = (a.nstreams + 255) / 256;
    if (nblocks >= (1ll << 31)) return fail(PTMI_EUNSUPPORTED, "ptmi_diag_update: %lld streams (a block per 256: below 2^31 blocks)", a.nstreams);
    hipLaunchKernelGGL(diag_rows_kernel, dim3((unsigned)nblocks), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

}  // extern "C"
