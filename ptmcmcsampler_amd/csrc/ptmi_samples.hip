// ptmi_samples.hip -- thinned snapshots of EVERY cold chain, kept on the device (ptmi_samples_attach / ptmi_samples_take, include/ptmi.h;
// the schedule: ptmcmcsampler_amd/samples.py SlotPlan).  The AM ring (ptmi_buffers.AM, [W][cov_update][ndim]) holds the rank-0 row of
// every walker for every iteration of the current covariance period; ptmi_update_cov, ptmi_hist_update, ptmi_pairs_update and
// ptmi_diag_update reduce it, this unit is a reader that keeps rows: for a list of (iteration, slot) the row every walker's cold chain
// held at that iteration goes to rows[slot][w][.] in PARAMETER order, its lnL and lp (ptmi_buffers.AMaux) to aux[slot][w][0 .. 1].
// The words are moved as 64-bit integers: NaN payloads, infinities and -0.0 arrive as they were.
//
// samples_gather_kernel: one wave per (pair, walker), four per 256-thread block.  With AMflag a row that was not stored repeats the
// last stored row before it (ptmi_am_expand's rule): the wave walks back 64 flag words per step, lane l looking at iteration k - l, and
// stops at the first set bit of the 64-bit ballot -- a run of 900 rejected steps costs 15 steps, not 900; ring row 1 of a period is a
// KEY row, so the walk ends inside the period (and is clamped to it whatever the flags hold).  The row is then loaded in ring order, 64
// consecutive words per instruction; the permutation of the exact 4-lane shape's row format (am_inv) falls on the stores.  lnL / lp
// come from iteration k's OWN ring row: the step kernels and the swap write AMaux at every iteration, stored or not.  The (k, slot)
// pairs travel as kernel arguments (copied at launch: nothing on the host has to outlive the call, and two queued calls share no
// staging buffer), PAIRS_PER_LAUNCH per launch.  The ring is only read.
#include "ptmi_common.h"
#define PTMI_RING_RANGE_ONLY       // this reader weighs no rows: no copy of hist_weight_kernel
#include "ptmi_ring_weight.h"      // ring_range
#include <vector>

struct ptmi_samples_state {
    double *rows;              // caller-owned [nslots][W][ndim], parameter order
    double *aux;               // caller-owned [nslots][W][2], or nullptr
    int nslots;
};

namespace {

constexpr int PAIRS_PER_LAUNCH = 256;   // 6 bytes each beside the header: a launch's arguments stay far below 4 KB
constexpr int NSLOTS_MAX = 65535;       // a slot travels as 16 bits

static_assert((AMROW_NEW | AMROW_KEY) == 3ull, "the flag bits sit in the low 32 bits of the word");

struct SamplesArgs {
    const u64 *AM;             // [W][cu][d] in the ring's row format
    const u64 *AMaux;          // [W][cu][2], or nullptr
    const AmFlag *flag;        // [W][cu], or nullptr: every row is stored
    u64 *rows, *aux;
    long long nwaves;          // n * W
    int W, d, epl, cu, n;
    int k[PAIRS_PER_LAUNCH];               // iteration base + k, 1 <= k <= cu
    unsigned short slot[PAIRS_PER_LAUNCH];
};
static_assert(sizeof(SamplesArgs) <= 4096, "kernel arguments: 4 KB at most");

// iteration base + k, k in 1 .. cu, sits in ring row k % cu
__device__ __forceinline__ int ring_row(int k, int cu) { return k == cu ? 0 : k; }

__global__ __launch_bounds__(256) void samples_gather_kernel(const SamplesArgs a)
{
    const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wv >= a.nwaves) return;                                    // wave-uniform
    const int lane = threadIdx.x & 63;
    const int pr = (int)(wv / a.W);
    const size_t w = (size_t)(wv - (long long)pr * a.W);
    const int cu = a.cu, d = a.d, k = a.k[pr];
    const size_t cell = (size_t)a.slot[pr] * a.W + w;

    int s = k;                                                     // the stored row iteration k stands for
    if (a.flag) {
        const unsigned *fw = reinterpret_cast<const unsigned *>(a.flag + w * cu);      // the low half of every word holds NEW and KEY
        for (;;) {
            const int kk = s - lane;
            const bool hit = kk >= 1 && (fw[2 * (size_t)ring_row(kk, cu)] & 3u) != 0;
            const unsigned long long m = __ballot(hit);
            if (m) { s -= __ffsll(m) - 1; break; }
            s -= 64;
            if (s < 1) { s = 1; break; }                           // (ring row 1 of a period is a KEY row: not reached)
        }
    }
    const u64 *src = a.AM + (w * cu + ring_row(s, cu)) * d;
    u64 *dst = a.rows + cell * d;
    for (int p = lane; p < d; p += 64) dst[am_inv(p, a.epl)] = src[p];
    if (a.aux && lane < 2) a.aux[cell * 2 + lane] = a.AMaux[(w * cu + ring_row(k, cu)) * 2 + lane];
}

}  // namespace

void ptmi_samples_free(ptmi_engine *h)
{
    delete h->samples;
    h->samples = nullptr;
}

extern "C" {

int ptmi_samples_attach(ptmi_handle h, double *rows, double *aux, int32_t nslots)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (h->samples) return fail(PTMI_EINVAL, "ptmi_samples_attach: already attached");
    if (nslots < 1 || nslots > NSLOTS_MAX) return fail(PTMI_EINVAL, "ptmi_samples_attach: 1 <= nslots <= %d (got %d)", NSLOTS_MAX, (int)nslots);
    if (!rows || ((uintptr_t)rows & 7) != 0) return fail(PTMI_EINVAL, "ptmi_samples_attach: rows must be non-NULL and 8-byte aligned");
    if (aux && ((uintptr_t)aux & 7) != 0) return fail(PTMI_EINVAL, "ptmi_samples_attach: aux must be 8-byte aligned (or NULL)");
    if (aux && !h->buf.AMaux) return fail(PTMI_EINVAL, "ptmi_samples_attach: aux needs a handle with AMaux (lnL and lp beside the ring's rows)");
    ptmi_samples_state *s = new ptmi_samples_state();
    s->rows = rows;
    s->aux = aux;
    s->nslots = (int)nslots;
    h->samples = s;
    return PTMI_OK;
}

int ptmi_samples_take(ptmi_handle h, const int64_t *iters, const int32_t *slots, int32_t n)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    const ptmi_samples_state *s = h->samples;
    if (!s) return fail(PTMI_EINVAL, "ptmi_samples_take: no buffer is attached (ptmi_samples_attach)");
    if (n < 0) return fail(PTMI_EINVAL, "ptmi_samples_take: n >= 0 (got %d)", (int)n);
    const ptmi_config &c = h->cfg;
    if (n == 0 || c.temp0 != 0) return PTMI_OK;                    // only the GPU holding rank 0 has the cold chains (as ptmi_update_cov)
    if (!iters || !slots) return fail(PTMI_EINVAL, "ptmi_samples_take: iters and slots must be non-NULL");
    std::vector<char> seen((size_t)s->nslots, 0);
    for (int i = 0; i < n; ++i) {
        if (i > 0 && iters[i] <= iters[i - 1])
            return fail(PTMI_EINVAL, "ptmi_samples_take: iters must be strictly ascending (entry %d: %lld behind %lld)", i, (long long)iters[i],
                        (long long)iters[i - 1]);
        if (slots[i] < 0 || slots[i] >= s->nslots)
            return fail(PTMI_EINVAL, "ptmi_samples_take: slot %d of entry %d is out of range 0 .. %d", (int)slots[i], i, s->nslots - 1);
        if (seen[(size_t)slots[i]]) return fail(PTMI_EINVAL, "ptmi_samples_take: slot %d is repeated (entry %d)", (int)slots[i], i);
        seen[(size_t)slots[i]] = 1;
    }
    long long base;
    if (int r = ring_range(h, "ptmi_samples_take", iters[0], iters[n - 1], &base)) return r == RING_IDLE ? PTMI_OK : r;
    if (s->aux && !h->buf.AMaux) return fail(PTMI_EINVAL, "ptmi_samples_take: the handle has no AMaux buffer");
    SamplesArgs a;
    a.AM = (const u64 *)h->buf.AM; a.AMaux = (const u64 *)h->buf.AMaux; a.flag = (const AmFlag *)h->buf.AMflag;
    a.rows = (u64 *)s->rows; a.aux = (u64 *)s->aux;
    a.W = c.nwalkers; a.d = c.ndim; a.epl = am_row_epl(h->G, h->EPL); a.cu = c.cov_update;
    if ((long long)PAIRS_PER_LAUNCH * c.nwalkers / 4 + 1 >= (1ll << 31))
        return fail(PTMI_EUNSUPPORTED, "ptmi_samples_take: %d walkers (a block per four (pair, walker): below 2^31 blocks)", (int)c.nwalkers);
    for (int i0 = 0; i0 < n; i0 += PAIRS_PER_LAUNCH) {
        a.n = n - i0 < PAIRS_PER_LAUNCH ? n - i0 : PAIRS_PER_LAUNCH;
        for (int i = 0; i < PAIRS_PER_LAUNCH; ++i) {
            a.k[i] = i < a.n ? (int)(iters[i0 + i] - base) : 1;
            a.slot[i] = i < a.n ? (unsigned short)slots[i0 + i] : 0;
        }
        a.nwaves = (long long)a.n * c.nwalkers;
        hipLaunchKernelGGL(samples_gather_kernel, dim3((unsigned)((a.nwaves + 3) / 4)), dim3(256), 0, h->stream, a);
        HIPCHK(hipGetLastError());
    }
    return PTMI_OK;
}

}  // extern "C"
