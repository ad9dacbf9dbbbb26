// ptmi_cj.hip -- custom jump proposals in the cycle as batched device callbacks on the split path (ptmi_cj_attach / ptmi_cj_work_bytes /
// ptmi_cj_begin / ptmi_cj_end / ptmi_cj_box_draw, include/ptmi.h).  The reference's extension point is addProposalToCycle(func, weight)
// (PT:988-1014, PT = PTMCMCSampler/PTMCMCSampler.py), dispatched per chain at PT:1058-1059: q, qxy = func(x, iter, beta).  Here every
// chain whose pick of an iteration is such an entry is served at once: the proposal launch hands its state back as the proposal row
// with jt = PTMI_J_NTYPES + pick in qaux[.][1] (ptmi_split.hip, propose() of ptmi_mh.inc.h); this stage, between that launch and the
// likelihood callback,
//
//   * lists those chains sorted by (function, chain slot w * T + s) -- per block of 1024 chain slots the counts per function
//     (cj_count_kernel), then each block's starts from the counts of the blocks before it and a ballot scan inside
//     (cj_gather_kernel): no atomics, the order is the same on every run -- and copies each listed chain's row out of the current
//     proposal buffer into the caller's rows [n][ndim], with beta [n] beside it; the per-function offsets go to the host, the
//     stage's one read-back (ptmi_cj_begin);
//   * the caller runs func_f(rows[offs[f] .. offs[f + 1]), iter, beta) -> (rows', qxy) for every function with a non-empty span;
//   * cj_scatter_kernel puts the rows back into the listed chains' rows of the proposal buffer and qxy into qaux[.][0] (ptmi_cj_end).
//
// Row copies are contiguous 16-byte pieces (8-byte for odd ndim), as in split_rows_kernel.  Per update that is 5/65 (the reference's
// test cycle, tests/test_simple.py:94-97) of three row passes: proposal buffer -> rows, the callback's own read and write, rows ->
// proposal buffer.  cj_box_kernel is the reference's UniformJump (tests/test_simple.py:44-62) on the library's own Philox stream.
#include "ptmi_common.h"

namespace {

constexpr int LB = 1024;             // chain slots per block of the listing kernels
constexpr int NF = PTMI_CJ_MAXFUN;
constexpr int SR = 64;               // rows per block of the scatter kernel

// The work area (ptmi_cj_work_bytes): list [nch] int32 (the listed chains' slots, sorted by (function, slot)), bcnt [nblk][NF] int32 (the
// listing's block counts), offs [NF + 1] int64 (function f owns list[offs[f] .. offs[f + 1]); entries beyond nfun repeat the total).
struct Work {
    int32_t *list, *bcnt;
    long long *offs;
};
inline size_t al16(size_t b) { return (b + 15) & ~(size_t)15; }
inline size_t work_layout(long long nch, char *base, Work *w)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += al16(bytes); return p; };
    const size_t nblk = (size_t)((nch + LB - 1) / LB);
    Work t;
    t.list = (int32_t *)take(sizeof(int32_t) * (size_t)nch);
    t.bcnt = (int32_t *)take(sizeof(int32_t) * nblk * NF);
    t.offs = (long long *)take(sizeof(long long) * (NF + 1));
    if (w) *w = t;
    return off;
}

struct CjArgs {
    Work w;
    long long nch;
    int d, nt, w_host, nfun;
    const int32_t *fun_of_pick;      // [w_host]
    double *Q;                       // the current proposal buffer
    double *qaux;
    const int32_t *temp_of;
    const double *beta;
};

template <int VEC> struct Piece;
template <> struct Piece<2> { typedef ptmi_dev_d2 T; };
template <> struct Piece<1> { typedef double T; };

// the function that serves chain slot ch's pick, or -1: a built-in jump
__device__ __forceinline__ int fun_of(const CjArgs &a, long long ch)
{
    if (ch >= a.nch) return -1;
    const int pick = (int)a.qaux[ch * 4 + 1] - PTMI_J_NTYPES;
    return (pick >= 0 && pick < a.w_host) ? a.fun_of_pick[pick] : -1;
}

// The listing: block b counts, per function, the listed chains of slots [b LB, (b + 1) LB) ...
__global__ __launch_bounds__(LB) void cj_count_kernel(const CjArgs a)
{
    const int f = fun_of(a, (long long)blockIdx.x * LB + threadIdx.x);
    for (int g = 0; g < a.nfun; ++g) {
        const int c = __syncthreads_count(f == g);
        if (threadIdx.x == 0) a.w.bcnt[(size_t)blockIdx.x * NF + g] = c;
    }
}

// ... and writes them to list[] from its starts -- function f's span begins behind all chains of the functions before it, the
// block's part of it behind the parts of the blocks before it; inside the block slot order by a ballot scan -- and copies their rows
// and beta.  Block 0 writes the offsets.
template <int VEC>
__global__ __launch_bounds__(LB) void cj_gather_kernel(const CjArgs a, double *rows, double *beta_out)
{
    __shared__ int ptot[LB / NF][NF], ppre[LB / NF][NF];     // partial sums over the blocks: all of them, the ones before this
    __shared__ long long start[NF];                          // where this block's chains of function f go in list[]
    __shared__ int lstart[NF];                               // ... and in the block's own compact order
    __shared__ int wcnt[LB / 64][NF];
    __shared__ int32_t lch[LB];
    __shared__ long long lpos[LB];
    __shared__ int mtot;
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nblk = (int)gridDim.x, me = (int)blockIdx.x;
    {
        const int g = tid % NF, part = tid / NF;
        int tot = 0, pre = 0;
        if (g < a.nfun)
            for (int b = part; b < nblk; b += LB / NF) {
                const int c = a.w.bcnt[(size_t)b * NF + g];
                tot += c;
                if (b < me) pre += c;
            }
        ptot[part][g] = tot;
        ppre[part][g] = pre;
    }
    const long long ch = (long long)me * LB + tid;
    const int f = fun_of(a, ch);
    int wrank = 0;
    for (int g = 0; g < a.nfun; ++g) {
        const u64 mask = __ballot(f == g);
        if (lane == 0) wcnt[wv][g] = __popcll(mask);
        if (f == g) wrank = __popcll(mask & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    if (tid < NF) {                                          // thread g: function g's totals over the partial sums
        int tot = 0, pre = 0, mine = 0;
        if (tid < a.nfun) {
#pragma unroll 1
            for (int p = 0; p < LB / NF; ++p) { tot += ptot[p][tid]; pre += ppre[p][tid]; }
#pragma unroll 1
            for (int k = 0; k < LB / 64; ++k) mine += wcnt[k][tid];
        }
        ptot[0][tid] = tot;
        ppre[0][tid] = pre;
        lstart[tid] = mine;
    }
    __syncthreads();
    if (tid == 0) {                                          // ... and the running sums over the functions
        long long base = 0;
        int lb = 0;
#pragma unroll 1
        for (int g = 0; g < NF; ++g) {
            const int mine = lstart[g];
            if (me == 0) a.w.offs[g] = base;
            start[g] = base + ppre[0][g];
            lstart[g] = lb;
            base += ptot[0][g];
            lb += mine;
        }
        if (me == 0) a.w.offs[NF] = base;
        mtot = lb;
    }
    __syncthreads();
    if (f >= 0) {
        int r = wrank;
        for (int k = 0; k < wv; ++k) r += wcnt[k][f];
        const long long pos = start[f] + r;
        a.w.list[pos] = (int32_t)ch;
        beta_out[pos] = a.beta[a.temp_of[ch]];
        lch[lstart[f] + r] = (int32_t)ch;
        lpos[lstart[f] + r] = pos;
    }
    __syncthreads();
    typedef typename Piece<VEC>::T PT;
    const int P = a.d / VEC, total = mtot * P;
    const PT *src = reinterpret_cast<const PT *>(a.Q);
    PT *dst = reinterpret_cast<PT *>(rows);
    for (int p = tid; p < total; p += LB) {
        const int c = p / P, ip = p - c * P;
        dst[(size_t)lpos[c] * P + ip] = src[(size_t)lch[c] * P + ip];
    }
}

// ptmi_cj_end: row k of the callbacks' rows goes back to chain list[k]'s row of the proposal buffer, qxy[k] (or 0) to its qaux[.][0]
template <int VEC>
__global__ __launch_bounds__(256) void cj_scatter_kernel(const CjArgs a, long long n, const double *rows, const double *qxy)
{
    __shared__ int32_t lch[SR];
    const long long k0 = (long long)blockIdx.x * SR;
    const int nr = (int)(n - k0 < SR ? n - k0 : SR), tid = (int)threadIdx.x;
    if (tid < nr) {
        const int32_t ch = a.w.list[k0 + tid];
        lch[tid] = ch;
        a.qaux[(size_t)ch * 4] = qxy ? qxy[k0 + tid] : 0.0;
    }
    __syncthreads();
    typedef typename Piece<VEC>::T PT;
    const int P = a.d / VEC, total = nr * P;
    const PT *src = reinterpret_cast<const PT *>(rows) + (size_t)k0 * P;
    PT *dst = reinterpret_cast<PT *>(a.Q);
    for (int p = tid; p < total; p += 256) {
        const int c = p / P, ip = p - c * P;
        dst[(size_t)lch[c] * P + ip] = src[p];
    }
}

// ptmi_cj_box_draw: the reference's UniformJump (tests/test_simple.py:44-62) for the chains list[k0 .. k0 + n): one thread per pair of
// parameters (2 j, 2 j + 1) = the two words of one Philox call
__global__ __launch_bounds__(256) void cj_box_kernel(const CjArgs a, long long k0, long long n, u64 seed, long long it, int ntg, int temp0,
                                                     int walker0, const double *lo, const double *hi, double *rows)
{
    const int hp = (a.d + 1) / 2;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n * hp) return;
    const long long k = g / hp;
    const int j = (int)(g - k * hp);
    const long long ch = a.w.list[k0 + k];
    const int w = (int)(ch / a.nt), t = a.temp_of[ch];
    const u32 sid = (u32)((u64)(walker0 + w) * (u32)ntg) + (u32)(temp0 + t);
    u64 w0, w1;
    philox_words(seed, (u64)it, sid, SLOT_CJ + (u32)j, w0, w1);
    double *q = rows + (size_t)k * a.d;
    const int i = 2 * j;
    const double s0 = (hi[i] - lo[i]) * w2uniform(w0);
    q[i] = lo[i] + s0;
    if (i + 1 < a.d) {
        const double s1 = (hi[i + 1] - lo[i + 1]) * w2uniform(w1);
        q[i + 1] = lo[i + 1] + s1;
    }
}

CjArgs make_cj_args(ptmi_engine *h, void *work)
{
    const ptmi_config &c = h->cfg;
    CjArgs a;
    memset(&a, 0, sizeof(a));
    a.nch = (long long)c.nwalkers * c.ntemps;
    work_layout(a.nch, (char *)work, &a.w);
    a.d = c.ndim; a.nt = c.ntemps; a.w_host = c.w_host; a.nfun = h->cj_nfun;
    a.fun_of_pick = h->d_cj_fun;
    a.Q = (h->q_cur && h->buf.Q2) ? h->buf.Q2 : h->buf.Q;
    a.qaux = h->buf.qaux; a.temp_of = h->buf.temp_of; a.beta = h->d_beta;
    return a;
}

}  // namespace

extern "C" {

int ptmi_cj_attach(ptmi_handle h, uint64_t *cjstat, const int32_t *fun_of_pick, int32_t nfun)
{
    if (!h || !cjstat || !fun_of_pick) return fail(PTMI_EINVAL, "NULL argument");
    const ptmi_config &c = h->cfg;
    if (c.w_host <= 0) return fail(PTMI_EINVAL, "ptmi_cj_attach: the handle has no host-served cycle entries (w_host = 0)");
    if (!h->buf.Q || !h->buf.qaux) return fail(PTMI_EINVAL, "ptmi_cj_attach: split path needs the Q and qaux buffers");
    if (nfun < 1) return fail(PTMI_EINVAL, "ptmi_cj_attach: nfun = %d", (int)nfun);
    if (nfun > PTMI_CJ_MAXFUN) return fail(PTMI_EUNSUPPORTED, "ptmi_cj_attach: %d functions, at most %d", (int)nfun, PTMI_CJ_MAXFUN);
    if (h->cj_nfun > 0) return fail(PTMI_EINVAL, "ptmi_cj_attach: already attached");
    if (h->cj_phase != PTMI_GJ_NONE || h->gj_phase != PTMI_GJ_NONE) return fail(PTMI_EINVAL, "ptmi_cj_attach: call it before the first ptmi_propose");
    for (int k = 0; k < c.w_host; ++k)
        if (fun_of_pick[k] < 0 || fun_of_pick[k] >= nfun) return fail(PTMI_EINVAL, "ptmi_cj_attach: fun_of_pick[%d] = %d outside [0, %d)", k, (int)fun_of_pick[k], (int)nfun);
    HIPCHK(hipMalloc((void **)&h->d_cj_fun, sizeof(int32_t) * (size_t)c.w_host));
    HIPCHK(hipMemcpy(h->d_cj_fun, fun_of_pick, sizeof(int32_t) * (size_t)c.w_host, hipMemcpyHostToDevice));
    HIPCHK(hipHostMalloc((void **)&h->h_cj_offs, sizeof(long long) * (PTMI_CJ_MAXFUN + 1)));
    // cycles with AM entries: the increments' scratch ptmi_create left out for w_host > 0 -- the row kernels then serve the handle
    if (c.w_am > 0 && c.ndim <= 1024 && h->split_am_piece == 0 && h->am_piece == 0) {
        const hipError_t e = ptmi_am_scratch_alloc(h, false);
        if (e != hipSuccess) return fail(PTMI_EHIP, "ptmi_cj_attach: %s", hipGetErrorString(e));
    }
    h->cjstat = (u64 *)cjstat;
    h->cj_nfun = nfun;
    return PTMI_OK;
}

int ptmi_cj_work_bytes(ptmi_handle h, size_t *bytes)
{
    if (!h || !bytes) return fail(PTMI_EINVAL, "NULL argument");
    *bytes = work_layout((long long)h->cfg.nwalkers * h->cfg.ntemps, nullptr, nullptr);
    return PTMI_OK;
}

int ptmi_cj_begin(ptmi_handle h, int64_t iter, void *work, double *rows, double *beta, int64_t *offs)
{
    if (!h || !work || !rows || !beta || !offs) return fail(PTMI_EINVAL, "NULL argument");
    if (h->cj_nfun <= 0) return fail(PTMI_EINVAL, "ptmi_cj_begin: no batched custom jumps are attached (ptmi_cj_attach)");
    if (h->dev_iter) return fail(PTMI_EUNSUPPORTED, "ptmi_cj_begin: the stage reads its offsets on the host: not in ptmi_device_iter mode");
    if (h->cj_phase != PTMI_GJ_PENDING || h->cj_iter != (long long)iter)
        return fail(PTMI_EINVAL, "ptmi_cj_begin(%lld): no proposals of that iteration wait for their custom jumps (%s)", (long long)iter,
                    h->cj_phase == PTMI_GJ_PENDING ? "the proposals are another iteration's" : "call it once, after ptmi_propose / ptmi_accept_propose");
    if (((uintptr_t)work & 15) != 0 || ((uintptr_t)rows & 15) != 0) return fail(PTMI_EINVAL, "ptmi_cj_begin: the work area and the rows must be 16-byte aligned");
    const CjArgs a = make_cj_args(h, work);
    const unsigned nblk = (unsigned)((a.nch + LB - 1) / LB);
    hipLaunchKernelGGL(cj_count_kernel, dim3(nblk), dim3(LB), 0, h->stream, a);
    if (a.d % 2 == 0) hipLaunchKernelGGL(cj_gather_kernel<2>, dim3(nblk), dim3(LB), 0, h->stream, a, rows, beta);
    else hipLaunchKernelGGL(cj_gather_kernel<1>, dim3(nblk), dim3(LB), 0, h->stream, a, rows, beta);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h->h_cj_offs, a.w.offs, sizeof(long long) * (PTMI_CJ_MAXFUN + 1), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));                  // the stage's one read-back
    for (int f = 0; f <= PTMI_CJ_MAXFUN; ++f) h->cj_offs[f] = h->h_cj_offs[f];
    for (int f = 0; f <= h->cj_nfun; ++f) offs[f] = (int64_t)h->cj_offs[f];
    h->cj_work = work;
    h->cj_phase = PTMI_GJ_ROUNDS;
    return PTMI_OK;
}

int ptmi_cj_end(ptmi_handle h, void *work, const double *rows, const double *qxy)
{
    if (!h || !work || !rows) return fail(PTMI_EINVAL, "NULL argument");
    if (h->cj_phase != PTMI_GJ_ROUNDS) return fail(PTMI_EINVAL, "ptmi_cj_end: no custom-jump stage is open (ptmi_cj_begin first)");
    if (work != h->cj_work) return fail(PTMI_EINVAL, "ptmi_cj_end: not the work area ptmi_cj_begin was given");
    if (((uintptr_t)rows & 15) != 0) return fail(PTMI_EINVAL, "ptmi_cj_end: the rows must be 16-byte aligned");
    const CjArgs a = make_cj_args(h, work);
    const long long n = h->cj_offs[h->cj_nfun];
    if (n > 0) {
        const unsigned grid = (unsigned)((n + SR - 1) / SR);
        if (a.d % 2 == 0) hipLaunchKernelGGL(cj_scatter_kernel<2>, dim3(grid), dim3(256), 0, h->stream, a, n, rows, qxy);
        else hipLaunchKernelGGL(cj_scatter_kernel<1>, dim3(grid), dim3(256), 0, h->stream, a, n, rows, qxy);
        HIPCHK(hipGetLastError());
    }
    h->cj_phase = PTMI_GJ_DONE;
    return PTMI_OK;
}

int ptmi_cj_box_draw(ptmi_handle h, void *work, int32_t fun, const double *lo, const double *hi, double *rows)
{
    if (!h || !work || !lo || !hi || !rows) return fail(PTMI_EINVAL, "NULL argument");
    if (h->cj_phase != PTMI_GJ_ROUNDS) return fail(PTMI_EINVAL, "ptmi_cj_box_draw: no custom-jump stage is open (ptmi_cj_begin first)");
    if (work != h->cj_work) return fail(PTMI_EINVAL, "ptmi_cj_box_draw: not the work area ptmi_cj_begin was given");
    if (fun < 0 || fun >= h->cj_nfun) return fail(PTMI_EINVAL, "ptmi_cj_box_draw: function %d outside [0, %d)", (int)fun, h->cj_nfun);
    const CjArgs a = make_cj_args(h, work);
    const ptmi_config &c = h->cfg;
    const long long k0 = h->cj_offs[fun], n = h->cj_offs[fun + 1] - k0;
    if (n <= 0) return PTMI_OK;
    const long long threads = n * ((a.d + 1) / 2);
    hipLaunchKernelGGL(cj_box_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, h->stream, a, k0, n, (u64)c.seed, h->cj_iter,
                       c.ntemps_global, c.temp0, c.walker0, lo, hi, rows);
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

}  // extern "C"
