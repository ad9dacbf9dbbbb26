// ptmi_sup.hip -- the likelihood callback only inside the prior's support (ptmi_sup_work_bytes / ptmi_sup_begin / ptmi_sup_rows /
// ptmi_sup_end, include/ptmi.h).  The reference reads lp = logp(y) and calls logl(y) only when lp != -inf (PT:605-612, PT =
// PTMCMCSampler/PTMCMCSampler.py; the first evaluation the same, PT:479-487).  On the batched callback path this stage sits between the
// prior callback and the likelihood callback of n_in rows:
//
//   * ptmi_sup_begin lists the rows k with lp[k] != -inf in ascending k (NaN and +inf are listed: the reference tests == -inf and
//     nothing else): sup_count_kernel counts them per block of 1024 rows, sup_scan_kernel -- ONE block -- scans the block counts once
//     and leaves the total, sup_rank_kernel ranks every block's rows by ballots behind its start: pos[k] = the row's rank in the list
//     or -1, list[pos[k]] = k.  No atomics: the same order on every run.  The total goes to the host, the stage's one read-back;
//   * ptmi_sup_rows copies the listed rows to rows[pos] (sup_rows_kernel: launched behind the read-back, its grid sized from n; a row
//     belongs to a wave, or to a power-of-two share of its lanes where a row has fewer pieces than the wave lanes), contiguous 16-byte
//     pieces, 8-byte for odd ndim;
//   * the caller runs logl on rows[0 .. n);
//   * ptmi_sup_end writes out[k] = pos[k] >= 0 ? vals[pos[k]] : -inf (sup_end_kernel, one element-wise pass).
//
// It knows nothing about the proposal buffer: any row tensor of ndim columns, so the first evaluation takes it too.
#include "ptmi_common.h"

namespace {

constexpr int LB = 1024;             // rows per block of the listing kernels

// The work area (ptmi_sup_work_bytes): pos [n_in] int32 (a row's rank in the list, or -1), list [n_in] int32 (the listed rows, ascending),
// bcnt [nblk] int32 (the listing's block counts), boff [nblk] int32 (their exclusive scan), n int64 (the total).
struct Work {
    int32_t *pos, *list, *bcnt, *boff;
    long long *n;
};
inline size_t al16(size_t b) { return (b + 15) & ~(size_t)15; }
inline size_t work_layout(long long n_in, char *base, Work *w)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += al16(bytes); return p; };
    const size_t nblk = (size_t)((n_in + LB - 1) / LB);
    Work t;
    t.pos = (int32_t *)take(sizeof(int32_t) * (size_t)n_in);
    t.list = (int32_t *)take(sizeof(int32_t) * (size_t)n_in);
    t.bcnt = (int32_t *)take(sizeof(int32_t) * nblk);
    t.boff = (int32_t *)take(sizeof(int32_t) * nblk);
    t.n = (long long *)take(sizeof(long long));
    if (w) *w = t;
    return off;
}

template <int VEC> struct Piece;
template <> struct Piece<2> { typedef ptmi_dev_d2 T; };
template <> struct Piece<1> { typedef double T; };

__device__ __forceinline__ bool listed(const double *lp, long long k, long long n_in)
{
    return k < n_in && lp[k] != -__builtin_inf();            // NaN != -inf: listed, as the reference's lp == -np.inf leaves it
}

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ int wave_scan(int v, int lane)
{
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_up(v, s, 64);
        if (lane >= s) v += o;
    }
    return v;
}

// The listing: block b counts the listed rows of [b LB, (b + 1) LB) ...
__global__ __launch_bounds__(LB) void sup_count_kernel(const Work w, const double *lp, long long n_in)
{
    const int c = __syncthreads_count(listed(lp, (long long)blockIdx.x * LB + threadIdx.x, n_in));
    if (threadIdx.x == 0) w.bcnt[blockIdx.x] = c;
}

// ... ONE block turns the counts into every block's start (LB counts at a time, the running total carried along) and leaves the total ...
__global__ __launch_bounds__(LB) void sup_scan_kernel(const Work w, int nblk)
{
    __shared__ int wtot[LB / 64];
    __shared__ int carry;
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nblk; b0 += LB) {
        const int b = b0 + tid;
        const int c = b < nblk ? w.bcnt[b] : 0;
        const int inc = wave_scan(c, lane);
        if (lane == 63) wtot[wv] = inc;
        __syncthreads();
        int before = carry;
        for (int k = 0; k < wv; ++k) before += wtot[k];
        if (b < nblk) w.boff[b] = before + inc - c;
        __syncthreads();
        if (tid == LB - 1) carry = before + inc;
        __syncthreads();
    }
    if (tid == 0) *w.n = (long long)carry;
}

// ... and every block ranks its rows behind its start: wave order, lane order
__global__ __launch_bounds__(LB) void sup_rank_kernel(const Work w, const double *lp, long long n_in)
{
    __shared__ int wcnt[LB / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long k = (long long)blockIdx.x * LB + tid;
    const bool in = listed(lp, k, n_in);
    const u64 mask = __ballot(in);
    if (lane == 0) wcnt[wv] = __popcll(mask);
    __syncthreads();
    if (k >= n_in) return;
    int r = -1;
    if (in) {
        r = w.boff[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
        for (int j = 0; j < wv; ++j) r += wcnt[j];
        w.list[r] = (int32_t)k;
    }
    w.pos[k] = r;
}

// ptmi_sup_rows: listed row j = rows_in[list[j]] goes to rows[j]; 1 << lsh lanes share a row (a whole wave from 33 pieces on)
template <int VEC>
__global__ __launch_bounds__(256) void sup_rows_kernel(const int32_t *list, long long n, int P, int lsh, const double *rows_in, double *rows)
{
    typedef typename Piece<VEC>::T PT;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long j = g >> lsh;
    if (j >= n) return;
    const int l0 = (int)(g & ((1ll << lsh) - 1)), step = 1 << lsh;
    const PT *src = reinterpret_cast<const PT *>(rows_in) + (size_t)list[j] * P;
    PT *dst = reinterpret_cast<PT *>(rows) + (size_t)j * P;
    for (int p = l0; p < P; p += step) dst[p] = src[p];
}

// ptmi_sup_end: the callback's values back to their rows, -inf to the rows it was not given (vals == nullptr: to all of them)
__global__ __launch_bounds__(256) void sup_end_kernel(const int32_t *pos, long long n_in, const double *vals, double *out)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_in) return;
    const int r = vals ? pos[k] : -1;
    out[k] = r >= 0 ? vals[r] : -__builtin_inf();
}

}  // namespace

extern "C" {

int ptmi_sup_work_bytes(ptmi_handle h, int64_t n_in, size_t *bytes)
{
    if (!h || !bytes) return fail(PTMI_EINVAL, "NULL argument");
    if (n_in < 1 || n_in > 0x7fffffffll) return fail(PTMI_EINVAL, "ptmi_sup_work_bytes: n_in = %lld outside [1, 2^31)", (long long)n_in);
    *bytes = work_layout((long long)n_in, nullptr, nullptr);
    return PTMI_OK;
}

int ptmi_sup_begin(ptmi_handle h, void *work, const double *lp, int64_t n_in, int64_t *n)
{
    if (!h || !work || !lp || !n) return fail(PTMI_EINVAL, "NULL argument");
    if (h->dev_iter) return fail(PTMI_EUNSUPPORTED, "ptmi_sup_begin: the stage reads its count on the host: not in ptmi_device_iter mode");
    if (n_in < 1 || n_in > 0x7fffffffll) return fail(PTMI_EINVAL, "ptmi_sup_begin: n_in = %lld outside [1, 2^31)", (long long)n_in);
    if (((uintptr_t)work & 15) != 0 || ((uintptr_t)lp & 7) != 0)
        return fail(PTMI_EINVAL, "ptmi_sup_begin: the work area must be 16-byte aligned, lp 8-byte aligned");
    // the arguments are in order: from here on the call replaces an open stage (a HIP error below leaves none open); a call refused
    // above has changed nothing, an open stage stays open
    h->sup_work = nullptr;
    Work w;
    work_layout((long long)n_in, (char *)work, &w);
    const unsigned nblk = (unsigned)((n_in + LB - 1) / LB);
    hipLaunchKernelGGL(sup_count_kernel, dim3(nblk), dim3(LB), 0, h->stream, w, lp, (long long)n_in);
    hipLaunchKernelGGL(sup_scan_kernel, dim3(1), dim3(LB), 0, h->stream, w, (int)nblk);
    hipLaunchKernelGGL(sup_rank_kernel, dim3(nblk), dim3(LB), 0, h->stream, w, lp, (long long)n_in);
    HIPCHK(hipGetLastError());
    if (!h->h_sup_n) HIPCHK(hipHostMalloc((void **)&h->h_sup_n, sizeof(long long)));
    HIPCHK(hipMemcpyAsync(h->h_sup_n, w.n, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));                  // the stage's one read-back
    h->sup_n = *h->h_sup_n;
    h->sup_nin = (long long)n_in;
    h->sup_work = work;
    *n = (int64_t)h->sup_n;
    return PTMI_OK;
}

int ptmi_sup_rows(ptmi_handle h, void *work, const double *rows_in, double *rows)
{
    if (!h || !work || !rows_in || !rows) return fail(PTMI_EINVAL, "NULL argument");
    if (!h->sup_work) return fail(PTMI_EINVAL, "ptmi_sup_rows: no support stage is open (ptmi_sup_begin first)");
    if (work != h->sup_work) return fail(PTMI_EINVAL, "ptmi_sup_rows: not the work area ptmi_sup_begin was given");
    const int d = h->cfg.ndim;
    const uintptr_t am = d % 2 == 0 ? 15 : 7;
    if (((uintptr_t)rows_in & am) != 0 || ((uintptr_t)rows & am) != 0)
        return fail(PTMI_EINVAL, "ptmi_sup_rows: the rows must be %d-byte aligned", (int)am + 1);
    if (h->sup_n <= 0) return PTMI_OK;
    Work w;
    work_layout(h->sup_nin, (char *)work, &w);
    const int vec = d % 2 == 0 ? 2 : 1, P = d / vec;
    int lsh = 0;
    while (lsh < 6 && (1 << lsh) < P) ++lsh;
    const long long threads = h->sup_n << lsh;
    const unsigned grid = (unsigned)((threads + 255) / 256);
    if (vec == 2) hipLaunchKernelGGL(sup_rows_kernel<2>, dim3(grid), dim3(256), 0, h->stream, (const int32_t *)w.list, h->sup_n, P, lsh, rows_in, rows);
    else hipLaunchKernelGGL(sup_rows_kernel<1>, dim3(grid), dim3(256), 0, h->stream, (const int32_t *)w.list, h->sup_n, P, lsh, rows_in, rows);
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

int ptmi_sup_end(ptmi_handle h, void *work, const double *vals, double *out)
{
    if (!h || !work || !out) return fail(PTMI_EINVAL, "NULL argument");
    if (!h->sup_work) return fail(PTMI_EINVAL, "ptmi_sup_end: no support stage is open (ptmi_sup_begin first)");
    if (work != h->sup_work) return fail(PTMI_EINVAL, "ptmi_sup_end: not the work area ptmi_sup_begin was given");
    if (((uintptr_t)vals & 7) != 0 || ((uintptr_t)out & 7) != 0) return fail(PTMI_EINVAL, "ptmi_sup_end: vals and out must be 8-byte aligned");
    Work w;
    work_layout(h->sup_nin, (char *)work, &w);
    hipLaunchKernelGGL(sup_end_kernel, dim3((unsigned)((h->sup_nin + 255) / 256)), dim3(256), 0, h->stream, (const int32_t *)w.pos, h->sup_nin, vals, out);
    HIPCHK(hipGetLastError());
    h->sup_work = nullptr;
    return PTMI_OK;
}

}  // extern "C"
