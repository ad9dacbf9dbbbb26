// ptmi_aux.hip -- auxiliary jumps as batched device callbacks on the split path (ptmi_aux_attach / ptmi_aux_begin / ptmi_aux_end,
// include/ptmi.h).  The reference runs every auxiliary jump on the result of the cycle entry it picked (PT:1062-1065, PT =
// PTMCMCSampler/PTMCMCSampler.py; added with addAuxilaryJump, PT:1017-1028): q, qxy_aux = aux(x, q, iter, beta); qxy += qxy_aux.  Here the
// stage sits behind the gradient stage (ptmi_gjcb.hip) and the custom-jump stage (ptmi_cj.hip) of a proposal launch and serves EVERY
// chain at once:
//
//   * q is the current proposal buffer itself (ptmi_proposals): on this path a chain's row is contiguous and the rows are in chain slot
//     order, so the caller hands the buffer to its functions as Q [W*T][ndim] -- no copy;
//   * x is what needs a kernel: between a proposal launch and the accept test a chain's state lives in X or in the proposal buffer that
//     does NOT hold the current proposals (sloc, csrc/ptmi_split.hip).  aux_gather_kernel writes every chain's state row into the
//     caller's xrows [W*T][ndim] in slot order, and beta = 1 / T of the chain beside it.  Every chain takes part: no listing, no
//     atomics, no read-back;
//   * the caller runs its functions in turn, each on (xrows, Q, iter, beta) -> (Q', qxy);
//   * ptmi_aux_end copies Q' into the proposal buffer when a function returned a tensor of its own (aux_copy_kernel) and adds the summed
//     qxy to qaux[.][0] (aux_qxy_kernel).
//
// Memory path.  The gather is a row copy with an indirection per row: 8 d bytes in and 8 d bytes out per chain.  A block takes 64
// consecutive chain slots = one contiguous span of the destination and of each of the three possible sources; its threads walk the
// span in 16-byte pieces (8-byte for odd ndim), a wave instruction = 1 KB of consecutive addresses wherever neighbouring chains live
// in the same buffer, four pieces in flight per thread (split_rows_kernel's layout).  The loads are plain, not non-temporal: the
// accept launch that follows reads the same state rows again (the row pass of split_rows_kernel), so this is not their last use
// (non-temporal loads were measured in the engine and gain nothing: DESIGN.md section 3.13), and the gathered rows are stored plainly because the callback reads them next.
#include "ptmi_common.h"

namespace {

constexpr int TILE = 64;             // chain slots per block of the gather
constexpr int UNR = 4;               // pieces in flight per thread

template <int VEC> struct Piece;
template <> struct Piece<2> { typedef ptmi_dev_d2 T; };
template <> struct Piece<1> { typedef double T; };

struct AuxArgs {
    long long nch;
    int d;
    const double *X, *Q, *Q2;        // Q2 == Q on a handle with one proposal buffer
    const int32_t *sloc;             // or nullptr: every state is in X
    const int32_t *temp_of;
    const double *beta;
};

template <int VEC>
__global__ __launch_bounds__(256) void aux_gather_kernel(const AuxArgs a, double *xrows, double *beta_out)
{
    __shared__ int src[TILE];
    const long long c0 = (long long)blockIdx.x * TILE;
    const int ntile = (int)(a.nch - c0 < TILE ? a.nch - c0 : TILE), tid = (int)threadIdx.x;
    if (tid < ntile) {
        const long long ch = c0 + tid;
        src[tid] = a.sloc ? a.sloc[ch] : 0;
        beta_out[ch] = a.beta[a.temp_of[ch]];
    }
    __syncthreads();
    typedef typename Piece<VEC>::T PT;
    const int P = a.d / VEC, total = ntile * P;
    const PT *Xp = reinterpret_cast<const PT *>(a.X + (size_t)c0 * a.d);
    const PT *Q0p = reinterpret_cast<const PT *>(a.Q + (size_t)c0 * a.d);
    const PT *Q1p = reinterpret_cast<const PT *>(a.Q2 + (size_t)c0 * a.d);
    PT *dst = reinterpret_cast<PT *>(xrows + (size_t)c0 * a.d);
    // piece p = tid + 256 j of the tile: chain p / P -- kept current by increments
    const int dc = 256 / P, dp = 256 % P;
    int cl = tid / P, ip = tid % P;
    for (int p0 = tid; p0 < total; p0 += 256 * UNR) {
        PT v[UNR];
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const int p = p0 + 256 * j;
            if (p < total) {
                const int s = src[cl];
                v[j] = s == 0 ? Xp[p] : (s == 1 ? Q0p[p] : Q1p[p]);
            }
            cl += dc; ip += dp;
            if (ip >= P) { ip -= P; cl += 1; }
        }
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const int p = p0 + 256 * j;
            if (p < total) dst[p] = v[j];
        }
    }
}

// ptmi_aux_end, a function returned a tensor of its own: n pieces of it into the proposal buffer
template <int VEC>
__global__ __launch_bounds__(256) void aux_copy_kernel(const double *from, double *to, long long n)
{
    typedef typename Piece<VEC>::T PT;
    const PT *src = reinterpret_cast<const PT *>(from);
    PT *dst = reinterpret_cast<PT *>(to);
    const long long p0 = ((long long)blockIdx.x * UNR) * 256 + threadIdx.x;
    PT v[UNR];
#pragma unroll
    for (int j = 0; j < UNR; ++j)
        if (p0 + 256 * j < n) v[j] = src[p0 + 256 * j];
#pragma unroll
    for (int j = 0; j < UNR; ++j)
        if (p0 + 256 * j < n) dst[p0 + 256 * j] = v[j];
}

// ... and qxy += qxy_aux (PT:1065)
__global__ __launch_bounds__(256) void aux_qxy_kernel(double *qaux, const double *qxy, long long nch)
{
    const long long ch = (long long)blockIdx.x * 256 + threadIdx.x;
    if (ch < nch) qaux[ch * 4] = qaux[ch * 4] + qxy[ch];
}

double *proposals(ptmi_engine *h) { return (h->q_cur && h->buf.Q2) ? h->buf.Q2 : h->buf.Q; }

}  // namespace

extern "C" {

int ptmi_aux_attach(ptmi_handle h)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (!h->buf.Q || !h->buf.qaux) return fail(PTMI_EINVAL, "ptmi_aux_attach: split path needs the Q and qaux buffers");
    if (h->aux_on) return fail(PTMI_EINVAL, "ptmi_aux_attach: already attached");
    if (h->cj_phase != PTMI_GJ_NONE || h->gj_phase != PTMI_GJ_NONE || h->aux_phase != PTMI_GJ_NONE)
        return fail(PTMI_EINVAL, "ptmi_aux_attach: call it before the first ptmi_propose");
    h->aux_on = 1;
    return PTMI_OK;
}

int ptmi_aux_begin(ptmi_handle h, int64_t iter, double *xrows, double *beta)
{
    if (!h || !xrows || !beta) return fail(PTMI_EINVAL, "NULL argument");
    if (!h->aux_on) return fail(PTMI_EINVAL, "ptmi_aux_begin: no auxiliary jumps are attached (ptmi_aux_attach)");
    if (h->dev_iter) return fail(PTMI_EUNSUPPORTED, "ptmi_aux_begin: the stage is driven from the host between the launches: not in ptmi_device_iter mode");
    if (h->gj_phase == PTMI_GJ_PENDING || h->gj_phase == PTMI_GJ_ROUNDS)
        return fail(PTMI_EINVAL, "ptmi_aux_begin(%lld): the auxiliary jumps run on the jump's result (PT:1062): the gradient stage of these proposals has not ended",
                    (long long)iter);
    if (h->cj_phase == PTMI_GJ_PENDING || h->cj_phase == PTMI_GJ_ROUNDS)
        return fail(PTMI_EINVAL, "ptmi_aux_begin(%lld): the auxiliary jumps run on the jump's result (PT:1062): the custom-jump stage of these proposals has not ended",
                    (long long)iter);
    if (h->aux_phase != PTMI_GJ_PENDING || h->gj_iter != (long long)iter)
        return fail(PTMI_EINVAL, "ptmi_aux_begin(%lld): no proposals of that iteration wait for their auxiliary jumps (%s)", (long long)iter,
                    h->aux_phase == PTMI_GJ_PENDING ? "the proposals are another iteration's" : "call it once, after ptmi_propose / ptmi_accept_propose");
    if (((uintptr_t)xrows & 15) != 0) return fail(PTMI_EINVAL, "ptmi_aux_begin: xrows must be 16-byte aligned");
    const ptmi_config &c = h->cfg;
    AuxArgs a;
    a.nch = (long long)c.nwalkers * c.ntemps;
    a.d = c.ndim;
    a.X = h->buf.X; a.Q = h->buf.Q; a.Q2 = h->buf.Q2 ? h->buf.Q2 : h->buf.Q;
    // the row kernels keep a state where its accepted proposal was written (sloc); the shape kernels' split path keeps it in X
    a.sloc = (ptmi_split_rows_ok(h) && h->buf.Q2 && h->buf.sloc) ? h->buf.sloc : nullptr;
    a.temp_of = h->buf.temp_of; a.beta = h->d_beta;
    const unsigned grid = (unsigned)((a.nch + TILE - 1) / TILE);
    if (a.d % 2 == 0) hipLaunchKernelGGL(aux_gather_kernel<2>, dim3(grid), dim3(256), 0, h->stream, a, xrows, beta);
    else hipLaunchKernelGGL(aux_gather_kernel<1>, dim3(grid), dim3(256), 0, h->stream, a, xrows, beta);
    HIPCHK(hipGetLastError());
    h->aux_phase = PTMI_GJ_ROUNDS;
    return PTMI_OK;
}

int ptmi_aux_end(ptmi_handle h, const double *qrows, const double *qxy)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    // the arguments first: a refused call launches nothing and leaves the stage as it was (open: a correct call ends it)
    if (qrows && ((uintptr_t)qrows & 15) != 0) return fail(PTMI_EINVAL, "ptmi_aux_end: qrows must be 16-byte aligned");
    if (h->aux_phase != PTMI_GJ_ROUNDS) return fail(PTMI_EINVAL, "ptmi_aux_end: no auxiliary stage is open (ptmi_aux_begin first)");
    const ptmi_config &c = h->cfg;
    const long long nch = (long long)c.nwalkers * c.ntemps;
    double *Q = proposals(h);
    if (qrows && qrows != Q) {
        const int vec = c.ndim % 2 == 0 ? 2 : 1;
        const long long n = nch * c.ndim / vec;
        const unsigned grid = (unsigned)((n + 256 * UNR - 1) / (256 * UNR));
        if (vec == 2) hipLaunchKernelGGL(aux_copy_kernel<2>, dim3(grid), dim3(256), 0, h->stream, qrows, Q, n);
        else hipLaunchKernelGGL(aux_copy_kernel<1>, dim3(grid), dim3(256), 0, h->stream, qrows, Q, n);
    }
    if (qxy) hipLaunchKernelGGL(aux_qxy_kernel, dim3((unsigned)((nch + 255) / 256)), dim3(256), 0, h->stream, h->buf.qaux, qxy, nch);
    HIPCHK(hipGetLastError());
    h->aux_phase = PTMI_GJ_DONE;
    return PTMI_OK;
}

}  // extern "C"
