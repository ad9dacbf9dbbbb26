// ptmi_abi.hip -- the C ABI of libptmi.so, the engine object, and the kernels of the gradient-jump launch order and the
// self-tests.  See include/ptmi.h for the boundary and DESIGN.md.
#include <math.h>
#include <stdlib.h>

#include <new>
#include <vector>

#include "ptmi_common.h"

// ------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
int ptmi_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// ------------------------------------------------ launch order of the gradient-jump kernel
// Counting sort of the chains by the NUTS step size of their rank (half-octave classes, smallest first = longest
// trees first; a rank that has no step size yet is in class 0: its first call searches for one), then dealt across the
// waves like cards.  The order only decides which chains share a wave; it is not stable and need not be.
__device__ __forceinline__ int gj_class(const double *gj, size_t r)
{
    const double eps = gj[r * GJ_NSTATE + GJ_EPS];
    if (gj[r * GJ_NSTATE + GJ_HAVE_EPS] == 0.0 || !(eps > 0.0)) return 0;
    const int ex = (int)((__double_as_longlong(eps) >> 52) & 0x7FF) - 1023;          // floor(log2 eps)
    const int half = (int)((__double_as_longlong(eps) >> 51) & 1);                   // upper half of the octave
    const int c = 2 * (ex + 24) + half + 1;                                          // eps = 2^-24 -> class 1
    return c < 1 ? 1 : (c > GJ_BUCKETS - 1 ? GJ_BUCKETS - 1 : c);
}
__global__ void gj_order_count_kernel(const double *gj, const int32_t *temp_of, long long nch, int nt, int32_t *bucket)
{
    __shared__ int32_t local[GJ_BUCKETS];                 // most chains fall into two or three classes: count per block first
    for (int b = (int)threadIdx.x; b < GJ_BUCKETS; b += (int)blockDim.x) local[b] = 0;
    __syncthreads();
    const long long ch = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ch < nch) atomicAdd(&local[gj_class(gj, (size_t)(ch / nt) * nt + temp_of[ch])], 1);
    __syncthreads();
    for (int b = (int)threadIdx.x; b < GJ_BUCKETS; b += (int)blockDim.x)
        if (local[b]) atomicAdd(&bucket[b], local[b]);
}
__global__ void gj_order_scan_kernel(int32_t *bucket)
{
    if (threadIdx.x != 0) return;
    int32_t run = 0;
    for (int b = 0; b < GJ_BUCKETS; ++b) { bucket[GJ_BUCKETS + b] = run; run += bucket[b]; bucket[2 * GJ_BUCKETS + b] = 0; }
}
__global__ void gj_order_fill_kernel(const double *gj, const int32_t *temp_of, long long nch, int nt, int32_t *bucket, int32_t *order, int cpw, int nsolo)
{
    // a block reserves its share of every class with one atomic per class; inside the block the order is by thread
    __shared__ int32_t local[GJ_BUCKETS], base[GJ_BUCKETS];
    for (int b = (int)threadIdx.x; b < GJ_BUCKETS; b += (int)blockDim.x) local[b] = 0;
    __syncthreads();
    const long long ch = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int b = ch < nch ? gj_class(gj, (size_t)(ch / nt) * nt + temp_of[ch]) : 0;
    const int mine = ch < nch ? atomicAdd(&local[b], 1) : 0;
    __syncthreads();
    for (int bb = (int)threadIdx.x; bb < GJ_BUCKETS; bb += (int)blockDim.x)
        base[bb] = local[bb] ? atomicAdd(&bucket[2 * GJ_BUCKETS + bb], local[bb]) : 0;
    __syncthreads();
    if (ch >= nch) return;
    // rank t in the sorted list (longest trees first) -> chain slot: consecutive ranks go to DIFFERENT waves, so the few
    // chains with long trees are dealt one per wave and a launch lasts as long as its slowest chain, not the slowest sum
    const long long t = bucket[GJ_BUCKETS + b] + base[b] + mine;
    // the first nsolo chains of the list (the longest trees) get a wave each -- its first chain slot, the others stay empty (-1: the
    // caller fills the array with it) -- and the rest is dealt over the waves behind them
    if (t < nsolo) { order[t * cpw] = (int32_t)ch; return; }
    const long long tr = t - nsolo, nrest = nch - nsolo;
    const long long nw = nrest / cpw, whole = nw * cpw;
    order[(long long)nsolo * cpw + (tr < whole ? (tr % nw) * cpw + tr / nw : tr)] = (int32_t)ch;
}

// ----------------------------------------------------------------- selftest
__global__ void selftest_math_kernel(int op, const double *in, const double *in2, double *out, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = in[i];
    double r;
    switch (op) {
    case 0: r = det_log(x); break;
    case 1: r = det_exp(x); break;
    case 2: r = det_cos2pi(x); break;
    case 3: r = det_sqrt(x); break;
    case 4: r = x / in2[i]; break;
    case 5: r = det_normal((u64)__double_as_longlong(x), (u64)__double_as_longlong(in2[i])); break;
    case 10: r = unit_log((u64)__double_as_longlong(x)); break;
    case 11: case 12: {
        u32 j;
        double t, sn, cs;
        unit_angle64((u64)__double_as_longlong(x), j, t);
        unit_sincos(j, t, sn, cs);
        r = op == 11 ? cs : sn;
        break;
    }
    case 13: {
        u32 j;
        double t, sn, cs;
        unit_angle32((u32)(u64)__double_as_longlong(x), j, t);
        unit_sincos(j, t, sn, cs);
        r = det_sqrt(-2.0 * unit_log((u64)__double_as_longlong(in2[i]))) * cs;
        break;
    }
    default: r = group_sum<16>(x); break;
    }
    out[i] = r;
}
__global__ void selftest_philox_kernel(const u32 *ck, u32 *out, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 *c = ck + i * 6;
    u64 w0, w1;
    philox_words(((u64)c[5] << 32) | c[4], ((u64)c[1] << 32) | c[0], c[2], c[3], w0, w1);
    out[i * 4 + 0] = (u32)w0; out[i * 4 + 1] = (u32)(w0 >> 32);
    out[i * 4 + 2] = (u32)w1; out[i * 4 + 3] = (u32)(w1 >> 32);
}

// ------------------------------------------------------------------- engine
struct Shape { int G, EPL; };
static bool pick_shape(int d, bool grad, Shape *s)
{
    static const Shape table[] = {
#define PTMI_TABLE_ENTRY(G_, E_) {G_, E_},
        PTMI_SHAPE_LIST(PTMI_TABLE_ENTRY)};
    if (d > PTMI_GJ_REG_MAX) grad = false;           // beyond the fused gradient kernels the proposal kernels run in the ordinary 64-lane shape
    const int G = grad ? ptmi_lanes_for_grad(d) : ptmi_lanes_for(d);
    for (const Shape &c : table)
        if (c.G == G && c.G * c.EPL >= d && (!grad || c.EPL <= 8) && (!ptmi_shape_exact(c.G, c.EPL) || c.G * c.EPL == d)) { *s = c; return true; }
    return false;
}

static KArgs make_args(ptmi_engine *h)
{
    KArgs a;
    memset(&a, 0, sizeof(a));
    a.box_off = -1;
    a.tab_off = -1;
    const ptmi_config &c = h->cfg;
    const ptmi_buffers &b = h->buf;
    a.X = b.X; a.lnL = b.lnL; a.lp = b.lp; a.temp_of = b.temp_of; a.slot_of = b.slot_of;
    a.Ut = b.Ut; a.S = b.S; a.DE = b.DE; a.AM = c.temp0 == 0 ? b.AM : nullptr; a.AMaux = c.temp0 == 0 ? b.AMaux : nullptr;
    a.AMflag = c.temp0 == 0 ? (AmFlag *)b.AMflag : nullptr;
    a.rp_draws = h->rp_draws;
    a.nacc = (u64 *)b.nacc; a.jstat = (u64 *)b.jstat; a.cjstat = h->cjstat;
    a.temps_mh = h->d_temps; a.beta = h->d_beta; a.logl_par = h->d_loglpar; a.logp_par = h->d_logppar;
    a.gsize = h->d_gsize; a.gmask = h->d_gmask; a.gcn = h->d_gcn; a.gdiv = h->d_gdiv; a.ngroups = c.ngroups > 1 ? c.ngroups : 1;
    a.Q = b.Q; a.qaux = b.qaux; a.Q2 = nullptr; a.sloc = nullptr; a.q_cur = 0; a.q_tgt = 0;
    a.seed = c.seed;
    a.d = c.ndim; a.nt = c.ntemps; a.W = c.nwalkers; a.ntg = c.ntemps_global; a.temp0 = c.temp0; a.walker0 = c.walker0;
    a.w_host = c.w_host; a.w_scam = c.w_scam; a.w_am = c.w_am; a.w_de = c.w_de; a.de_on = h->de_on; a.de_size = c.de_size; a.de_head = h->de_head;
    a.cov_update = c.cov_update; a.tskip = c.tskip; a.per_walker = c.cov_per_walker; a.logp_kind = c.logp_kind;
    a.pick_walker = c.pick_mode == PTMI_PICK_WALKER;
    a.de_ld = de_row_ld(h->G, h->EPL, c.ndim);
    a.lanes = h->G;
    a.am_epl = am_row_epl(h->G, h->EPL);
    a.w_nuts = c.w_nuts; a.w_hmc = c.w_hmc; a.gj_nburn = c.gj_nburn; a.hmc_min = c.hmc_min; a.hmc_max = c.hmc_max;
    a.nuts_maxdepth = c.nuts_maxdepth; a.hmc_eps = c.hmc_eps; a.nuts_delta = c.nuts_delta;
    a.gj_tab = h->d_gj_tab; a.gj_diag = h->gj_diag; a.gj = b.gj; a.gj_scr = h->d_gj_scr; a.gj_scal = h->d_gj_scal;
    return a;
}

static ptmi_shape_fn shape_fn(int G, int EPL, int L)
{
    if (L == PTMI_LOGL_INTERVAL) {
#define PTMI_PICK_SHAPE3(G_, E_) if (G == G_ && EPL == E_) return ptmi_shape_##G_##_##E_##_3;
        PTMI_GJ_SHAPE_LIST(PTMI_PICK_SHAPE3)
        return nullptr;
    }
#define PTMI_PICK_SHAPE(G_, E_)                                                                        \
    if (G == G_ && EPL == E_) return L == 0 ? ptmi_shape_##G_##_##E_##_0 : (L == 1 ? ptmi_shape_##G_##_##E_##_1 : ptmi_shape_##G_##_##E_##_2);
    PTMI_SHAPE_LIST(PTMI_PICK_SHAPE)
    return nullptr;
}
static int run_shape(ptmi_engine *h, int op, KArgs &a, int grid, bool full)
{
    const int L = (op == PTMI_OP_PROPOSE || op == PTMI_OP_ACCEPT) ? 0 : h->cfg.logl_kind;   // the split kernels live in family 0
    ptmi_shape_fn f = shape_fn(h->G, h->EPL, L);
    if (!f) return fail(PTMI_EUNSUPPORTED, "no kernel shape for ndim=%d", h->cfg.ndim);
    return f(op, h, a, grid, full);
}

// am_row0 / swap_last of a launch; a swap iteration may only be the last one of the range
static int set_step_args(const ptmi_engine *h, KArgs *a)
{
    const ptmi_config &c = h->cfg;
    a->am_row0 = (int)(a->iter0 % c.cov_update);
    if (a->AMflag != nullptr && a->nsteps > 0 && (a->iter0 - 1) / c.cov_update != (a->iter0 + a->nsteps - 2) / c.cov_update && a->iter0 > 0)
        return fail(PTMI_EINVAL, "with AM row flags a launch may not cross a multiple of cov_update (iterations %lld..%lld, cov_update=%d)",
                    a->iter0, a->iter0 + a->nsteps - 1, c.cov_update);
    a->swap_last = 0;
    if (c.tskip > 0 && c.ntemps_global > 1) {
        const long long last = a->iter0 + a->nsteps - 1;
        if (last / c.tskip != (a->iter0 - 1) / c.tskip && last % c.tskip != 0)
            return fail(PTMI_EINVAL, "iterations %lld..%lld contain a swap iteration (Tskip=%d) before their end", a->iter0, last, c.tskip);
        if ((last / c.tskip) - ((a->iter0 - 1) / c.tskip) > 1)
            return fail(PTMI_EINVAL, "iterations %lld..%lld span more than one swap epoch", a->iter0, last);
        a->swap_last = last % c.tskip == 0;
    }
    return PTMI_OK;
}

static int chains_grid(const ptmi_engine *h)
{
    const long long nch = (long long)h->cfg.nwalkers * h->cfg.ntemps;
    const int cpb = 256 / h->G;
    return (int)((nch + cpb - 1) / cpb);
}

extern "C" {

const char *ptmi_last_error(void) { return g_err; }
int ptmi_version(void) { return PTMI_VERSION; }
int ptmi_lanes_for(int ndim) { return ndim <= 104 ? 4 : (ndim <= 416 ? 16 : 64); }
// gradient jumps keep seven chain vectors in registers: at most 8 slots per lane (shapes (4,8), (16,7), (64,8)); beyond 512-d the
// callback path's HMC stage (ptmi_gjcb_wide.hip) keeps them in its work area: 64 lanes up to 2048
int ptmi_lanes_for_grad(int ndim) { return ndim <= 32 ? 4 : (ndim <= 112 ? 16 : (ndim <= 2048 ? 64 : 0)); }

// PT:699-720: geometric ladder T_i = Tmin * tstep^i; the spacing is 1 + sqrt(2/ndim) unless Tmax (> 0) or tstep (> 0)
// fixes it.  Host arithmetic in the reference's operation order (libm pow / exp / log, as NumPy's scalar path).
int ptmi_temperature_ladder(int nchain, int ndim, double Tmin, double Tmax, double tstep, double *out)
{
    if (!out || nchain < 1 || ndim < 1) return fail(PTMI_EINVAL, "ladder: bad argument");
    double step = tstep;
    if (!(step > 0.0)) step = Tmax > 0.0 ? exp(log(Tmax / Tmin) / (double)(nchain - 1)) : 1.0 + sqrt(2.0 / (double)ndim);
    for (int i = 0; i < nchain; ++i) out[i] = nchain > 1 ? Tmin * pow(step, (double)i) : 1.0;
    return PTMI_OK;
}

// doubles per row of the DE buffer and the slots per lane of its piece-cyclic format (0 = rows in element order), see de_update_kernel
int ptmi_de_row_stride(int ndim, int grad, int *stride, int *epl)
{
    Shape s;
    if (!stride || !epl) return fail(PTMI_EINVAL, "NULL argument");
    if (!pick_shape(ndim, grad != 0, &s)) return fail(PTMI_EUNSUPPORTED, "ndim=%d not supported", ndim);
    *stride = de_row_ld(s.G, s.EPL, ndim);
    *epl = s.G == 4 ? s.EPL : 0;
    return PTMI_OK;
}

// row format of the AM buffer for a given ndim (grad != 0: with gradient jumps in the cycle): *epl == 0: parameter order; *epl > 0:
// the lanes' order of the exact 4-lane shape (include/ptmi.h)
int ptmi_am_row_format(int ndim, int grad, int *epl)
{
    Shape s;
    if (!epl) return fail(PTMI_EINVAL, "NULL argument");
    if (!pick_shape(ndim, grad != 0, &s)) return fail(PTMI_EUNSUPPORTED, "ndim=%d not supported", ndim);
    *epl = am_row_epl(s.G, s.EPL);
    return PTMI_OK;
}

int ptmi_device_count(int *count)
{
    if (!count) return fail(PTMI_EINVAL, "count is NULL");
    hipError_t e = hipGetDeviceCount(count);
    if (e != hipSuccess) { *count = 0; return fail(PTMI_ENODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    return PTMI_OK;
}

static int upload(double **dst, const double *src, long long n)
{
    *dst = nullptr;
    if (n <= 0 || !src) return PTMI_OK;
    HIPCHK(hipMalloc((void **)dst, sizeof(double) * (size_t)n));
    HIPCHK(hipMemcpy(*dst, src, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    return PTMI_OK;
}

// AM row flags serve the pooled covariance (the per-walker recurrence of PT:778-794 takes every row in turn) on the GPU that holds
// rank 0
int ptmi_am_flags_ok(const ptmi_config *c)
{
    if (!c) return 0;
    return !c->cov_per_walker && c->temp0 == 0;
}

int ptmi_create(const ptmi_config *cfg, const ptmi_buffers *buf, ptmi_handle *out)
{
    if (!cfg || !buf || !out) return fail(PTMI_EINVAL, "NULL argument");
    *out = nullptr;
    const ptmi_config &c = *cfg;
    if (c.ndim < 1 || c.ntemps < 1 || c.nwalkers < 1) return fail(PTMI_EINVAL, "ndim/ntemps/nwalkers must be >= 1");
    if (c.ntemps_global < c.ntemps || c.temp0 < 0 || c.temp0 + c.ntemps > c.ntemps_global)
        return fail(PTMI_EINVAL, "temperature block [%d,%d) outside ladder of %d", c.temp0, c.temp0 + c.ntemps, c.ntemps_global);
    if (c.w_host < 0 || c.w_scam < 0 || c.w_am < 0 || c.w_de < 0 || c.w_nuts < 0 || c.w_hmc < 0 ||
        c.w_host + c.w_scam + c.w_am + c.w_nuts + c.w_hmc <= 0)
        return fail(PTMI_EINVAL, "No jump proposals specified! (PTMCMCSampler.py:267)");
    if (c.cov_update < 1) return fail(PTMI_EINVAL, "cov_update must be >= 1");
    if (c.w_de > 0 && c.de_size < 2) return fail(PTMI_EINVAL, "de_size must be >= 2 when DE is used");
    if (c.logl_kind < 0 || c.logl_kind > PTMI_LOGL_INTERVAL || c.logp_kind < 0 || c.logp_kind > PTMI_LOGP_BOX)
        return fail(PTMI_EINVAL, "unknown logl/logp kind");
    if (c.logl_kind == PTMI_LOGL_INTERVAL && c.logl_par_len != 3LL * c.ndim)
        return fail(PTMI_EINVAL, "interval logl needs a[d] + w[d] + log w[d] parameters");
    if (c.logl_kind == PTMI_LOGL_INTERVAL && (c.w_host > 0 || c.ngroups > 1))
        return fail(PTMI_EUNSUPPORTED, "the interval logl runs in the fused kernels with one parameter group");
    if (c.logl_kind == PTMI_LOGL_DENSE && c.logl_par_len != (long long)c.ndim * (c.ndim + 1))
        return fail(PTMI_EINVAL, "dense logl needs mu[d] + Pt[d*d] parameters");
    if (c.logl_kind == PTMI_LOGL_CURVED && (c.ndim & 1)) return fail(PTMI_EINVAL, "curved logl needs an even ndim");
    if (c.logp_kind == PTMI_LOGP_BOX && c.logp_par_len != 2LL * c.ndim) return fail(PTMI_EINVAL, "box prior needs lo[d] + hi[d]");
    if (!c.ladder || !c.temps_mh) return fail(PTMI_EINVAL, "ladder / temps_mh missing");
    if (c.ngroups < 0 || c.ngroups > 1024) return fail(PTMI_EINVAL, "ngroups out of range");
    if (c.swap_mode != PTMI_SWAP_SWEEP && c.swap_mode != PTMI_SWAP_ODDEVEN) return fail(PTMI_EINVAL, "unknown swap_mode %d", c.swap_mode);
    if (c.pick_mode != PTMI_PICK_CHAIN && c.pick_mode != PTMI_PICK_WALKER) return fail(PTMI_EINVAL, "unknown pick_mode %d", c.pick_mode);
    if (c.ngroups > 1) {
        if (!c.group_size || !c.group_mask) return fail(PTMI_EINVAL, "group_size / group_mask missing");
        for (int g = 0; g < c.ngroups; ++g)
            if (c.group_size[g] < 1 || c.group_size[g] > c.ndim) return fail(PTMI_EINVAL, "group %d has %d parameters", g, c.group_size[g]);
    }
    const bool gj = c.w_nuts + c.w_hmc > 0;
    const bool gshape = gj || c.logl_kind == PTMI_LOGL_INTERVAL;                     // (the interval family lives in the gradient-jump shapes)
    if (gshape && !gj && c.ndim > 512) return fail(PTMI_EUNSUPPORTED, "the interval logl is built for ndim <= 512 (got %d)", c.ndim);
    if (c.w_nuts < 0 || c.w_hmc < 0) return fail(PTMI_EINVAL, "negative gradient-jump weight");
    if (gj) {
        if (!c.gj_tab) return fail(PTMI_EINVAL, "gradient jumps need the whitening tables (gj_tab)");
        if (!buf->gj) return fail(PTMI_EINVAL, "gradient jumps need the gj buffer");
        if (c.ndim > 2048) return fail(PTMI_EUNSUPPORTED, "gradient jumps on the device stop at ndim 2048 (got %d)", c.ndim);
        // 512 < ndim <= 2048: HMC through the batched gradient stage of a split handle (ptmi_gj_begin / ptmi_gj_step, ptmi_gjcb_wide.hip)
        if (c.ndim > PTMI_GJ_REG_MAX && (c.w_nuts > 0 || !buf->Q || c.logl_kind == PTMI_LOGL_INTERVAL))
            return fail(PTMI_EUNSUPPORTED, "gradient jumps on the device are built for ndim <= 512 (got %d); up to 2048 a split handle "
                                           "(ptmi_buffers.Q) runs HMC alone (w_nuts == 0) through ptmi_gj_begin / ptmi_gj_step", c.ndim);
        // host-served entries beside them: on the split path, where ptmi_cj_attach declares them batched device callbacks (both stages
        // run per proposal launch, on disjoint chains); the fused kernels (ptmi_mh_steps) refuse w_host > 0 whatever else is in the cycle
        if (c.w_host > 0 && !buf->Q) return fail(PTMI_EUNSUPPORTED, "gradient jumps on the device cannot be mixed with host-served jumps (on the split path they can: Q and qaux)");
        if (c.nuts_maxdepth < 0 || c.nuts_maxdepth > 24) return fail(PTMI_EINVAL, "nuts_maxdepth out of range");
        if (c.w_hmc > 0 && (c.hmc_min < 0 || c.hmc_max <= c.hmc_min)) return fail(PTMI_EINVAL, "HMC needs 0 <= hmc_min < hmc_max");
    }
    if (!buf->X || !buf->lnL || !buf->lp || !buf->temp_of || !buf->slot_of || !buf->Ut || !buf->S || !buf->nacc || !buf->jstat)
        return fail(PTMI_EINVAL, "a required device buffer is NULL");
    if (c.w_de > 0 && !buf->DE) return fail(PTMI_EINVAL, "DE weight > 0 but no DE buffer");
    if (buf->AMflag) {
        if (!ptmi_am_flags_ok(cfg)) return fail(PTMI_EINVAL, "AM row flags (ptmi_buffers.AMflag) serve the pooled covariance on the GPU that holds rank 0 (ptmi_am_flags_ok)");
        if (!buf->AM) return fail(PTMI_EINVAL, "AM row flags need the AM buffer");
        if ((long long)c.nwalkers * c.cov_update > 0x7FFFFFFFLL) return fail(PTMI_EINVAL, "AM row flags index rows with 32 bits: nwalkers * cov_update too large");
    }
    if ((unsigned long long)c.nwalkers * (unsigned)c.ntemps_global > 0xFFFFFFFFull) return fail(PTMI_EINVAL, "too many RNG streams");
    Shape s;
    if (!pick_shape(c.ndim, gshape, &s)) return fail(PTMI_EUNSUPPORTED, "ndim=%d not supported (max 2048)", c.ndim);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(PTMI_ENODEVICE, "no HIP device visible: libptmi has no CPU fallback");
    if (c.device < 0 || c.device >= ndev) return fail(PTMI_EINVAL, "device %d of %d", c.device, ndev);
    HIPCHK(hipSetDevice(c.device));
    ptmi_engine *h = new (std::nothrow) ptmi_engine();
    if (!h) return fail(PTMI_EINVAL, "out of host memory");
    memset(h, 0, sizeof(*h));
    h->cfg = c; h->buf = *buf; h->stream = (hipStream_t)c.stream; h->G = s.G; h->EPL = s.EPL;
    std::vector<double> beta((size_t)c.ntemps);
    for (int t = 0; t < c.ntemps; ++t) beta[(size_t)t] = 1.0 / c.temps_mh[t];   // 1/self.temp, PT:612
    // likelihood parameters on the device.  Dense: mu | Pt | Tl, Tl = the half of the symmetric part of P the VALUE is summed over
    // (Tl[k][i] = Ps[k][i] for k > i, Ps[i][i] / 2 for k == i, 0 for k < i: -r^T P r / 2 = -sum_i r_i sum_{k >= i} Tl[k][i] r_k,
    // half the products of the full form; the oracle's dense_par builds the same table); Pt stays for the gradient -P r
    std::vector<double> loglpar(c.logl_par, c.logl_par + (c.logl_par ? c.logl_par_len : 0));
    if (c.logl_kind == PTMI_LOGL_DENSE) {
        const size_t d = (size_t)c.ndim;
        loglpar.resize(d + 2 * d * d, 0.0);
        const double *Pt = loglpar.data() + d;
        double *Tl = loglpar.data() + d + d * d;
        for (size_t k = 0; k < d; ++k)
            for (size_t i = 0; i <= k; ++i) {
                const double ps = (Pt[k * d + i] + Pt[i * d + k]) * 0.5;
                Tl[k * d + i] = k == i ? ps * 0.5 : ps;
            }
    }
    int rc;
    if ((rc = upload(&h->d_ladder, c.ladder, c.ntemps_global)) || (rc = upload(&h->d_temps, c.temps_mh, c.ntemps)) ||
        (rc = upload(&h->d_beta, beta.data(), c.ntemps)) || (rc = upload(&h->d_loglpar, loglpar.data(), (long long)loglpar.size())) ||
        (rc = upload(&h->d_logppar, c.logp_par, c.logp_par_len))) {
        ptmi_destroy(h);
        return rc;
    }
    {   // per-group constants of the AM / DE scales: 2.4/sqrt(2 n_g) (PT:928) and sqrt(2 n_g) (PT:976)
        const int Ng = c.ngroups > 1 ? c.ngroups : 1;
        std::vector<double> gcn((size_t)Ng), gdiv((size_t)Ng), gmask((size_t)Ng * c.ndim, 1.0);
        std::vector<int32_t> gsize((size_t)Ng, c.ndim);
        for (int g = 0; g < Ng; ++g) {
            if (c.ngroups > 1) gsize[(size_t)g] = c.group_size[g];
            gcn[(size_t)g] = 2.4 / sqrt(2.0 * (double)gsize[(size_t)g]);
            gdiv[(size_t)g] = sqrt(2.0 * (double)gsize[(size_t)g]);
        }
        if (c.ngroups > 1) memcpy(gmask.data(), c.group_mask, sizeof(double) * gmask.size());
        h->gsize_host = (int32_t *)malloc(sizeof(int32_t) * Ng);
        if (h->gsize_host) memcpy(h->gsize_host, gsize.data(), sizeof(int32_t) * Ng);
        hipError_t e2 = h->gsize_host ? hipMalloc((void **)&h->d_gsize, sizeof(int32_t) * Ng) : hipErrorOutOfMemory;
        if (e2 == hipSuccess) e2 = hipMemcpy(h->d_gsize, gsize.data(), sizeof(int32_t) * Ng, hipMemcpyHostToDevice);
        if (e2 != hipSuccess || (rc = upload(&h->d_gcn, gcn.data(), Ng)) || (rc = upload(&h->d_gdiv, gdiv.data(), Ng)) ||
            (rc = upload(&h->d_gmask, gmask.data(), (long long)gmask.size()))) {
            ptmi_destroy(h);
            return e2 != hipSuccess ? fail(PTMI_EHIP, "group tables: %s", hipGetErrorString(e2)) : rc;
        }
    }
    if (gj && c.ndim > PTMI_GJ_REG_MAX) {                                            // the callback path alone: the tables, no scratch of the fused kernels
        if ((rc = upload(&h->d_gj_tab, c.gj_tab, 3LL * c.ndim * c.ndim))) {
            ptmi_destroy(h);
            return rc;
        }
    } else if (gj) {
        const size_t nch = (size_t)c.nwalkers * c.ntemps, lanes = (size_t)s.G * s.EPL;
        const size_t nvec = (size_t)GJV_TOP + (size_t)GJL_VECS * (c.nuts_maxdepth + 1);
        hipError_t e3 = hipMalloc((void **)&h->d_gj_scr, sizeof(double) * nvec * lanes * nch);
        if (e3 == hipSuccess) e3 = hipMalloc((void **)&h->d_gj_scal, sizeof(double) * (size_t)GJS_SCALARS * (c.nuts_maxdepth + 1) * nch);
        // chains with a wave of their own (the longest trees of the launch order): up to 1024, a 32nd of the chains at most (config-5 share
        // with 0 / 128 / 512 / 1024 / 2048 of 65 536: 4.67e8 / 4.92e8 / 4.82e8 / 5.37e8 / 5.18e8 updates/s); PTMI_GJ_SOLO=n overrides (0: none; a
        // test hook: the order never enters a chain's arithmetic)
        const int cpw = 64 / s.G;
        long long solo = cpw > 1 ? (long long)ptmi_env("PTMI_GJ_SOLO", (double)(nch / 32 < 1024 ? nch / 32 : 1024)) : 0;
        if (solo > (long long)nch) solo = (long long)nch;
        if (solo < 0) solo = 0;
        h->gj_solo = (int)solo;
        if (e3 == hipSuccess) e3 = hipMalloc((void **)&h->d_gj_order, sizeof(int32_t) * (nch + (size_t)solo * cpw + cpw));
        if (e3 == hipSuccess) e3 = hipMalloc((void **)&h->d_gj_bucket, sizeof(int32_t) * 3 * GJ_BUCKETS);
        if (e3 != hipSuccess || (rc = upload(&h->d_gj_tab, c.gj_tab, 3LL * c.ndim * c.ndim))) {
            ptmi_destroy(h);
            return e3 != hipSuccess ? fail(PTMI_EHIP, "gradient-jump scratch: %s", hipGetErrorString(e3)) : rc;
        }
    }
    if (gj) {
        // diagonal whitening (cov0 diagonal: the curved-likelihood runs start from the identity): a product is d multiplications
        // (the oracle's tab_vec defines the same rule)
        h->gj_diag = 1;
        for (long long i = 0; i < 3LL * c.ndim * c.ndim && h->gj_diag; ++i) {
            const long long r = (i / c.ndim) % c.ndim, col = i % c.ndim;
            if (r != col && c.gj_tab[i] != 0.0) h->gj_diag = 0;
        }
    }
    h->cfg.gj_tab = nullptr;
    h->cfg.ladder = h->cfg.temps_mh = h->cfg.logl_par = h->cfg.logp_par = h->cfg.group_mask = nullptr;  // host copies are not kept
    h->cfg.group_size = nullptr;
    hipError_t e = hipMalloc((void **)&h->d_pre, PTMI_SWAP_PRE_BYTES * (size_t)c.nwalkers * c.ntemps_global);
    if (e == hipSuccess && !c.cov_per_walker && c.temp0 == 0) e = ptmi_pool_scratch_alloc(h);
    // AM increments ahead of the launch (am_gemm_kernel): the 16- and 64-lane shapes with one pooled table, ndim <= 1024
    // ... and every shape with parameter groups (PT:129-145: a chain's pick has its own group, hence its own table: the step kernels'
    // matrix-core product shares one table between the 16 chains of a wave, and the vector-pipe product they fall back to takes
    // 284 ms per 100 steps of the default mix at 64 x 4096 x 100-d with three groups -- 35 times the one-group kernel)
    // -- with groups also per-walker covariances (an event's table is then its walker's group table: lists per (walker, group)): 505 ms
    // per 100 steps of the default mix at 64 x 4096 x 100-d with three groups before
    // -- and the gradient-jump shapes at 16 / 64 lanes per chain (the interval family, NUTS / HMC cycles at ndim > 32): their step kernels'
    // own AM product is the vector pipe's too
    // -- and per-walker covariances at 16 / 64 lanes per chain without groups (one key per walker)
    // -- and the SPLIT path of every shape (ptmi_propose / ptmi_accept_propose on contiguous rows, csrc/ptmi_split.hip): an AM pick's 2 d^2
    // flop belong on the matrix cores there too; the row kernel reads the increment as it reads a SCAM direction.  For handles the fused
    // kernels do not take this way (4 lanes per chain, one group: their own matrix-core product) the scratch serves the split path alone.
    const bool am_main = c.w_am > 0 && (c.ngroups > 1 || s.G > 4) && c.ndim <= 1024 && c.w_host == 0;
    const bool am_split = !am_main && buf->Q != nullptr && c.w_am > 0 && c.ndim <= 1024 && c.w_host == 0;
    if (e == hipSuccess && (am_main || am_split)) e = ptmi_am_scratch_alloc(h, am_main);
    if (e == hipSuccess) e = hipEventCreate(&h->ev0);
    if (e == hipSuccess) e = hipEventCreate(&h->ev1);
    if (e != hipSuccess) { ptmi_destroy(h); return fail(PTMI_EHIP, "create: %s", hipGetErrorString(e)); }
    *out = h;
    return PTMI_OK;
}

int ptmi_destroy(ptmi_handle h)
{
    if (!h) return PTMI_OK;
    (void)hipFree(h->d_ladder); (void)hipFree(h->d_temps); (void)hipFree(h->d_beta); (void)hipFree(h->d_loglpar); (void)hipFree(h->d_logppar);
    (void)hipFree(h->d_pre); (void)hipFree(h->d_xint); (void)hipFree(h->d_hop);
    if (h->h_hop) { (void)hipHostFree(h->h_hop); (void)hipEventDestroy(h->hop_ev); }
    (void)hipFree(h->d_gsize); (void)hipFree(h->d_gmask); (void)hipFree(h->d_gcn); (void)hipFree(h->d_gdiv); (void)hipFree(h->d_pool_part); (void)hipFree(h->d_pool_T);
    (void)hipFree(h->d_ql_scr); (void)hipFree(h->d_qlw_scr); (void)hipFree(h->d_qlg_scr); (void)hipFree(h->d_sy_scr); (void)hipFree(h->d_utpad);
    free(h->gsize_host);
    ptmi_dc_plan_free(h);
    if (h->h_sy_info) (void)hipHostFree(h->h_sy_info);
    (void)hipFree(h->d_rle_ent); (void)hipFree(h->d_rle_cnt);
    (void)hipFree(h->d_am_ev); (void)hipFree(h->d_am_count); (void)hipFree(h->d_am_base); (void)hipFree(h->d_am_inc);
    (void)hipFree(h->d_am_grp); (void)hipFree(h->d_am_perm); (void)hipFree(h->d_am_kbase); (void)hipFree(h->d_am_next); (void)hipFree(h->d_iter);
    if (h->h_gj_n) (void)hipHostFree(h->h_gj_n);
    (void)hipFree(h->d_cj_fun);
    if (h->h_cj_offs) (void)hipHostFree(h->h_cj_offs);
    if (h->h_sup_n) (void)hipHostFree(h->h_sup_n);
    ptmi_hist_free(h);
    ptmi_ev_free(h);
    ptmi_diag_free(h);
    ptmi_ladder_free(h);
    ptmi_pairs_free(h);
    ptmi_samples_free(h);
    ptmi_best_free(h);
    (void)hipFree(h->d_gj_tab); (void)hipFree(h->d_gj_scr); (void)hipFree(h->d_gj_scal); (void)hipFree(h->d_gj_order); (void)hipFree(h->d_gj_bucket);
    if (h->side) { (void)hipStreamDestroy(h->side); (void)hipEventDestroy(h->side_go); (void)hipEventDestroy(h->side_done); }
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    delete h;
    return PTMI_OK;
}

int ptmi_sync(ptmi_handle h)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    HIPCHK(hipStreamSynchronize(h->stream));
    return PTMI_OK;
}

int ptmi_set_de_active(ptmi_handle h, int on)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (on && (h->cfg.w_de <= 0 || !h->buf.DE)) return fail(PTMI_EINVAL, "DE has no weight or no buffer");
    h->de_on = on ? 1 : 0;
    h->split_am_lo = h->split_am_hi = 0;                         // the cycle changed: increments made ahead (ptmi_split_am_prepare) are void
    return PTMI_OK;
}

int ptmi_eval_state(ptmi_handle h)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    const KArgs a = make_args(h);
    const int grid = chains_grid(h);
    KArgs aa = a;
    if (int rc = run_shape(h, PTMI_OP_EVAL, aa, grid, false)) return rc;
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

// rows of ld >= d doubles, zero beyond column d: the 16- / 64-lane step kernels read a row with unconditional loads
__global__ __launch_bounds__(256) void ut_pad_kernel(const double *Ut, double *out, int d, int ld, unsigned long long *absmax)
{
    const double *src = Ut + (size_t)blockIdx.x * d;
    double *dst = out + (size_t)blockIdx.x * ld;
    double am = 0.0;
    for (int i = (int)threadIdx.x; i < ld; i += 256) {
        const double v = i < d ? src[i] : 0.0;
        dst[i] = v;
        am = __builtin_fabs(v) > am ? __builtin_fabs(v) : am;
    }
    // max |U| of the table (non-negative doubles order like their bit patterns): the box prior's fast path bounds a SCAM jump by it
    for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_xor(am, o, 64); am = t > am ? t : am; }
    if ((threadIdx.x & 63) == 0) atomicMax(absmax, (unsigned long long)__double_as_longlong(am));
}
// ONE table for the launch and a wide shape: the padded copy the step kernels read (the caller's Ut may have changed since the
// last launch -- an epoch, put_eig -- so it is made anew every launch: 16 MB of traffic at ndim = 1000 beside a launch of milliseconds)
static int make_ut_pad(ptmi_engine *h, KArgs *a)
{
    const ptmi_config &c = h->cfg;
    a->UtPad = nullptr;
    a->ut_pad_ld = 0;
    a->ut_absmax = nullptr;
    if (h->G <= 4 || c.cov_per_walker || c.ngroups > 1) return PTMI_OK;
    const int ld = h->G * h->EPL;
    if (!h->d_utpad) HIPCHK(hipMalloc((void **)&h->d_utpad, sizeof(double) * ((size_t)c.ndim * ld + 2)));
    unsigned long long *amax = (unsigned long long *)(h->d_utpad + (size_t)c.ndim * ld);
    HIPCHK(hipMemsetAsync(amax, 0, sizeof(unsigned long long), h->stream));
    hipLaunchKernelGGL(ut_pad_kernel, dim3(c.ndim), dim3(256), 0, h->stream, (const double *)h->buf.Ut, h->d_utpad, c.ndim, ld, amax);
    a->UtPad = h->d_utpad;
    a->ut_pad_ld = ld;
    a->ut_absmax = (const double *)amax;
    return PTMI_OK;
}

int ptmi_mh_steps(ptmi_handle h, int64_t iter0, int32_t nsteps)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (nsteps < 0 || iter0 < 0) return fail(PTMI_EINVAL, "iter0/nsteps negative");
    if (h->cfg.w_nuts + h->cfg.w_hmc > 0 && h->cfg.ndim > PTMI_GJ_REG_MAX)
        return fail(PTMI_EUNSUPPORTED, "ptmi_mh_steps: the fused gradient kernels are built for ndim <= 512 (got %d); beyond, HMC runs on the "
                                       "split path (ptmi_propose / ptmi_gj_begin / ptmi_gj_step)", h->cfg.ndim);
    if (nsteps == 0) return PTMI_OK;
    KArgs a = make_args(h);
    a.iter0 = iter0; a.nsteps = nsteps;
    if (int rc = set_step_args(h, &a)) return rc;
    if (h->cfg.w_host > 0) return fail(PTMI_EINVAL, "host-served jumps need the split path (ptmi_propose / ptmi_accept)");
    const bool gjc = h->cfg.w_nuts + h->cfg.w_hmc > 0;       // the fused kernel with the NUTS / HMC branch (csrc/ptmi_gj.inc.h)
    auto launch_gj = [&](KArgs &a) -> int {
        if (h->cfg.w_nuts > 0 && h->d_gj_order) {                                   // chains of similar step size share a wave
            const long long nch = (long long)h->cfg.nwalkers * h->cfg.ntemps;
            const unsigned g = (unsigned)((nch + 255) / 256);
            HIPCHK(hipMemsetAsync(h->d_gj_bucket, 0, sizeof(int32_t) * GJ_BUCKETS, h->stream));
            hipLaunchKernelGGL(gj_order_count_kernel, dim3(g), dim3(256), 0, h->stream, (const double *)h->buf.gj, (const int32_t *)h->buf.temp_of,
                               nch, h->cfg.ntemps, h->d_gj_bucket);
            hipLaunchKernelGGL(gj_order_scan_kernel, dim3(1), dim3(64), 0, h->stream, h->d_gj_bucket);
            const int cpw = 64 / h->G;
            const long long nslots = (long long)h->gj_solo * cpw + ((nch - h->gj_solo + cpw - 1) / cpw) * cpw;
            HIPCHK(hipMemsetAsync(h->d_gj_order, 0xFF, sizeof(int32_t) * (size_t)nslots, h->stream));           // -1: an empty chain slot
            hipLaunchKernelGGL(gj_order_fill_kernel, dim3(g), dim3(256), 0, h->stream, (const double *)h->buf.gj, (const int32_t *)h->buf.temp_of,
                               nch, h->cfg.ntemps, h->d_gj_bucket, h->d_gj_order, cpw, h->gj_solo);
            a.gj_order = h->d_gj_order;
            a.gj_nslots = (int)nslots;
        }
        if (int rc = run_shape(h, PTMI_OP_MH_GJ, a, chains_grid(h), true)) return rc;
        h->last_variant = PTMI_VAR_GRADJUMP | PTMI_VAR_FULL;
        if (a.gj_order) h->gj_last[0] |= PTMI_GJL_ORDERED;
        return PTMI_OK;
    };
    if (gjc && h->am_piece <= 0) {
        if (int rc = launch_gj(a)) return rc;
        HIPCHK(hipGetLastError());
        return PTMI_OK;
    }
    const bool full = h->cfg.w_am > 0 || (h->de_on && h->cfg.w_de > 0);
    if (!full && h->cfg.w_scam <= 0 && !gjc) return fail(PTMI_EINVAL, "empty proposal cycle");
    const int grid = chains_grid(h);
    if (!gjc)
        if (int rc = make_ut_pad(h, &a)) return rc;
    if (h->am_piece > 0) {
        // large ndim: the launch goes in pieces, each behind the matrix product that computes its AM increments
        const ptmi_config &c = h->cfg;
        const long long nch = (long long)c.nwalkers * c.ntemps;
        for (int s0 = 0; s0 < nsteps; s0 += h->am_piece) {
            const int ns = nsteps - s0 < h->am_piece ? nsteps - s0 : h->am_piece;
            if (int rc = ptmi_am_prepare(h, iter0 + s0, ns)) return rc;
            KArgs ap = make_args(h);
            ap.iter0 = iter0 + s0; ap.nsteps = ns;
            if (int rc = set_step_args(h, &ap)) return rc;
            ap.am_inc = h->d_am_inc; ap.am_base = h->d_am_base;
            ap.UtPad = a.UtPad; ap.ut_pad_ld = a.ut_pad_ld; ap.ut_absmax = a.ut_absmax;
            if (gjc) {                                                   // (the gradient-jump kernel reads its AM increments the same way)
                if (int rc = launch_gj(ap)) return rc;
                h->gj_last[0] |= PTMI_GJL_AM_AHEAD;
                continue;
            }
            if (int rc = run_shape(h, PTMI_OP_MH, ap, grid, full)) return rc;
        }
        HIPCHK(hipGetLastError());
        return PTMI_OK;
    }
    if (int rc = run_shape(h, PTMI_OP_MH, a, grid, full)) return rc;
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

int ptmi_last_mh_variant(ptmi_handle h, int32_t *variant)
{
    if (!h || !variant) return fail(PTMI_EINVAL, "NULL argument");
    *variant = h->last_variant | ((h->cfg.pick_mode == PTMI_PICK_WALKER && (h->last_variant & PTMI_VAR_FULL)) ? PTMI_VAR_UNIFORM : 0) |
               (h->G << 12) | (h->EPL << 20);
    return PTMI_OK;
}

int ptmi_last_gj_launch(ptmi_handle h, int32_t *layout, int32_t *lds_levels, int32_t *lds_bytes, int32_t *nslots)
{
    if (!h || !layout || !lds_levels || !lds_bytes || !nslots) return fail(PTMI_EINVAL, "NULL argument");
    *layout = h->gj_last[0]; *lds_levels = h->gj_last[1]; *lds_bytes = h->gj_last[2]; *nslots = h->gj_last[3];
    return PTMI_OK;
}

// HMC and NUTS on the split path (ptmi_gjcb.hip): proposals of `iter` were just made -- with gradient jumps in the cycle their gradient
// stage is pending
static void gj_proposed(ptmi_engine *h, long long iter)
{
    h->gj_phase = h->cfg.w_nuts + h->cfg.w_hmc > 0 ? PTMI_GJ_PENDING : PTMI_GJ_NONE;
    h->gj_iter = iter;
    // ... and with batched custom jumps attached (ptmi_cj.hip) their stage
    h->cj_phase = h->cj_nfun > 0 ? PTMI_GJ_PENDING : PTMI_GJ_NONE;
    h->cj_iter = iter;
    // ... and with auxiliary jumps attached (ptmi_aux.hip) theirs, behind the other two
    h->aux_phase = h->aux_on ? PTMI_GJ_PENDING : PTMI_GJ_NONE;
}
// ... and an accept test may only read them once that stage is over
static int gj_stage_over(const ptmi_engine *h, const char *who, int64_t iter)
{
    if (h->gj_phase == PTMI_GJ_PENDING || h->gj_phase == PTMI_GJ_ROUNDS)
        return fail(PTMI_EINVAL, "%s(%lld): the HMC / NUTS proposals of iteration %lld are not made yet -- ptmi_gj_begin and ptmi_gj_step until n = 0 first",
                    who, (long long)iter, h->gj_iter);
    if (h->cj_phase == PTMI_GJ_PENDING || h->cj_phase == PTMI_GJ_ROUNDS)
        return fail(PTMI_EINVAL, "%s(%lld): the custom jumps' proposals of iteration %lld are not made yet -- ptmi_cj_begin, the callbacks, ptmi_cj_end first",
                    who, (long long)iter, h->cj_iter);
    if (h->aux_phase == PTMI_GJ_PENDING || h->aux_phase == PTMI_GJ_ROUNDS)
        return fail(PTMI_EINVAL, "%s(%lld): the auxiliary jumps of the proposals of iteration %lld have not run yet -- ptmi_aux_begin, the callbacks, ptmi_aux_end first",
                    who, (long long)iter, h->gj_iter);
    return PTMI_OK;
}

// ptmi_device_iter: the split calls' `iter` is an offset from the counter in device memory (launches captured in a graph).  The row
// kernels derive the ring row and the swap-iteration test from the counter themselves; what the host cannot know then it cannot check.
static int split_iter_args(ptmi_engine *h, KArgs *a, int mode)
{
    if (!h->dev_iter) return set_step_args(h, a);
    if (!ptmi_split_rows_ok(h) || h->cfg.w_am > 0)
        return fail(PTMI_EUNSUPPORTED, "ptmi_device_iter serves the row kernels' cycles without AM entries (the AM increments are listed on the host's iteration)");
    (void)mode;
    a->iter_dev = h->d_iter;
    a->am_row0 = 0; a->swap_last = 0;
    return PTMI_OK;
}

// The AM increments the split path's row kernel reads for the proposals of iteration `it`: the prepared piece when it covers `it`
// (ptmi_split_am_prepare), else a piece of that one iteration made now (the tables as they are at this call).
static int split_am_args(ptmi_engine *h, KArgs *a, long long it)
{
    if (h->cfg.w_am <= 0) return PTMI_OK;
    if (!(it >= h->split_am_lo && it < h->split_am_hi))
        if (int rc = ptmi_split_am_prepare(h, it, 1)) return rc;
    a->am_inc = h->d_am_inc;
    a->am_next = h->d_am_next;
    return PTMI_OK;
}

int ptmi_propose(ptmi_handle h, int64_t iter)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (!h->buf.Q || !h->buf.qaux) return fail(PTMI_EINVAL, "split path needs the Q and qaux buffers");
    if (int rc = ptmi_gj_split_check(h)) return rc;
    KArgs a = make_args(h);
    a.iter0 = iter; a.nsteps = 1;
    if (int rc = split_iter_args(h, &a, 0)) return rc;
    h->q_cur = 0;                                            // the proposals go to Q
    if (ptmi_split_rows_ok(h)) {
        if (h->buf.Q2 && h->buf.sloc) { a.Q2 = h->buf.Q2; a.sloc = h->buf.sloc; }
        if (int rc = split_am_args(h, &a, iter)) return rc;
        if (int rc = ptmi_split_rows(h, a, 0)) return rc;
    } else {
        const int grid = chains_grid(h);
        if (int rc = run_shape(h, PTMI_OP_PROPOSE, a, grid, true)) return rc;
    }
    HIPCHK(hipGetLastError());
    gj_proposed(h, iter);
    return PTMI_OK;
}

int ptmi_accept(ptmi_handle h, int64_t iter, const double *newlnL, const double *newlp)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (!h->buf.Q || !h->buf.qaux || !newlnL || !newlp) return fail(PTMI_EINVAL, "split path buffers missing");
    if (int rc = gj_stage_over(h, "ptmi_accept", iter)) return rc;
    KArgs a = make_args(h);
    a.iter0 = iter; a.nsteps = 1; a.newlnL = newlnL; a.newlp = newlp;
    if (int rc = split_iter_args(h, &a, 1)) return rc;
    if (ptmi_split_rows_ok(h)) {
        if (h->buf.Q2 && h->buf.sloc) { a.Q2 = h->buf.Q2; a.sloc = h->buf.sloc; }
        a.q_cur = h->q_cur;
        if (int rc = ptmi_split_rows(h, a, 1)) return rc;
    } else {
        const int grid = chains_grid(h);
        if (int rc = run_shape(h, PTMI_OP_ACCEPT, a, grid, true)) return rc;
    }
    HIPCHK(hipGetLastError());
    h->gj_phase = PTMI_GJ_NONE;
    h->cj_phase = PTMI_GJ_NONE;
    h->aux_phase = PTMI_GJ_NONE;
    return PTMI_OK;
}

int ptmi_accept_propose(ptmi_handle h, int64_t iter, const double *newlnL, const double *newlp)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (!h->buf.Q || !h->buf.qaux || !newlnL || !newlp) return fail(PTMI_EINVAL, "split path buffers missing");
    const ptmi_config &c = h->cfg;
    // nothing may sit between the two iterations: a swap (iter a multiple of Tskip), a covariance or DE epoch (the caller's: they
    // change the tables the proposal of iter + 1 reads)
    if (!h->dev_iter && c.tskip > 0 && c.ntemps_global > 1 && iter % c.tskip == 0)
        return fail(PTMI_EINVAL, "ptmi_accept_propose(%lld): a swap iteration (Tskip=%d) is accepted with ptmi_accept, the swap follows", (long long)iter, c.tskip);
    if (int rc = ptmi_gj_split_check(h)) return rc;
    if (int rc = gj_stage_over(h, "ptmi_accept_propose", iter)) return rc;
    KArgs a = make_args(h);
    a.iter0 = iter; a.nsteps = 1; a.newlnL = newlnL; a.newlp = newlp;
    if (int rc = split_iter_args(h, &a, 2)) return rc;
    if (ptmi_split_rows_ok(h)) {
        a.q_cur = a.q_tgt = h->q_cur;
        if (h->buf.Q2 && h->buf.sloc) { a.Q2 = h->buf.Q2; a.sloc = h->buf.sloc; a.q_tgt = 1 - h->q_cur; }
        if (int rc = split_am_args(h, &a, iter + 1)) return rc;
        if (int rc = ptmi_split_rows(h, a, 2)) return rc;
        h->q_cur = a.q_tgt;
        HIPCHK(hipGetLastError());
        gj_proposed(h, iter + 1);
        return PTMI_OK;
    }
    // configurations the row kernels do not serve (AM entries in the cycle): the two shape kernels back to back
    const int grid = chains_grid(h);
    if (int rc = run_shape(h, PTMI_OP_ACCEPT, a, grid, true)) return rc;
    KArgs b = make_args(h);
    b.iter0 = iter + 1; b.nsteps = 1;
    if (int rc = set_step_args(h, &b)) return rc;
    if (int rc = run_shape(h, PTMI_OP_PROPOSE, b, grid, true)) return rc;
    HIPCHK(hipGetLastError());
    gj_proposed(h, iter + 1);
    return PTMI_OK;
}

int ptmi_rows_logl(ptmi_handle h, const double *rows, int64_t n, double *out)
{
    if (!h || !rows || !out || n < 0) return fail(PTMI_EINVAL, "bad argument");
    const int L = h->cfg.logl_kind;
    if (L != PTMI_LOGL_ISO && L != PTMI_LOGL_DENSE)
        return fail(PTMI_EUNSUPPORTED, "ptmi_rows_logl serves the isotropic and the dense Gaussian (PTMI_LOGL_ISO, PTMI_LOGL_DENSE)");
    if (n == 0) return PTMI_OK;
    if (int rc = L == PTMI_LOGL_ISO ? ptmi_rows_iso(h, rows, (long long)n, out) : ptmi_rows_dense(h, rows, (long long)n, out, nullptr)) return rc;
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

int ptmi_rows_logl_grad(ptmi_handle h, const double *rows, int64_t n, double *lnl, double *dlnl)
{
    if (!h || !rows || !lnl || !dlnl || n < 0) return fail(PTMI_EINVAL, "bad argument");
    const int L = h->cfg.logl_kind;
    if (L != PTMI_LOGL_ISO && L != PTMI_LOGL_DENSE)
        return fail(PTMI_EUNSUPPORTED, "ptmi_rows_logl_grad serves the isotropic and the dense Gaussian (PTMI_LOGL_ISO, PTMI_LOGL_DENSE)");
    if (n == 0) return PTMI_OK;
    if (L == PTMI_LOGL_ISO) {
        if (int rc = ptmi_rows_iso(h, rows, (long long)n, lnl)) return rc;
        if (int rc = ptmi_rows_neg(h, rows, (long long)n, dlnl)) return rc;
    } else if (int rc = ptmi_rows_dense(h, rows, (long long)n, lnl, dlnl)) return rc;
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

int ptmi_rows_logp(ptmi_handle h, const double *rows, int64_t n, double *lp, double *dlp)
{
    if (!h || !rows || !lp || n < 0) return fail(PTMI_EINVAL, "bad argument");
    if (n == 0) return PTMI_OK;
    if (int rc = ptmi_rows_prior(h, rows, (long long)n, lp)) return rc;
    HIPCHK(hipGetLastError());
    if (dlp) HIPCHK(hipMemsetAsync(dlp, 0, sizeof(double) * (size_t)n * h->cfg.ndim, h->stream));      // the built-in priors are flat where finite
    return PTMI_OK;
}

int ptmi_set_proposals(ptmi_handle h, int32_t which)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    h->q_cur = (which && h->buf.Q2) ? 1 : 0;
    return PTMI_OK;
}

int ptmi_set_stream(ptmi_handle h, void *stream)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    h->stream = (hipStream_t)stream;
    h->cfg.stream = stream;
    return PTMI_OK;
}

int ptmi_device_iter(ptmi_handle h, int32_t on)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (on && !h->d_iter) HIPCHK(hipMalloc((void **)&h->d_iter, sizeof(long long)));
    h->dev_iter = on ? 1 : 0;
    return PTMI_OK;
}

int ptmi_set_device_iter(ptmi_handle h, int64_t value)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (!h->d_iter) HIPCHK(hipMalloc((void **)&h->d_iter, sizeof(long long)));
    if (int rc = ptmi_set_iter_device(h, h->d_iter, (long long)value)) return rc;
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

int ptmi_proposals(ptmi_handle h, double **q)
{
    if (!h || !q) return fail(PTMI_EINVAL, "NULL argument");
    *q = (h->q_cur && h->buf.Q2) ? h->buf.Q2 : h->buf.Q;
    return PTMI_OK;
}

int ptmi_test_replay(ptmi_handle h, const double *swap_uniforms, const uint64_t *draws)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    h->rp_swap_u = swap_uniforms;
    h->rp_draws = (const u64 *)draws;
    return PTMI_OK;
}

int ptmi_selftest_math(int device, int op, const double *in, const double *in2, double *out, int64_t n)
{
    if (!in || !out || n < 0) return fail(PTMI_EINVAL, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(PTMI_ENODEVICE, "no HIP device visible");
    HIPCHK(hipSetDevice(device));
    double *di = nullptr, *di2 = nullptr, *dout = nullptr;
    HIPCHK(hipMalloc((void **)&di, sizeof(double) * (size_t)n));
    HIPCHK(hipMalloc((void **)&di2, sizeof(double) * (size_t)n));
    HIPCHK(hipMalloc((void **)&dout, sizeof(double) * (size_t)n));
    HIPCHK(hipMemcpy(di, in, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(di2, in2 ? in2 : in, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(selftest_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, (const double *)di,
                       (const double *)di2, dout, (long long)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    (void)hipFree(di); (void)hipFree(di2); (void)hipFree(dout);
    return PTMI_OK;
}

int ptmi_selftest_philox(int device, const uint32_t *ck, uint32_t *out, int64_t n)
{
    if (!ck || !out || n < 0) return fail(PTMI_EINVAL, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(PTMI_ENODEVICE, "no HIP device visible");
    HIPCHK(hipSetDevice(device));
    u32 *dc = nullptr, *dout = nullptr;
    HIPCHK(hipMalloc((void **)&dc, sizeof(u32) * 6 * (size_t)n));
    HIPCHK(hipMalloc((void **)&dout, sizeof(u32) * 4 * (size_t)n));
    HIPCHK(hipMemcpy(dc, ck, sizeof(u32) * 6 * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(selftest_philox_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const u32 *)dc, dout, (long long)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dout, sizeof(u32) * 4 * (size_t)n, hipMemcpyDeviceToHost));
    (void)hipFree(dc); (void)hipFree(dout);
    return PTMI_OK;
}

int ptmi_malloc(void **p, size_t bytes)
{
    if (!p) return fail(PTMI_EINVAL, "NULL argument");
    HIPCHK(hipMalloc(p, bytes));
    return PTMI_OK;
}
int ptmi_free(void *p) { HIPCHK(hipFree(p)); return PTMI_OK; }
int ptmi_memcpy_h2d(void *dst, const void *src, size_t bytes) { HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return PTMI_OK; }
int ptmi_memcpy_d2h(void *dst, const void *src, size_t bytes) { HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return PTMI_OK; }
int ptmi_memset(void *dst, int value, size_t bytes) { HIPCHK(hipMemset(dst, value, bytes)); return PTMI_OK; }

int ptmi_timer_start(ptmi_handle h)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    return PTMI_OK;
}
int ptmi_timer_stop_ms(ptmi_handle h, double *ms)
{
    if (!h || !ms) return fail(PTMI_EINVAL, "NULL argument");
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev1));
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, h->ev0, h->ev1));
    *ms = (double)f;
    return PTMI_OK;
}

#ifdef PTMI_UNIT_STAMPS
// diagnostic build (tools/unit_stamps.py): the stamps of the last persistent SCAM launch, copied to the host
int ptmi_unit_stamps(void *dst, size_t bytes)
{
    const size_t all = sizeof(u64) * (size_t)PTMI_STAMP_WAVE * PTMI_STAMP_WAVES;
    if (!dst || bytes > all) return fail(PTMI_EINVAL, "at most %zu bytes of stamps", all);
    u64 *buf = ptmi_stamp_buffer();
    if (!buf) return fail(PTMI_EHIP, "no stamp buffer");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(dst, buf, bytes, hipMemcpyDeviceToHost));
    return PTMI_OK;
}
#endif

}  // extern "C"

#ifdef PTMI_UNIT_STAMPS
u64 *ptmi_stamp_buffer()
{
    static u64 *buf = nullptr;
    const size_t all = sizeof(u64) * (size_t)PTMI_STAMP_WAVE * PTMI_STAMP_WAVES;
    if (!buf && (hipMalloc((void **)&buf, all) != hipSuccess || hipMemset(buf, 0, all) != hipSuccess)) buf = nullptr;
    return buf;
}
#endif
