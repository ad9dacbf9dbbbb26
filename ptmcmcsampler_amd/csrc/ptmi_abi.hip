// ptmi_abi.hip -- the C ABI of libptmi.so, the engine object, and the kernels of the statistics (Welford / pooling), the AM
// producers, the DE ring, the gradient-jump launch order and the self-tests.  See include/ptmi.h for the boundary and DESIGN.md.
#include <math.h>
#include <stdlib.h>

#include <new>
#include <vector>

#include <type_traits>

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

// ------------------------------------------------------------------ Welford
// PT:769-794.  Block (walker, tile_i, tile_j) keeps a 112x112 tile of M2 in registers
// (7x7 per thread, 16x16 threads) and streams the `mem` buffered rows; the running mean
// of the tile's i- and j-slices is recomputed by the first 2x112 threads and handed to
// the tile through LDS.  Every element sees exactly the reference's operation order:
// M2[i][j] += diff[i] * (row[j] - mu_new[j]), one product and one sum, rows ascending.
constexpr int WT = 7, WTILE = 16 * WT;
template <bool FUSED>
__global__ __launch_bounds__(256) void welford_kernel(const double *AM, double *mu, double *M2, double *cov, int d, int mem,
                                                     long long iter, int cov_stride_per_walker, int am_epl)
{
    constexpr int PF = 8;       // rows fetched ahead by the carrier threads (one HBM latency per PF rows)
    constexpr int RB = 4;       // rows handed to the tile per barrier
    __shared__ double sh[2][RB][2][WTILE];  // [buf][row][diff|e][WTILE]
    if (FUSED && blockIdx.y > blockIdx.x) return;       // pooled definition: the lower triangle is mirrored afterwards
    const int w = (int)blockIdx.z;
    const int ti0 = (int)blockIdx.y * WTILE, tj0 = (int)blockIdx.x * WTILE;
    const int tx = (int)(threadIdx.x & 15), ty = (int)(threadIdx.x >> 4);
    const double *am = AM + (size_t)w * mem * d;
    double *muw = mu + (size_t)w * d, *M2w = M2 + (size_t)w * d * d;
    long long it = iter - mem;
    const bool reset = it == 0;

    // threads 0..111 carry mu of the i-slice, 112..223 of the j-slice
    const int role = (int)threadIdx.x / WTILE, ridx = (int)threadIdx.x % WTILE;
    const int rel = role == 0 ? ti0 + ridx : tj0 + ridx;
    const bool carrier = role < 2 && rel < d;
    double m = carrier && !reset ? muw[rel] : 0.0;

    double acc[WT][WT];
#pragma unroll
    for (int p = 0; p < WT; ++p)
#pragma unroll
        for (int r = 0; r < WT; ++r) {
            const int i = ti0 + ty + 16 * p, j = tj0 + tx + 16 * r;
            acc[p][r] = (!reset && i < d && j < d) ? M2w[(size_t)i * d + j] : 0.0;
        }
    int bsel = 0;
    for (int ii0 = 0; ii0 < mem; ii0 += PF) {
        double vpre[PF];
#pragma unroll
        for (int u = 0; u < PF; ++u) vpre[u] = (carrier && ii0 + u < mem) ? am[(size_t)(ii0 + u) * d + am_pos(rel < d ? rel : 0, am_epl)] : 0.0;
#pragma unroll
        for (int u0 = 0; u0 < PF; u0 += RB) {
            if (ii0 + u0 >= mem) break;
            // the carriers advance the running mean through RB rows (the recurrence is theirs alone) ...
            if (role < 2) {
#pragma unroll
                for (int u = 0; u < RB; ++u) {
                    double df = 0.0, ev = 0.0;
                    if (carrier && ii0 + u0 + u < mem) {
                        const double v = vpre[u0 + u];
                        df = v - m;
                        if (FUSED) m = m + df * (1.0 / (double)(it + 1 + u));
                        else m += df / (double)(it + 1 + u);
                        ev = v - m;
                    }
                    if (role == 0) sh[bsel][u][0][ridx] = df;
                    else sh[bsel][u][1][ridx] = ev;
                }
            }
            __syncthreads();
            // ... and the whole tile applies the RB rank-1 updates, rows ascending (rows past the end carry zeros)
#pragma unroll
            for (int u = 0; u < RB; ++u) {
                double dv[WT], evv[WT];
#pragma unroll
                for (int p = 0; p < WT; ++p) dv[p] = sh[bsel][u][0][ty + 16 * p];
#pragma unroll
                for (int r = 0; r < WT; ++r) evv[r] = sh[bsel][u][1][tx + 16 * r];
                if (ii0 + u0 + u < mem) {
#pragma unroll
                    for (int p = 0; p < WT; ++p)
#pragma unroll
                        for (int r = 0; r < WT; ++r) {
                            if (FUSED) acc[p][r] = __builtin_fma(dv[p], evv[r], acc[p][r]);   // pooled mode: not a reference replica
                            else acc[p][r] += dv[p] * evv[r];                                 // PT:792, one product and one sum
                        }
                }
            }
            const int done = mem - (ii0 + u0) < RB ? mem - (ii0 + u0) : RB;
            it += done;
            bsel ^= 1;
        }
    }
    const double den = (double)(it - 1);
    double *covw = cov ? cov + (size_t)w * cov_stride_per_walker : nullptr;
#pragma unroll
    for (int p = 0; p < WT; ++p)
#pragma unroll
        for (int r = 0; r < WT; ++r) {
            const int i = ti0 + ty + 16 * p, j = tj0 + tx + 16 * r;
            if (i < d && j < d) {
                M2w[(size_t)i * d + j] = acc[p][r];
                if (covw) covw[(size_t)i * d + j] = acc[p][r] / den;
            }
        }
    // Several tiles per walker: mu is advanced by welford_mean_kernel, launched after this one (every tile needs
    // the old mean).  One tile: this block's carriers hold the new mean already.
    if (gridDim.x == 1 && role == 0 && carrier) muw[rel] = m;
}

// One tile per walker (d <= TYN * PR, the per-walker replica mode at ndim <= 100): the same recurrence with the work split by waves.
// welford_kernel's carriers are threads of the tile's own four waves, so every wave pays for the mean's division (a dozen
// instructions beside the 98 of a row) and a quarter of its 7 x 7 accumulators lie outside a 100 x 100 matrix: 5.1 ms per epoch at
// 4096 x 1000 x 100 against 2.1 ms of products and sums.  Here threads 0 .. TYN TXN - 1 hold PR x PC accumulators each (25 x 10
// threads of 4 x 10: no padding at d = 100, the row's factors read from LDS as 16-byte pieces), and two more waves carry the mean:
// thread 256 + i advances mu[i] through the rows one batch AHEAD of the tile (double-buffered in LDS, one barrier per RB rows).
// The division df / n (n = the row count, the same for every lane) is Markstein's: r = 1 / n by a true division once per batch
// and lane, then q = df r corrected twice through the exact remainder fma(-n, q, df) -- the correctly rounded quotient (r is the
// correctly rounded reciprocal of an integer below 2^53; 4e8 random and near-tie cases against a / n: tests/test_welford_div.py
// runs the same arithmetic on the host).
__device__ __forceinline__ double div_by_count(double a, double n, double r)
{
    if (__builtin_fabs(a) < 0x1p-900) return a / n;         // a remainder in the subnormal range would not be exact
    double q = a * r;
    double e = __builtin_fma(-n, q, a);
    q = __builtin_fma(e, r, q);
    e = __builtin_fma(-n, q, a);
    return __builtin_fma(e, r, q);
}
template <int TYN, int TXN, int PR, int PC>
__global__ __launch_bounds__(768) void welford_rows_kernel(const double *AM, double *mu, double *M2, double *cov, int d, int mem, long long iter,
                                                           int cov_stride_per_walker, int am_epl, int nwalkers)
{
    // a block = TWO walkers: 2 x 4 tile waves + 2 x 2 carrier waves = three waves on every SIMD (up to 170 registers each); a block
    // of one walker's six waves lands 2 + 2 + 1 + 1 on the SIMDs and a second block no longer fits beside it
#ifndef PTMI_WF_RB
#define PTMI_WF_RB 8
#endif
    constexpr int RB = PTMI_WF_RB, LW = TYN * PR > TXN * PC ? TYN * PR : TXN * PC;
    __shared__ __attribute__((aligned(16))) double sh_all[2][2][RB][2][LW];      // [walker of the block][buffer][row][diff | e][element]
    const int tb = (int)threadIdx.x;
    const int slot = tb < 512 ? tb >> 8 : (tb - 512) >> 7;
    const int w = 2 * (int)blockIdx.x + slot;
    const bool wact = w < nwalkers;
    double (*sh)[RB][2][LW] = sh_all[slot];
    const double *am = AM + (size_t)(wact ? w : 0) * mem * d;
    double *muw = mu + (size_t)(wact ? w : 0) * d, *M2w = M2 + (size_t)(wact ? w : 0) * d * d;
    const long long it0 = iter - mem;
    const bool reset = it0 == 0;
    const int t = tb < 512 ? (tb & 255) : 256 + ((tb - 512) & 127);      // 0 .. 255 the tile, 256 .. 383 the carriers of this walker
    const int nb = (mem + RB - 1) / RB;
    if (t >= 256) {
        // ------------------------------------------------ the mean's carriers
        const int rel = t - 256;
        const bool carrier = rel < d && wact;
        const int pos = am_pos(carrier ? rel : 0, am_epl);
        double m = carrier && !reset ? muw[rel] : 0.0;
        double vc[RB], vn[RB];
        auto load = [&](int b, double (&v)[RB]) {
#pragma unroll
            for (int u = 0; u < RB; ++u) {
                const int row = b * RB + u;
                v[u] = (carrier && row < mem) ? am[(size_t)row * d + pos] : 0.0;
            }
        };
        auto produce = [&](int b, const double (&v)[RB]) {
            const double nl = (double)(it0 + (long long)b * RB + 1 + (t & (RB - 1))), rl = 1.0 / nl;      // lane u of every RB: row u's count
#pragma unroll
            for (int u = 0; u < RB; ++u) {
                const double n = __shfl(nl, u, RB), r = __shfl(rl, u, RB);
                double df = 0.0, ev = 0.0;
#ifdef PTMI_WF_NOCARRY
                df = v[u] + n; ev = v[u] + r;
#else
                if (b * RB + u < mem) {
                    df = v[u] - m;
                    m += div_by_count(df, n, r);            // PT:787 (mean += diff / n)
                    ev = v[u] - m;
                }
#endif
                if (rel < LW) { sh[b & 1][u][0][rel] = carrier ? df : 0.0; sh[b & 1][u][1][rel] = carrier ? ev : 0.0; }
            }
        };
        load(0, vc);
        if (nb > 1) load(1, vn);
        produce(0, vc);
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
            if (b + 1 < nb) {
#pragma unroll
                for (int u = 0; u < RB; ++u) vc[u] = vn[u];
                if (b + 2 < nb) load(b + 2, vn);
                produce(b + 1, vc);
            }
            __syncthreads();
        }
        if (carrier && wact) muw[rel] = m;
        return;
    }
    // ---------------------------------------------------- the tile
    const int ty = t / TXN, tx = t % TXN;
    const bool live = t < TYN * TXN && wact;
    double acc[PR][PC];
#pragma unroll
    for (int p = 0; p < PR; ++p)
#pragma unroll
        for (int r = 0; r < PC; ++r) {
            const int i = ty * PR + p, j = tx * PC + r;
            acc[p][r] = (live && !reset && i < d && j < d) ? M2w[(size_t)i * d + j] : 0.0;
        }
    __syncthreads();
    for (int b = 0; b < nb; ++b) {
        if (live) {
            // the next row's factors are requested before this row's products (two register sets): an LDS round trip per row is
            // not covered by the one or two other waves of the SIMD
            double dv[2][PR], ev[2][PC];
            auto rd = [&](int u, int k) {
#pragma unroll
                for (int p = 0; p < PR; ++p) dv[k][p] = sh[b & 1][u][0][ty * PR + p];
#pragma unroll
                for (int r = 0; r < PC; ++r) ev[k][r] = sh[b & 1][u][1][tx * PC + r];
            };
            // PT:792, one product and one sum per element, rows ascending (fencing a row's products off from their sums cost 37
            // spilled registers and 2 ms).  Rows past the end of the buffer carry zeros from the carriers (acc + 0 * 0: an accumulator
            // is never -0), so the batch is straight-line code.
            auto row = [&](int k) {
#pragma unroll
                for (int p = 0; p < PR; ++p)
#pragma unroll
                    for (int r = 0; r < PC; ++r) acc[p][r] += dv[k][p] * ev[k][r];
            };
            rd(0, 0);
#pragma unroll
            for (int u = 0; u < RB; ++u) {
                if (u + 1 < RB) {
                    rd(u + 1, (u + 1) & 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
                row(u & 1);
            }
        }
        __syncthreads();
    }
    if (!live) return;
    const double den = (double)(iter - 1);
    double *covw = cov ? cov + (size_t)w * cov_stride_per_walker : nullptr;
#pragma unroll
    for (int p = 0; p < PR; ++p)
#pragma unroll
        for (int r = 0; r < PC; ++r) {
            const int i = ty * PR + p, j = tx * PC + r;
            if (i < d && j < d) M2w[(size_t)i * d + j] = acc[p][r];
        }
    // the covariance in a rolled loop over the thread's own elements, read back (forty unrolled divisions beside the accumulators
    // cost the main loop 44 spilled registers)
    if (covw) {
#pragma unroll 1
        for (int e = 0; e < PR * PC; ++e) {
            const int i = ty * PR + e / PC, j = tx * PC + e % PC;
            if (i < d && j < d) covw[(size_t)i * d + j] = M2w[(size_t)i * d + j] / den;
        }
    }
}

// ---------------------------------------------------------------- pooled covariance
// cov_mode "pooled" (one covariance adapted from all walkers' rank-0 samples; oracle: orc_pool_update).  The epoch's chunk
// -- the W x cov_update buffered rows as one [rows][d] matrix -- enters as shifted sums T = sum dx dx^T, t = sum dx with
// dx = x - (the running pooled mean): a symmetric rank-k update with no recurrence in it, so the rows go straight from
// memory through LDS into v_mfma_f64_16x16x4_f64, whose k-ascending fma chain is the oracle's row-ascending definition.
// The column sums come out of the same instructions: column d of dx is the constant 1.
// Grid: (macro tile, slab): the tiles of a slab are neighbours in launch order, so that its rows, wanted by every one of them, are
// read from memory once and from the caches after that.  A slab is a contiguous run of rows (pool_slab walkers); a macro tile is 112 x 112 outputs
// (7 x 7 matrix tiles) of the columns [112 I, 112 I + 112) x [112 J, 112 J + 112), I <= J.  DIAG (I == J): the 28 tiles with
// ti <= tj, seven per wave; else all 49, 13 / 12 / 12 / 12.  Rows are staged 32 at a time (eight k-steps) in a double-buffered LDS
// chunk, the next chunk's global loads in flight during the matrix work; one barrier per chunk.  Each block writes its
// slab's partial sums; pool_reduce_kernel adds the slabs in order, pool_finish_kernel applies Chan's formula.
// Round 2 ran a per-walker Welford recurrence on the matrix cores (1.45 ms per epoch at 4096 x 1000 x 100, two carrier waves
// feeding the recurrence) + a 328 MB two-level combination (0.12 ms); d > 112 had no matrix-core path at all (26 ms at d = 1000).
constexpr int PS_W = 112;       // columns of a macro tile
// rows per staged chunk: 32 (8 k-steps x 7 tiles) on the diagonal, 16 (4 k-steps x 13 tiles) off it: some 55 matrix instructions
// per wave cover a memory round trip, and two blocks share a CU (57 KB of LDS each)
constexpr int ps_rc(bool diag) { return diag ? 32 : 16; }
typedef double ps_d4 __attribute__((ext_vector_type(4)));
__host__ __device__ inline int pool_groups(int d) { return (d + 1 + PS_W - 1) / PS_W; }          // macro tiles per side (columns 0 .. d)
// walkers per slab: up to 512 slabs when one macro tile covers the matrix, up to 32 beyond (a partial is d (d + 1) doubles);
// part of the definition (summation order): oracle/oracle.py pool_slab is the same rule
static inline int pool_slab(int nwalkers, int d) { const int target = d + 1 <= PS_W ? 512 : 32; const int s = (nwalkers + target - 1) / target; return s < 1 ? 1 : s; }
// RLE (AM row flags, ptmi_common.h): a slab's matrix is not its rows but its STORED rows, each scaled by the square root of the
// length of its run (pool_rle_kernel lists them: PoolEnt = the row inside the slab and sqrt(run length)): sum over runs of n dx dx^T
// as (sqrt(n) dx) (sqrt(n) dx)^T, column d of the staged matrix holding sqrt(n) so that the column sums come out as sum n dx.
// The oracle defines the same sums (orc_pool_update_rle): 43 % fewer rows to read, stage and multiply at the stationary
// acceptance of a SCAM cycle.  A stager needs the list entry before it can ask for the row: the entries of chunk i + 2 are
// requested while the rows of chunk i + 1 are in flight and chunk i is multiplied.
// Round 4, second form (the first took 1.22 ms per epoch at 4096 x 1000 x 100 against 0.42 ms of matrix instructions: 350 vector
// instructions of 64-bit index arithmetic and selects per wave and chunk beside the 56 matrix ones, which the f64 matrix pipe does
// not overlap): the macro tile lives in POSITION space -- column p of the staged matrix is position p of a buffered row, whatever
// parameter am_pos put there; an element's k-ascending fma chain does not care where its column sits, the epilogue maps the
// pair back with am_inv -- so a stager takes 16 bytes of a row per load (PAIR: d even) at a 32-bit offset from the slab's base;
// a dead row is a zero weight, not a select per element; the waves' tiles are compile-time lists (row-major runs: a wave's
// fragments are read from LDS once per k-step on the diagonal, 7 instead of 14).
struct PoolEnt { double wgt; int32_t src; int32_t pad; };
struct PoolRle { const PoolEnt *ent; const int32_t *cnt; };
typedef double ps_d2 __attribute__((ext_vector_type(2)));
// tiles of wave wv: on the diagonal tile rows wv and 7 - wv (7 tiles each wave), off it the row-major run [1 + 12 wv, ...) of the 49
constexpr int ps_nt(bool diag, int wv) { return diag ? 7 : (wv == 0 ? 13 : 12); }
__host__ __device__ constexpr int ps_t0(int wv) { return wv == 0 ? 0 : 1 + 12 * wv; }
constexpr int ps_ti(bool diag, int wv, int n) { return diag ? (n < 7 - wv ? wv : 7 - wv) : (ps_t0(wv) + n) / 7; }
constexpr int ps_tj(bool diag, int wv, int n) { return diag ? (n < 7 - wv ? wv + n : n) : (ps_t0(wv) + n) % 7; }
template <bool DIAG, int WV>
__device__ __forceinline__ void ps_mma(const double *Ab, const double *Bb, ps_d4 (&acc)[DIAG ? 7 : 13])
{
#pragma unroll
    for (int k0 = 0; k0 < ps_rc(DIAG); k0 += 4)
#pragma unroll
        for (int n = 0; n < ps_nt(DIAG, WV); ++n)
            acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(Ab[k0 * PS_W + 16 * ps_ti(DIAG, WV, n)], Bb[k0 * PS_W + 16 * ps_tj(DIAG, WV, n)], acc[n], 0, 0, 0);
}
template <bool DIAG, int WV>
__device__ __forceinline__ void ps_store(const ps_d4 (&acc)[DIAG ? 7 : 13], double *out, int I, int J, int d, int am_epl, int g, int c)
{
#pragma unroll
    for (int n = 0; n < ps_nt(DIAG, WV); ++n) {
        const int ti = ps_ti(DIAG, WV, n), tj = ps_tj(DIAG, WV, n);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int pi = I * PS_W + 16 * ti + g + 4 * r, pj = J * PS_W + 16 * tj + c;
            if (pi < d && pj <= d && (!(DIAG && ti == tj) || pi <= pj)) {
                const int ci = am_inv(pi, am_epl), cj = pj < d ? am_inv(pj, am_epl) : d;
                const int lo = ci < cj ? ci : cj, hi = ci < cj ? cj : ci;
                out[(size_t)lo * (d + 1) + hi] = acc[n][r];
            }
        }
    }
}
template <bool DIAG, bool RLE, bool PAIR>
__global__ __launch_bounds__(256, 2) void pool_syrk_kernel(const double *rows, long long nrows, int d, const double *shift,
                                                                     long long rows_per_slab, double *part, int am_epl,
                                                                     int shift_epl /* row format of `shift` (an AM row at the first epoch) */,
                                                                     PoolRle rl)
{
    constexpr int NTW = DIAG ? 7 : 13, NA = DIAG ? 1 : 2, PS_RC = ps_rc(DIAG), NU = PS_RC / 4;
    __shared__ double Dl[NA][2][PS_RC][PS_W];
    const int lane = (int)(threadIdx.x & 63), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c = lane & 15, g = lane >> 4;
    const int ng = pool_groups(d);
    int I = (int)blockIdx.x, J = (int)blockIdx.x;
    if (!DIAG) {                                            // blockIdx.x enumerates the pairs I < J row by row
        int p = (int)blockIdx.x;
        I = 0;
        while (p >= ng - 1 - I) { p -= ng - 1 - I; ++I; }
        J = I + 1 + p;
    }
    const long long beg = (long long)blockIdx.y * rows_per_slab;
    // the loop runs over the slab's LIST: RLE its stored rows (entries 0 .. count - 1 of ent), else its rows
    const int nlist = RLE ? rl.cnt[blockIdx.y] : (int)(beg + rows_per_slab < nrows ? rows_per_slab : nrows - beg);
    const char *slab = (const char *)(rows + beg * d);      // byte offsets inside a slab fit 32 bits (checked by the host)
    const PoolEnt *ent = RLE ? rl.ent + beg : nullptr;
    ps_d4 acc[NTW];
#pragma unroll
    for (int n = 0; n < NTW; ++n) acc[n] = ps_d4{0.0, 0.0, 0.0, 0.0};
    // off the diagonal a wave's tiles are the run [ps_t0(wave), ...) of the 49, their fragments' offsets in scalar registers (four
    // compile-time copies of 13 accumulators' code spilled 93 registers)
    int offa[DIAG ? 1 : NTW], offb[DIAG ? 1 : NTW];
    if constexpr (!DIAG) {
#pragma unroll
        for (int n = 0; n < NTW; ++n) {
            const int t = ps_t0(wave) + n < 49 ? ps_t0(wave) + n : 48;
            offa[n] = __builtin_amdgcn_readfirstlane(16 * (t / 7));
            offb[n] = __builtin_amdgcn_readfirstlane(16 * (t % 7));
        }
    }
    // staging: a wave's lanes 16 r4 + (q & 15) own the position pair (2 q, 2 q + 1) of the macro tile(s) and rows r4, r4 + 4, ... of a
    // chunk: a load instruction takes 256 contiguous bytes of four rows, an LDS store fills all the banks
    const int q = 16 * wave + c, r4 = g;
    const bool stager = q < PS_W / 2;
    unsigned colb[NA][2];           // byte offset of the elements' positions inside a row (clamped into it)
    double sh[NA][2], one[NA][2];
    bool dat[NA][2];
    bool plain = true;
#pragma unroll
    for (int a2 = 0; a2 < NA; ++a2)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int p = (a2 == 0 ? I : J) * PS_W + 2 * q + e;
            dat[a2][e] = p < d;
            const int pc = PAIR ? (p - e < d ? p : d - 2 + e) : (p < d ? p : d - 1);
            colb[a2][e] = 8u * (unsigned)pc;
            sh[a2][e] = (stager && p < d) ? shift[am_pos(am_inv(p, am_epl), shift_epl)] : 0.0;
            one[a2][e] = p == d ? 1.0 : 0.0;
            plain = plain && (dat[a2][e] || !stager);
        }
    const bool wave_plain = __all(plain);                   // no ones / padding column among this wave's stagers: no selects at all
    const unsigned rstride = 8u * (unsigned)d;
    // Loads are unconditional (list index and column clamped: a branch per load made every one of them wait for its own round
    // trip, 2.6 ms per epoch); what a slot really holds is decided when it is staged.
    ps_d2 v[NA][NU];
    double wg[NU];                 // weight of the rows in v: sqrt(run length) (RLE) or 1, zero past the end of the list
    int nsrc[RLE ? NU : 1];        // RLE: rows and weights of the chunk after the one in v
    double nwg[RLE ? NU : 1];
    auto list = [&](int j0) {      // RLE: request the list entries of the chunk that starts at entry j0
        if constexpr (RLE) {
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int j = j0 + 4 * u + r4, jc = j < nlist ? j : nlist - 1;
                const ps_d2 e2 = *(const ps_d2 *)(ent + jc);
                nwg[u] = e2.x;
                nsrc[u] = (int)(__double_as_longlong(e2.y) & 0xffffffffll);
            }
        }
    };
    auto fetch = [&](int j0) {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int j = j0 + 4 * u + r4, jc = j < nlist ? j : nlist - 1;
            const unsigned rb = (unsigned)(RLE ? nsrc[u] : jc) * rstride;
            wg[u] = j < nlist ? (RLE ? nwg[u] : 1.0) : 0.0;
#pragma unroll
            for (int a2 = 0; a2 < NA; ++a2) {
                if constexpr (PAIR) v[a2][u] = *(const ps_d2 *)(slab + (rb + colb[a2][0]));
                else {
                    v[a2][u].x = *(const double *)(slab + (rb + colb[a2][0]));
                    v[a2][u].y = *(const double *)(slab + (rb + colb[a2][1]));
                }
            }
        }
    };
    auto stage = [&](int buf) {
        if (!stager) return;
        if (wave_plain) {
#pragma unroll
            for (int a2 = 0; a2 < NA; ++a2)
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    ps_d2 x;
                    x.x = (v[a2][u].x - sh[a2][0]) * wg[u];
                    x.y = (v[a2][u].y - sh[a2][1]) * wg[u];
                    *(ps_d2 *)&Dl[a2][buf][4 * u + r4][2 * q] = x;
                }
        } else {
#pragma unroll
            for (int a2 = 0; a2 < NA; ++a2)
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    ps_d2 x;
                    x.x = (dat[a2][0] ? v[a2][u].x - sh[a2][0] : one[a2][0]) * wg[u];
                    x.y = (dat[a2][1] ? v[a2][u].y - sh[a2][1] : one[a2][1]) * wg[u];
                    *(ps_d2 *)&Dl[a2][buf][4 * u + r4][2 * q] = x;
                }
        }
    };
    if (nlist > 0) {
        list(0);
        fetch(0);
        list(PS_RC);
        stage(0);
    }
    __syncthreads();
    int buf = 0;
    for (int j0 = 0; j0 < nlist; j0 += PS_RC) {
        const bool more = j0 + PS_RC < nlist;
        if (more) {
            fetch(j0 + PS_RC);
            list(j0 + 2 * PS_RC);
        }
        const double *Ab = &Dl[0][buf][0][0] + g * PS_W + c, *Bb = &Dl[NA - 1][buf][0][0] + g * PS_W + c;
        if constexpr (DIAG) {
            switch (wave) {
            case 0: ps_mma<DIAG, 0>(Ab, Bb, acc); break;
            case 1: ps_mma<DIAG, 1>(Ab, Bb, acc); break;
            case 2: ps_mma<DIAG, 2>(Ab, Bb, acc); break;
            default: ps_mma<DIAG, 3>(Ab, Bb, acc); break;
            }
        } else {
#pragma unroll
            for (int k0 = 0; k0 < PS_RC; k0 += 4)
#pragma unroll
                for (int n = 0; n < NTW; ++n)
                    if (n < 12 || wave == 0) acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(Ab[k0 * PS_W + offa[n]], Bb[k0 * PS_W + offb[n]], acc[n], 0, 0, 0);
        }
        if (more) stage(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    double *out = part + (size_t)blockIdx.y * d * (d + 1);
    if constexpr (DIAG) {
        switch (wave) {
        case 0: ps_store<DIAG, 0>(acc, out, I, J, d, am_epl, g, c); break;
        case 1: ps_store<DIAG, 1>(acc, out, I, J, d, am_epl, g, c); break;
        case 2: ps_store<DIAG, 2>(acc, out, I, J, d, am_epl, g, c); break;
        default: ps_store<DIAG, 3>(acc, out, I, J, d, am_epl, g, c); break;
        }
    } else {
#pragma unroll
        for (int n = 0; n < NTW; ++n) {
            if (!(n < 12 || wave == 0)) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int pi = I * PS_W + offa[n] + g + 4 * r, pj = J * PS_W + offb[n] + c;
                if (pi < d && pj <= d) {
                    const int ci = am_inv(pi, am_epl), cj = pj < d ? am_inv(pj, am_epl) : d;
                    const int lo = ci < cj ? ci : cj, hi = ci < cj ? cj : ci;
                    out[(size_t)lo * (d + 1) + hi] = acc[n][r];
                }
            }
        }
    }
}

// The list of a slab's stored rows (AM row flags) and the square roots of their run lengths: entry j of slab s (at beg + j) is the
// j-th row of the slab whose flag word says NEW or KEY; its run ends where the next stored row begins (ring row 0 of every walker is
// a KEY row, so a run never crosses into another walker's ring) or at the slab's end.  One block per slab, rows in order.
__global__ __launch_bounds__(256) void pool_rle_kernel(const AmFlag *flag, long long nrows, long long rows_per_slab, PoolEnt *ent, int32_t *cnt)
{
    // eight groups of 256 rows per trip: the flags of a trip are requested together and its ballots share two barriers (a load,
    // a ballot and three barriers per 256 rows made the kernel the latency of 31 round trips: 59 us per epoch at 4096 x 1000)
    constexpr int NG = 8;
    __shared__ int wsum[NG][4], base_s;
    const long long beg = (long long)blockIdx.x * rows_per_slab;
    const long long end = beg + rows_per_slab < nrows ? beg + rows_per_slab : nrows;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    if (threadIdx.x == 0) base_s = 0;
    __syncthreads();
    for (long long r0 = beg; r0 < end; r0 += 256 * NG) {
        AmFlag f[NG];
#pragma unroll
        for (int u = 0; u < NG; ++u) { const long long r = r0 + 256 * u + threadIdx.x; f[u] = flag[r < end ? r : end - 1]; }
        unsigned long long m[NG];
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const long long r = r0 + 256 * u + threadIdx.x;
            m[u] = __ballot(r < end && (f[u] & (AMROW_NEW | AMROW_KEY)) != 0);
            if (lane == 0) wsum[u][wave] = (int)__popcll(m[u]);
        }
        __syncthreads();
        int off = base_s;
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const long long r = r0 + 256 * u + threadIdx.x;
            int mine = off + (int)__popcll(m[u] & ((1ull << lane) - 1ull));
            for (int k = 0; k < wave; ++k) mine += wsum[u][k];
            if ((m[u] >> lane) & 1ull) ent[beg + mine].src = (int32_t)(r - beg);
            off += wsum[u][0] + wsum[u][1] + wsum[u][2] + wsum[u][3];
        }
        __syncthreads();
        if (threadIdx.x == 0) base_s = off;
        __syncthreads();
    }
    const int n = base_s;
    if (threadIdx.x == 0) cnt[blockIdx.x] = n;
    for (int j0 = 0; j0 < n; j0 += 256 * NG) {
        int here[NG], next[NG];
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const int j = j0 + 256 * u + (int)threadIdx.x, jc = j < n ? j : n - 1;
            here[u] = ent[beg + jc].src;
            next[u] = jc + 1 < n ? ent[beg + jc + 1].src : (int)(end - beg);
        }
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const int j = j0 + 256 * u + (int)threadIdx.x;
            if (j < n) ent[beg + j].wgt = det_sqrt((double)((long long)next[u] - (long long)here[u]));
        }
    }
}

// AM row flags -> every row: rows that were not stored (rejected steps) are copied forward from the row before them, in place,
// for the readers that want every row (DE history, chain files, the ESS window, tests): iterations it_lo .. it_hi of walkers
// w0 .. w0 + nw - 1.  Both iterations lie in the current covariance period [base, base + cu], base = the last multiple of cov_update
// below it_hi (ring row 0): once the ring wraps, the stored row an older repeat hangs on is overwritten (the statistics read a period
// when it is complete; nothing reads further back).  One block per walker, a thread per parameter, rows in time order.
__global__ __launch_bounds__(128) void am_expand_kernel(double *AM, const AmFlag *flag, int d, int cu, int w0, long long it_lo, long long it_hi,
                                                        long long base)
{
    const int w = w0 + (int)blockIdx.x;
    const AmFlag *fw = flag + (size_t)w * cu;
    double *aw = AM + (size_t)w * cu * d;
    long long it0 = it_lo;                                   // the stored row to start from (uniform)
    while (it0 > base && !(fw[it0 % cu] & (AMROW_NEW | AMROW_KEY))) --it0;
    for (int i = (int)threadIdx.x; i < d; i += (int)blockDim.x) {       // element i of the buffer's row format, whatever it is
        double x = aw[(size_t)(it0 % cu) * d + i];
        for (long long it = it0 + 1; it <= it_hi; ++it) {
            const int ring = (int)(it % cu);
            if (fw[ring] & (AMROW_NEW | AMROW_KEY)) x = aw[(size_t)ring * d + i];
            else if (it >= it_lo) aw[(size_t)ring * d + i] = x;
        }
    }
}
// sum of the slabs' partials, slabs ascending (plain sums): Tsum[i][j], j in [i, d]; column d holds t
__global__ void pool_reduce_kernel(const double *part, int nslab, int d, double *Tsum)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int ld = d + 1;
    if (idx >= (long long)d * ld) return;
    const int i = (int)(idx / ld), j = (int)(idx % ld);
    if (j < i) return;
    // 32 slabs' values requested at once (the sums stay in slab order): ten thousand threads walk 512 partials each, the kernel is
    // the latency of its loads
    const size_t st = (size_t)d * ld;
    double sum = 0.0;
    int s = 0;
    for (; s + 32 <= nslab; s += 32) {
        double v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) v[u] = part[(size_t)(s + u) * st + idx];
#pragma unroll
        for (int u = 0; u < 32; ++u) sum += v[u];
    }
    for (; s + 8 <= nslab; s += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(s + u) * st + idx];
#pragma unroll
        for (int u = 0; u < 8; ++u) sum += v[u];
    }
    for (; s < nslab; ++s) sum += part[(size_t)s * st + idx];
    Tsum[idx] = sum;
}
// Chan's combination of the chunk (nb samples, sums about the shift) with the running pooled statistics (nprev samples)
__global__ void pool_finish_kernel(const double *Tsum, const double *shift, int shift_epl, double *mu, double *M2, double *cov, int d, int first,
                                   double nb, double f /* nprev nb / (nprev + nb) */, double gw /* nb / (nprev + nb) */, double den)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)d * d) return;
    const int i = (int)(idx / d), j = (int)(idx % d), ld = d + 1;
    if (j < i) return;
    const double ti = Tsum[(size_t)i * ld + d], tj = Tsum[(size_t)j * ld + d];
    const double M2b = Tsum[(size_t)i * ld + j] - (ti * tj) / nb;
    double m;
    if (first) m = M2b;
    else m = (M2[idx] + M2b) + ((ti / nb) * (tj / nb)) * f;
    M2[idx] = m;
    M2[(size_t)j * d + i] = m;
    const double cv = m / den;
    cov[idx] = cv;
    cov[(size_t)j * d + i] = cv;
    if (i == j) mu[i] = first ? shift[am_pos(i, shift_epl)] + ti / nb : mu[i] + (ti / nb) * gw;
}

__global__ void welford_mean_kernel(const double *AM, double *mu, int d, int mem, long long iter, int fused, int am_epl)
{
    const int w = (int)blockIdx.y;
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= d) return;
    const double *am = AM + (size_t)w * mem * d;
    long long it = iter - mem;
    double m = it == 0 ? 0.0 : mu[(size_t)w * d + j];
    for (int ii = 0; ii < mem; ++ii) {
        it += 1;
        const double df = am[(size_t)ii * d + am_pos(j, am_epl)] - m;
        if (fused) m = m + df * (1.0 / (double)it);
        else m += df / (double)it;
    }
    mu[(size_t)w * d + j] = m;
}

// ------------------------------------------------- AM increments ahead of the launch (large ndim)
// The AM proposal q = x + U (cd sqrt(S) z) (PT:879-933) costs 2 ndim^2 flops per pick, and its increment depends on the chain's
// stream, the iteration and the scale branch only -- not on its state.  For the 16- and 64-lane shapes (ndim > 104), where a
// chain is a quarter of a wave or a whole one and the kernel's own product ran on the vector pipe (1.2 s per 100 steps of the
// default mix at ndim = 1000), the increments of a piece of the launch are computed AHEAD of it as one matrix product on the
// matrix cores: the piece's AM picks are listed (am_count / am_scan / am_fill: one thread per chain repeats the kernel's cycle
// draw), am_gemm_kernel computes INC[event][:] = sum_k Ut[k][:] w_event[k] -- 64 events per block, every weight generated in the
// block from the event's stream, v_mfma_f64_16x16x4 accumulating k ascending: the oracle's fma chain -- and the step kernel
// reads its increment instead of computing it.
struct AmEvent { long long it; double cd; u32 sid, pad /* the pick's parameter group */; };
struct AmArgs {
    u64 seed;
    long long iter0, nch;
    int nsteps, nt, ntg, temp0, walker0, w_host, w_scam, w_am, w_de, pick_walker;
    int w_gj;                          // NUTS + HMC entries behind the others in the cycle (propose() with GJ)
    int ngroups;                       // parameter groups (PT:129-145): > 1: the pick's group is drawn as propose() draws it
    int per_walker;                    // per-walker covariances: an event's table is its walker's (key = walker * ngroups + group), else key = group
    const double *gcn;                 // [ngroups] 2.4 / sqrt(2 size of the group) (PT:928)
    const int32_t *temp_of;
    const double *temps_mh;
};
// the cycle draw of propose() (ptmi_mh.inc.h) for one (chain, iteration); cd = 2.4 / sqrt(2 ndim) * scale (PT:846-862, 928)
__device__ __forceinline__ bool am_pick(const AmArgs &p, long long ch, long long it, AmEvent &e)
{
    const int w = (int)(ch / p.nt), t = p.temp_of[ch];
    const u32 sid0 = (u32)((u64)(p.walker0 + w) * (u32)p.ntg), sid = sid0 + (u32)(p.temp0 + t);
    u64 p0, p1;
    philox_words(p.seed, (u64)it, sid, 0u, p0, p1);
    u32 pickw = (u32)(p0 >> 32);
    if (p.pick_walker) {
        u64 q0, q1;
        philox_words(p.seed, (u64)it, sid0, 0u, q0, q1);
        pickw = (u32)(q0 >> 32);
    }
    const int L = p.w_host + p.w_scam + p.w_am + p.w_de + p.w_gj;
    const int ind = (int)__umulhi(pickw, (u32)L) - p.w_host;
    if (ind < p.w_scam || ind >= p.w_scam + p.w_am) return false;
    constexpr u32 T97 = (u32)(0.97 * 4294967296.0), T90 = (u32)(0.9 * 4294967296.0);
    const u32 plo = (u32)p0;
    const double temp = p.temps_mh[t];
    const bool warm = temp <= 100.0;
    const double sT = warm ? det_sqrt(temp) : 1.0;
    const double base = plo > T97 ? 10.0 : (plo > T90 ? 0.2 : 1.0);
    u32 g = 0;
    if (p.ngroups > 1) {               // propose()'s group draw (PT:897): its own Philox call
        u64 g0, g1;
        philox_words(p.seed, (u64)it, sid, 2u, g0, g1);
        g = __umulhi((u32)(g0 >> 32), (u32)p.ngroups);
    }
    e.it = it; e.sid = sid; e.pad = g;
    e.cd = p.gcn[g] * (warm ? base * sT : base);
    return true;
}
// (gtot: with parameter groups the picks per group, [ngroups] zeroed by the caller: the block's histogram first)
constexpr int AM_MAXG = 1024;         // = the ABI's limit on ngroups
__global__ __launch_bounds__(256) void am_count_kernel(const AmArgs p, int32_t *count, int32_t *gtot)
{
    __shared__ int32_t lh[AM_MAXG];
    const bool hist = gtot && !p.per_walker;                             // (per walker: thousands of keys, a handful of picks each: straight to memory)
    if (hist)
        for (int g = (int)threadIdx.x; g < p.ngroups; g += 256) lh[g] = 0;
    if (hist) __syncthreads();
    const long long ch = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ch < p.nch) {
        int n = 0;
        AmEvent e;
        const long long kw = p.per_walker ? (ch / p.nt) * p.ngroups : 0;
        for (int s = 0; s < p.nsteps; ++s)
            if (am_pick(p, ch, p.iter0 + s, e)) {
                n += 1;
                if (hist) atomicAdd(&lh[e.pad], 1);
                else if (gtot) atomicAdd(&gtot[kw + e.pad], 1);
            }
        count[ch] = n;
    }
    if (hist) {
        __syncthreads();
        for (int g = (int)threadIdx.x; g < p.ngroups; g += 256)
            if (lh[g]) atomicAdd(&gtot[g], lh[g]);
    }
}
// exclusive prefix sums of the chains' counts, base[nch] = the number of events; two launches of 1024-chain blocks: the blocks' sums, then
// every block adds up the sums before it and scans its own counts (one block over all chains took 0.44 ms at 262 144 chains: its
// threads walked the counts 256 apart)
__device__ __forceinline__ int am_block_scan(int v, int &total, int *wsum /* [16] */)
{
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < 16; ++w) { const int t = wsum[w]; all += t; if (w < wave) before += t; }
    total = all;
    return before + inc - v;                                             // exclusive
}
__global__ __launch_bounds__(1024) void am_scan_sums_kernel(const int32_t *count, int32_t *part, long long nch)
{
    __shared__ int wsum[16];
    const long long i = (long long)blockIdx.x * 1024 + threadIdx.x;
    int total;
    (void)am_block_scan(i < nch ? count[i] : 0, total, wsum);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}
__global__ __launch_bounds__(1024) void am_scan_kernel(const int32_t *count, const int32_t *part, long long *base, long long nch)
{
    __shared__ int wsum[16];
    __shared__ long long off_s;
    __shared__ long long red[16];
    long long off = 0;
    for (int j = (int)threadIdx.x; j < (int)blockIdx.x; j += 1024) off += part[j];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) off += __shfl_down(off, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = off;
    __syncthreads();
    if (threadIdx.x == 0) { long long t = 0; for (int w = 0; w < 16; ++w) t += red[w]; off_s = t; }
    __syncthreads();
    const long long i = (long long)blockIdx.x * 1024 + threadIdx.x;
    int total;
    const int ex = am_block_scan(i < nch ? count[i] : 0, total, wsum);
    if (i < nch) base[i] = off_s + ex;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) base[nch] = off_s + total;
}
// The events in chain order (the step kernel walks its chain's increments in step order); with parameter groups also perm: the
// events' indices listed group by group (group g: perm[gbase[g] ...), in no particular order inside a group -- an event's increment
// does not depend on its neighbours), so that a block of am_gemm_kernel holds 64 events of ONE group and multiplies by that group's
// rows only.  A block reserves its share of every group's list with one atomic per group.
__global__ __launch_bounds__(256) void am_fill_kernel(const AmArgs p, const long long *base, AmEvent *ev, const long long *gbase, int32_t *cursor, int32_t *perm)
{
    __shared__ int32_t lh[AM_MAXG];
    __shared__ long long lb[AM_MAXG];
    const long long ch = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    AmEvent e;
    const bool hist = perm && !p.per_walker;
    if (hist) {
        for (int g = (int)threadIdx.x; g < p.ngroups; g += 256) lh[g] = 0;
        __syncthreads();
        if (ch < p.nch)
            for (int s = 0; s < p.nsteps; ++s)
                if (am_pick(p, ch, p.iter0 + s, e)) atomicAdd(&lh[e.pad], 1);
        __syncthreads();
        for (int g = (int)threadIdx.x; g < p.ngroups; g += 256) {
            lb[g] = lh[g] ? gbase[g] + atomicAdd(&cursor[g], lh[g]) : 0;
            lh[g] = 0;
        }
        __syncthreads();
    }
    if (ch >= p.nch) return;
    long long at = base[ch];
    const long long kw = p.per_walker ? (ch / p.nt) * p.ngroups : 0;
    for (int s = 0; s < p.nsteps; ++s)
        if (am_pick(p, ch, p.iter0 + s, e)) {
            if (hist) perm[lb[e.pad] + atomicAdd(&lh[e.pad], 1)] = (int32_t)at;
            else if (perm) perm[gbase[kw + e.pad] + atomicAdd(&cursor[kw + e.pad], 1)] = (int32_t)at;      // per walker: the key's own cursor
            ev[at++] = e;
        }
}
// 64 events per block of four waves; wave v holds the output tiles v, v + 4, ... (16 rows of the increment each) of all four event
// tiles: at most 8 x 4 tiles of 8 registers = the 256 accumulation registers, i.e. 512 rows of the increment per block.  Beyond
// (ndim <= 1024) two blocks (blockIdx.y) share an event tile, each with half of the output rows and its own copy of the weights.
// The weights of 2 G consecutive directions -- G Box-Muller pairs (k, k + G) per event, the pairing of the step kernels -- are
// generated into LDS one super-chunk ahead of the products that use them.
// Parameter groups (PT:129-145, 897): one launch per group with the group's table (its eigenvectors embedded in the full space, rows
// k < nk = the group's size) over the group's list of events (am_fill_kernel's perm): an event's increment is the k-ascending fma
// chain over ITS group's rows, as the step kernel's own product, and lands in the event's row of inc.
template <int G, int MAXT>
__global__ __launch_bounds__(256, 1) void am_gemm_kernel(const AmEvent *ev, const long long *base, long long nch, int d, const double *Ut,
                                                        const double *S, u64 seed, double *inc, int nk, const long long *kbase /* the lists' starts (+ the end) */,
                                                        const int32_t *perm, int grp, int ngroups, int z0 /* first walker of this launch's grid rows */)
{
    constexpr int NEV = 64, K2 = 2 * G;
    extern __shared__ __attribute__((aligned(16))) double Wl[];          // [2][K2][NEV]
    __shared__ int32_t evi[NEV];                                         // parameter groups: the events' indices (their rows of inc)
    // one group (perm == nullptr): the events e0 .. of the chain-ordered list; else entries e0 .. of the group's list
    // the list's key: the group, or (blockIdx.z = the walker, group) with per-walker covariances -- and the key's table
    const long long key = perm ? ((long long)blockIdx.z + z0) * ngroups + grp : 0;
    const long long seg0 = perm ? kbase[key] : 0;
    const long long nev = perm ? kbase[key + 1] - seg0 : base[nch], e0 = (long long)blockIdx.x * NEV;
    if (e0 >= nev) return;
    Ut += (size_t)key * d * d;
    S += (size_t)key * d;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const bool ev_on = e0 + lane < nev;
    const long long mine = ev_on ? e0 + lane : e0;
    const long long ei = perm ? (long long)perm[seg0 + mine] : mine;
    const AmEvent me = ev[ei];
    if (perm && wave == 0) evi[lane] = (int32_t)ei;
    ps_d4 acc[MAXT][4];
#pragma unroll
    for (int tt = 0; tt < MAXT; ++tt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[tt][ct] = ps_d4{0.0, 0.0, 0.0, 0.0};
    const int ntile = (d + 15) / 16, nsup = (nk + K2 - 1) / K2;
    const int tile0 = (int)blockIdx.y * 4 * MAXT + wave;               // this wave's first output tile
    auto gen = [&](int m, int buf) {
        for (int kk = wave; kk < G; kk += 4) {                          // pair (k, k + G) of event `lane`
            const int k = m * K2 + kk;
            double wa = 0.0, wb = 0.0;
            if (ev_on && k < nk) {
                u64 w0, w1;
                philox_words(seed, (u64)me.it, me.sid, SLOT_AM + (u32)k, w0, w1);
                const double r = det_sqrt(-2.0 * unit_log<0>(w0));
                u32 aj;
                double at, sn, cs;
                unit_angle64(w1, aj, at);
                unit_sincos<0>(aj, at, sn, cs);
                wa = (r * cs) * me.cd * det_sqrt(S[k]);                   // PT:930
                if (k + G < nk) wb = (r * sn) * me.cd * det_sqrt(S[k + G]);
            }
            Wl[((size_t)buf * K2 + kk) * NEV + lane] = wa;
            Wl[((size_t)buf * K2 + kk + G) * NEV + lane] = wb;
        }
    };
    gen(0, 0);
    __syncthreads();
    int buf = 0;
    for (int m = 0; m < nsup; ++m) {
        if (m + 1 < nsup) gen(m + 1, buf ^ 1);
        const double *Wb = Wl + (size_t)buf * K2 * NEV + (size_t)g * NEV + c;
        // The table values go four output tiles at a time: the next group's (the next k-step's first group after the last) are
        // requested before the 16 matrix instructions of this one -- one wave per SIMD, nothing else hides the round trip, and
        // the 256 accumulation registers leave no room to hold a whole k-step ahead.
        auto rows_of = [&](int k0, int grp, double (&dst)[4]) {
            const int kr = k0 + g < nk ? k0 + g : nk - 1;                // rows past the end: their weights are zero
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int col = 16 * (tile0 + 4 * (4 * grp + u)) + c;
                dst[u] = Ut[(size_t)kr * d + (col < d ? col : d - 1)];
            }
        };
        double ga[4], gn[4];
        rows_of(m * K2, 0, ga);
#pragma unroll 1
        for (int ks = 0; ks < K2 / 4; ++ks) {
            const int k0 = m * K2 + 4 * ks;
            if (k0 >= nk) break;                                         // uniform
            double bq[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) bq[ct] = Wb[(size_t)(4 * ks) * NEV + 16 * ct];
#pragma unroll
            for (int grp = 0; grp < MAXT / 4; ++grp) {
                if (grp + 1 < MAXT / 4) rows_of(k0, grp + 1, gn);
                else rows_of(k0 + 4 < nk ? k0 + 4 : k0, 0, gn);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (tile0 + 4 * (4 * grp + u) < ntile) {
#pragma unroll
                        for (int ct = 0; ct < 4; ++ct)
                            acc[4 * grp + u][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(ga[u], bq[ct], acc[4 * grp + u][ct], 0, 0, 0);
                    }
#pragma unroll
                for (int u = 0; u < 4; ++u) ga[u] = gn[u];
            }
        }
        __syncthreads();
        buf ^= 1;
    }
#pragma unroll
    for (int tt = 0; tt < MAXT; ++tt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * (tile0 + 4 * tt) + g + 4 * r;
                const long long e = e0 + 16 * ct + c;
                if (i < d && e < nev) inc[(size_t)(perm ? (long long)evi[16 * ct + c] : e) * d + i] = acc[tt][ct][r];
            }
}

// DE history ring: rows [head, head+mem) are the oldest; overwrite them with the AM buffer.
// Row layout (ptmi_de_row_stride): with 4 lanes per chain a row is stored in 16-byte PIECES dealt to the lanes in turn --
// position 8 (e / 2) + 2 lane + e % 2 holds element lane + 4 e, zero where that is past ndim -- so that one read
// instruction of a DE proposal takes 64 contiguous bytes per chain (16 cache lines per wave instruction, each used
// again by the next instruction).  Round-2 history: in element order the four lanes pulled 8 B each out of 26 x 32-B
// pieces (140 us per step of 262 144 chains); lane-major rows (a lane's 26 values contiguous, 208 B) made every
// instruction touch 64 different lines and a piece straddle 2-3 of them (85 us).
__global__ void de_update_kernel(double *DE, const double *AM, int d, int de_size, int mem, int head, int W, int pooled, int ld, int epl, int am_epl)
{
    const int r = (int)blockIdx.x;   // new row index 0..mem-1 (or the tail when mem > de_size)
    const int wc = (int)blockIdx.y;
    const int skip = mem > de_size ? mem - de_size : 0;
    if (r < skip) return;
    const int phys = (head + (r - skip)) % de_size;
    const int src_w = pooled ? r % W : wc;
    const double *src = AM + ((size_t)src_w * mem + r) * d;
    double *dst = DE + ((size_t)wc * de_size + phys) * ld;
    for (int j = (int)threadIdx.x; j < ld; j += (int)blockDim.x) {
        int i = j;                                                    // element stored at position j
        if (epl) {
            const int e = 2 * (j / 8) + (j & 1);
            i = e < epl ? ((j & 7) >> 1) + 4 * e : d;
        }
        dst[j] = i < d ? src[am_pos(i, am_epl)] : 0.0;
    }
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
    a.de_ld = h->G == 4 ? 8 * ((h->EPL + 1) / 2) : c.ndim;
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

// am_gemm_kernel for up to max_events events (blocks beyond the actual count leave at once: no host round trip for it)
template <int G, int MAXT>
static int launch_am_gemm_t(ptmi_engine *h, long long max_events)
{
    const size_t lds = sizeof(double) * 2 * (2 * G) * 64;
    auto kern = am_gemm_kernel<G, MAXT>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return fail(PTMI_EHIP, "hipFuncSetAttribute(%zu B of LDS): %s", lds, hipGetErrorString(e));
    }
    const int d = h->cfg.ndim, ntile = (d + 15) / 16, parts = (ntile + 4 * MAXT - 1) / (4 * MAXT);      // blocks per event tile
    const int ngr = h->cfg.ngroups > 1 ? h->cfg.ngroups : 1;
    // parameter groups: a launch per group (am_gemm_kernel); with per-walker covariances a grid row per walker, its blocks enough for
    // every pick of the walker's chains in the piece
    const int pw = h->cfg.cov_per_walker ? 1 : 0;
    const long long per_key = pw ? (max_events / h->cfg.nwalkers) : max_events;
    // (a grid's z extent ends at 65535: more walkers than that go in several launches)
    const int nz = pw ? h->cfg.nwalkers : 1;
    for (int g = 0; g < ngr; ++g)
        for (int z0 = 0; z0 < nz; z0 += 65535)
            hipLaunchKernelGGL(kern, dim3((unsigned)((per_key + 63) / 64), parts, (unsigned)(nz - z0 < 65535 ? nz - z0 : 65535)), dim3(256), lds, h->stream,
                               (const AmEvent *)h->d_am_ev, (const long long *)h->d_am_base, (long long)h->cfg.nwalkers * h->cfg.ntemps, d,
                               (const double *)h->buf.Ut, (const double *)h->buf.S, h->cfg.seed, h->d_am_inc, ngr > 1 ? h->gsize_host[g] : d,
                               h->d_am_perm ? (const long long *)h->d_am_kbase : nullptr, (const int32_t *)h->d_am_perm, g, ngr, z0);
    return PTMI_OK;
}
static int launch_am_gemm(ptmi_engine *h, long long max_events)
{
    const int ntile = (h->cfg.ndim + 15) / 16;                          // output tiles of an increment
    if (h->G == 4) return launch_am_gemm_t<4, 4>(h, max_events);        // (parameter groups at ndim <= 104: 7 tiles at most)
    if (h->G == 16) return ntile <= 16 ? launch_am_gemm_t<16, 4>(h, max_events) : launch_am_gemm_t<16, 8>(h, max_events);
    if (h->G == 64) return launch_am_gemm_t<64, 8>(h, max_events);
    return fail(PTMI_EINVAL, "AM increments ahead of the launch: unknown shape");
}

// Scratch for the AM increments of one piece of iterations (am_gemm_kernel), and the split path's cursors into it.  An allocation that
// does not fit is no error: the handle then computes its AM products in the step kernels (split_am_piece = am_piece = 0).
hipError_t ptmi_am_scratch_alloc(ptmi_engine *h, bool am_main)
{
    const ptmi_config &c = h->cfg;
    const ptmi_buffers *buf = &h->buf;
    hipError_t e = hipSuccess;
    const long long nch = (long long)c.nwalkers * c.ntemps;
    // scratch for the increments of one piece (6 GB; 2 GB for the split path alone)
    const double budget = (am_main ? ptmi_env("PTMI_AM_BUDGET_MB", 6144.0) : ptmi_env("PTMI_SPLIT_AM_BUDGET_MB", 2048.0)) * 1048576.0;
    long long piece = (long long)(budget / ((double)c.ndim * 8.0 * (double)nch));
    piece = piece < 1 ? 1 : (piece > 64 ? 64 : piece);
    if ((c.ngroups > 1 || c.cov_per_walker) && nch * piece > 0x7FFFFFFFLL) piece = 0x7FFFFFFFLL / nch;      // (the group lists index the events with 32 bits; nch itself is below 2^32 / ntemps)
    if (piece < 1) piece = 1;
    h->am_piece = am_main ? (int)piece : 0;
    h->split_am_piece = (int)piece;
    h->am_cap = nch * piece;
    if (buf->Q != nullptr) e = hipMalloc((void **)&h->d_am_next, sizeof(long long) * (size_t)(nch + 1));
    if (e == hipSuccess)
    e = hipMalloc((void **)&h->d_am_ev, sizeof(AmEvent) * (size_t)h->am_cap);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_am_count, sizeof(int32_t) * (size_t)(nch + (nch + 1023) / 1024));      // counts | the scan's block sums
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_am_base, sizeof(long long) * (size_t)(nch + 1));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_am_inc, sizeof(double) * (size_t)h->am_cap * c.ndim);
    if (e == hipSuccess && (c.ngroups > 1 || c.cov_per_walker)) {    // the events listed key by key: totals | cursors | the scan's block sums; list starts (+ the end)
        const size_t nkeys = (size_t)(c.ngroups > 1 ? c.ngroups : 1) * (c.cov_per_walker ? (size_t)c.nwalkers : 1);
        if (h->am_cap > 0x7FFFFFFFLL) e = hipErrorInvalidValue;
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_am_grp, sizeof(int32_t) * (2 * nkeys + (nkeys + 1023) / 1024 + 1));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_am_kbase, sizeof(long long) * (nkeys + 1));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_am_perm, sizeof(int32_t) * (size_t)h->am_cap);
    }
    if (e == hipErrorOutOfMemory) {
        // no room for the scratch: the step kernels compute their own AM products (slower, the same results) instead of failing the
        // handle -- configurations that fitted before this path existed still do
        (void)hipGetLastError();
        (void)hipFree(h->d_am_ev); (void)hipFree(h->d_am_count); (void)hipFree(h->d_am_base); (void)hipFree(h->d_am_inc);
        (void)hipFree(h->d_am_grp); (void)hipFree(h->d_am_perm); (void)hipFree(h->d_am_kbase);
        h->d_am_ev = nullptr; h->d_am_count = nullptr; h->d_am_base = nullptr; h->d_am_inc = nullptr;
        h->d_am_grp = nullptr; h->d_am_perm = nullptr; h->d_am_kbase = nullptr;
        (void)hipFree(h->d_am_next); h->d_am_next = nullptr;
        h->am_piece = 0; h->am_cap = 0; h->split_am_piece = 0;
        e = hipSuccess;
    }
    return e;
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
    *stride = s.G == 4 ? 8 * ((s.EPL + 1) / 2) : ndim;
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
    if (e == hipSuccess && !c.cov_per_walker && c.temp0 == 0) {
        const int SL = pool_slab(c.nwalkers, c.ndim), nslab = (c.nwalkers + SL - 1) / SL;
        e = hipMalloc((void **)&h->d_pool_part, sizeof(double) * (size_t)nslab * c.ndim * (c.ndim + 1));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_pool_T, sizeof(double) * (size_t)c.ndim * (c.ndim + 1));
        if (buf->AMflag) {                                                // the slabs' lists of stored rows (pool_rle_kernel)
            const size_t nrows = (size_t)c.nwalkers * c.cov_update;
            if (e == hipSuccess) e = hipMalloc((void **)&h->d_rle_ent, sizeof(PoolEnt) * nrows);
            if (e == hipSuccess) e = hipMalloc((void **)&h->d_rle_cnt, sizeof(int32_t) * (size_t)nslab);
        }
    }
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

// The AM picks of iterations iter0 .. iter0 + ns - 1 listed (am_count / am_scan / am_fill) and their increments computed on the matrix
// cores (am_gemm_kernel) into h->d_am_inc: increment j of a chain's picks in the piece is row h->d_am_base[chain] + j.
static int am_prepare(ptmi_engine *h, long long iter0, int ns)
{
    const ptmi_config &c = h->cfg;
    const long long nch = (long long)c.nwalkers * c.ntemps;
    AmArgs p;
    p.seed = c.seed; p.iter0 = iter0; p.nch = nch; p.nsteps = ns; p.nt = c.ntemps; p.ntg = c.ntemps_global; p.temp0 = c.temp0;
    p.walker0 = c.walker0; p.w_host = c.w_host; p.w_scam = c.w_scam; p.w_am = c.w_am; p.w_de = h->de_on ? c.w_de : 0;
    p.w_gj = c.w_nuts + c.w_hmc;
    p.pick_walker = c.pick_mode == PTMI_PICK_WALKER; p.ngroups = c.ngroups > 1 ? c.ngroups : 1; p.gcn = h->d_gcn;
    p.per_walker = c.cov_per_walker ? 1 : 0;
    p.temp_of = h->buf.temp_of; p.temps_mh = h->d_temps;
    const unsigned gch = (unsigned)((nch + 255) / 256);
    const int ngr = p.ngroups;
    const long long nkeys = (long long)ngr * (c.cov_per_walker ? c.nwalkers : 1);
    int32_t *gtot = h->d_am_perm ? h->d_am_grp : nullptr, *gcur = gtot ? gtot + nkeys : nullptr, *gpart = gtot ? gtot + 2 * nkeys : nullptr;
    if (gtot) HIPCHK(hipMemsetAsync(gtot, 0, sizeof(int32_t) * 2 * (size_t)nkeys, h->stream));          // the keys' totals and the fill's cursors
    hipLaunchKernelGGL(am_count_kernel, dim3(gch), dim3(256), 0, h->stream, p, h->d_am_count, gtot);
    if (gtot) {                                                  // the lists' starts: the chains' scan over the keys' totals
        const unsigned gk = (unsigned)((nkeys + 1023) / 1024);
        hipLaunchKernelGGL(am_scan_sums_kernel, dim3(gk), dim3(1024), 0, h->stream, (const int32_t *)gtot, gpart, nkeys);
        hipLaunchKernelGGL(am_scan_kernel, dim3(gk), dim3(1024), 0, h->stream, (const int32_t *)gtot, (const int32_t *)gpart, h->d_am_kbase, nkeys);
    }
    const unsigned gsc = (unsigned)((nch + 1023) / 1024);
    hipLaunchKernelGGL(am_scan_sums_kernel, dim3(gsc), dim3(1024), 0, h->stream, (const int32_t *)h->d_am_count, h->d_am_count + nch, nch);
    hipLaunchKernelGGL(am_scan_kernel, dim3(gsc), dim3(1024), 0, h->stream, (const int32_t *)h->d_am_count, (const int32_t *)(h->d_am_count + nch),
                       h->d_am_base, nch);
    hipLaunchKernelGGL(am_fill_kernel, dim3(gch), dim3(256), 0, h->stream, p, (const long long *)h->d_am_base, (AmEvent *)h->d_am_ev,
                       (const long long *)h->d_am_kbase, gcur, gtot ? h->d_am_perm : nullptr);
    if (int rc = launch_am_gemm(h, nch * ns)) return rc;
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
            if (int rc = am_prepare(h, iter0 + s0, ns)) return rc;
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

int ptmi_split_am_piece(ptmi_handle h, int32_t *piece)
{
    if (!h || !piece) return fail(PTMI_EINVAL, "NULL argument");
    *piece = (h->cfg.w_am > 0 && ptmi_split_rows_ok(h)) ? h->split_am_piece : 0;
    return PTMI_OK;
}

int ptmi_split_am_prepare(ptmi_handle h, int64_t iter0, int32_t nsteps)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (h->cfg.w_am <= 0) return PTMI_OK;
    if (h->split_am_piece <= 0 || !h->d_am_next) return fail(PTMI_EUNSUPPORTED, "this handle's split path takes its AM proposals from the shape kernels");
    if (nsteps < 1 || nsteps > h->split_am_piece) return fail(PTMI_EINVAL, "ptmi_split_am_prepare: 1 <= nsteps <= %d (ptmi_split_am_piece)", h->split_am_piece);
    if (int rc = am_prepare(h, (long long)iter0, nsteps)) return rc;
    const long long nch = (long long)h->cfg.nwalkers * h->cfg.ntemps;
    HIPCHK(hipMemcpyAsync(h->d_am_next, h->d_am_base, sizeof(long long) * (size_t)(nch + 1), hipMemcpyDeviceToDevice, h->stream));      // every chain's cursor at its first increment
    HIPCHK(hipGetLastError());
    h->split_am_lo = iter0;
    h->split_am_hi = iter0 + nsteps;
    return PTMI_OK;
}

int ptmi_proposals(ptmi_handle h, double **q)
{
    if (!h || !q) return fail(PTMI_EINVAL, "NULL argument");
    *q = (h->q_cur && h->buf.Q2) ? h->buf.Q2 : h->buf.Q;
    return PTMI_OK;
}

int ptmi_update_cov(ptmi_handle h, int64_t iter) { return ptmi_update_cov_on(h, iter, nullptr, nullptr, nullptr); }

int ptmi_set_am_buffers(ptmi_handle h, double *AM, double *AMaux, uint64_t *AMflag)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (!AM || !h->buf.AM) return fail(PTMI_EINVAL, "the handle was created without an AM buffer, or AM is NULL");
    if ((AMaux != nullptr) != (h->buf.AMaux != nullptr) || (AMflag != nullptr) != (h->buf.AMflag != nullptr))
        return fail(PTMI_EINVAL, "AMaux / AMflag must be given exactly when the handle was created with them");
    h->buf.AM = AM; h->buf.AMaux = AMaux; h->buf.AMflag = AMflag;
    return PTMI_OK;
}

int ptmi_update_cov_on(ptmi_handle hh, int64_t iter, void *stream, const double *AM_in, const uint64_t *AMflag_in)
{
    if (!hh) return fail(PTMI_EINVAL, "NULL handle");
    // a view of the handle with the caller's stream and ring: the statistics below read h->stream / h->buf.AM / h->buf.AMflag only
    // (the scratch, the diagonal tiles' helper stream and mu / M2 / cov are the handle's own: one statistics call at a time)
    ptmi_engine view = *hh;
    if (stream) view.stream = (hipStream_t)stream;
    if (AM_in) { view.buf.AM = const_cast<double *>(AM_in); view.buf.AMflag = const_cast<uint64_t *>(AMflag_in); }
    ptmi_engine *h = &view;
    struct Back { ptmi_engine *to, *from; ~Back() { to->side = from->side; to->side_go = from->side_go; to->side_done = from->side_done; } } back{hh, h};
    const ptmi_config &c = h->cfg;
    if (c.temp0 != 0) return PTMI_OK;   // only the GPU holding rank 0 adapts (PT:545)
    if (!h->buf.AM || !h->buf.mu || !h->buf.M2 || !h->buf.cov) return fail(PTMI_EINVAL, "AM/mu/M2/cov buffers missing");
    if (iter < c.cov_update || iter % c.cov_update) return fail(PTMI_EINVAL, "iter must be a positive multiple of cov_update");
    const int d = c.ndim, nt = (d + WTILE - 1) / WTILE;
    if (c.cov_per_walker) {
        if (d <= 100)
            hipLaunchKernelGGL((welford_rows_kernel<25, 10, 4, 10>), dim3((c.nwalkers + 1) / 2), dim3(768), 0, h->stream, (const double *)h->buf.AM,
                               h->buf.mu, h->buf.M2, h->buf.cov, d, c.cov_update, (long long)iter, d * d, am_row_epl(h->G, h->EPL), c.nwalkers);
        else
        hipLaunchKernelGGL(welford_kernel<false>, dim3(nt, nt, c.nwalkers), dim3(256), 0, h->stream, (const double *)h->buf.AM,
                           h->buf.mu, h->buf.M2, h->buf.cov, d, c.cov_update, (long long)iter, d * d, am_row_epl(h->G, h->EPL));
        if (nt > 1)
            hipLaunchKernelGGL(welford_mean_kernel, dim3((d + 63) / 64, c.nwalkers), dim3(64), 0, h->stream, (const double *)h->buf.AM,
                               h->buf.mu, d, c.cov_update, (long long)iter, 0, am_row_epl(h->G, h->EPL));
    } else {
        // pooled statistics (orc_pool_update): mu[0 .. d), M2[0 .. d*d) of the buffers are the pooled state
        const int W = c.nwalkers, SL = pool_slab(W, d), nslab = (W + SL - 1) / SL, ng = pool_groups(d);
        const long long nrows = (long long)W * c.cov_update;
        const bool first = iter == c.cov_update;
        const double *shift = first ? (const double *)h->buf.AM : (const double *)h->buf.mu;     // the first epoch: walker 0's row 0
        // Several macro tiles per side: the diagonal ones (nslab x ng blocks, half a round of the chip) go to a side stream and
        // fill the last, partly empty round of the off-diagonal ones instead of a launch of their own behind them
        // (1000-d, 512 walkers: 288 blocks beside 1152 with 512 resident at a time).
        hipStream_t diag_stream = h->stream;
        // AM row flags: the slabs' lists of stored rows and run lengths first, then the sums over them
        const bool rle = h->buf.AMflag != nullptr, pair = d % 2 == 0;
        const PoolRle pr = {(const PoolEnt *)h->d_rle_ent, h->d_rle_cnt};
        const long long rps = (long long)SL * c.cov_update;
        if (rps * d * 8 >= (1ll << 32)) return fail(PTMI_EUNSUPPORTED, "pooled statistics: a slab of %d walkers x %d rows x %d parameters exceeds 4 GB", SL, c.cov_update, d);
        const int aepl = am_row_epl(h->G, h->EPL), sepl = first ? am_row_epl(h->G, h->EPL) : 0;
        if (rle) hipLaunchKernelGGL(pool_rle_kernel, dim3(nslab), dim3(256), 0, h->stream, (const AmFlag *)h->buf.AMflag, nrows, rps, (PoolEnt *)h->d_rle_ent,
                                    h->d_rle_cnt);
        auto syrk = [&](auto diag, dim3 grid, hipStream_t st) {
            constexpr bool DG = decltype(diag)::value;
            const void *fn = rle ? (pair ? (const void *)pool_syrk_kernel<DG, true, true> : (const void *)pool_syrk_kernel<DG, true, false>)
                                 : (pair ? (const void *)pool_syrk_kernel<DG, false, true> : (const void *)pool_syrk_kernel<DG, false, false>);
            const double *rows = (const double *)h->buf.AM;
            long long nr = nrows, rp = rps;
            int dd = d, ae = aepl, se = sepl;
            double *part = h->d_pool_part;
            PoolRle prl = pr;
            void *args[] = {&rows, &nr, &dd, (void *)&shift, &rp, &part, &ae, &se, &prl};
            return hipLaunchKernel(fn, grid, dim3(256), args, 0, st);
        };
        if (ng > 1) {
            if (!h->side) {
                HIPCHK(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
                HIPCHK(hipEventCreateWithFlags(&h->side_go, hipEventDisableTiming));
                HIPCHK(hipEventCreateWithFlags(&h->side_done, hipEventDisableTiming));
            }
            HIPCHK(hipEventRecord(h->side_go, h->stream));
            HIPCHK(hipStreamWaitEvent(h->side, h->side_go, 0));
            HIPCHK(syrk(std::false_type{}, dim3(ng * (ng - 1) / 2, nslab), h->stream));
            diag_stream = h->side;
        }
        HIPCHK(syrk(std::true_type{}, dim3(ng, nslab), diag_stream));
        if (ng > 1) {
            HIPCHK(hipEventRecord(h->side_done, h->side));
            HIPCHK(hipStreamWaitEvent(h->stream, h->side_done, 0));
        }
        const long long nel = (long long)d * (d + 1);
        hipLaunchKernelGGL(pool_reduce_kernel, dim3((unsigned)((nel + 63) / 64)), dim3(64), 0, h->stream, (const double *)h->d_pool_part, nslab, d,
                           h->d_pool_T);
        const double nb = (double)W * (double)c.cov_update, nprev = (double)W * (double)(iter - c.cov_update);
        hipLaunchKernelGGL(pool_finish_kernel, dim3((unsigned)(((long long)d * d + 255) / 256)), dim3(256), 0, h->stream, (const double *)h->d_pool_T,
                           shift, first ? am_row_epl(h->G, h->EPL) : 0, h->buf.mu, h->buf.M2, h->buf.cov, d, first ? 1 : 0, nb, nprev * nb / (nprev + nb), nb / (nprev + nb),
                           nprev + nb - 1.0);
    }
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

int ptmi_am_expand(ptmi_handle h, int32_t w0, int32_t nw, int64_t iter_lo, int64_t iter_hi)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    const ptmi_config &c = h->cfg;
    if (!h->buf.AMflag || !h->buf.AM) return PTMI_OK;                    // every row is stored already
    if (w0 < 0 || nw < 0 || w0 + nw > c.nwalkers) return fail(PTMI_EINVAL, "walkers [%d, %d) of %d", w0, w0 + nw, c.nwalkers);
    const long long base = iter_hi > 0 ? ((long long)(iter_hi - 1) / c.cov_update) * c.cov_update : 0;
    if (iter_lo < base || iter_hi < iter_lo || iter_hi - iter_lo >= c.cov_update)
        return fail(PTMI_EINVAL, "iterations %lld..%lld are not inside the covariance period that starts at %lld (with AM row flags the ring keeps "
                                 "the rows of the current period only)", (long long)iter_lo, (long long)iter_hi, base);
    if (nw == 0) return PTMI_OK;
    hipLaunchKernelGGL(am_expand_kernel, dim3((unsigned)nw), dim3(128), 0, h->stream, h->buf.AM, (const AmFlag *)h->buf.AMflag, c.ndim, c.cov_update,
                       (int)w0, (long long)iter_lo, (long long)iter_hi, base);
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

int ptmi_test_replay(ptmi_handle h, const double *swap_uniforms, const uint64_t *draws)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    h->rp_swap_u = swap_uniforms;
    h->rp_draws = (const u64 *)draws;
    return PTMI_OK;
}

int ptmi_update_de(ptmi_handle h)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    const ptmi_config &c = h->cfg;
    if (!h->buf.DE) return PTMI_OK;
    if (!h->buf.AM) return fail(PTMI_EINVAL, "DE update needs the AM buffer on this GPU");
    const int wc = c.cov_per_walker ? c.nwalkers : 1;
    hipLaunchKernelGGL(de_update_kernel, dim3(c.cov_update, wc), dim3(64), 0, h->stream, h->buf.DE, (const double *)h->buf.AM,
                       c.ndim, c.de_size, c.cov_update, h->de_head, c.nwalkers, c.cov_per_walker ? 0 : 1,
                       h->G == 4 ? 8 * ((h->EPL + 1) / 2) : c.ndim, h->G == 4 ? h->EPL : 0, am_row_epl(h->G, h->EPL));
    HIPCHK(hipGetLastError());
    const int adv = c.cov_update < c.de_size ? c.cov_update : c.de_size;
    h->de_head = (h->de_head + adv) % c.de_size;
    return PTMI_OK;
}

int ptmi_set_de_head(ptmi_handle h, int32_t head)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (head < 0 || head >= h->cfg.de_size) return fail(PTMI_EINVAL, "head %d outside the ring of %d rows", head, h->cfg.de_size);
    h->de_head = head;
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
