// ptmi_cov.hip -- what libptmi.so runs at a covariance epoch: the per-walker (Welford) and the pooled statistics, the AM ring's
// expansion and the DE ring's update: the kernels, then their entry points.  They reach the engine through the handle's fields
// only (ptmi_common.h).
#include <math.h>
#include <stdlib.h>

#include <type_traits>

#include "ptmi_common.h"

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

// Scratch of the pooled statistics, for ptmi_create: the slabs' partial sums and their total, and with AM row flags the slabs'
// lists of stored rows (pool_rle_kernel).  ptmi_destroy frees the fields.
hipError_t ptmi_pool_scratch_alloc(ptmi_engine *h)
{
    const ptmi_config &c = h->cfg;
    const int SL = pool_slab(c.nwalkers, c.ndim), nslab = (c.nwalkers + SL - 1) / SL;
    hipError_t e = hipMalloc((void **)&h->d_pool_part, sizeof(double) * (size_t)nslab * c.ndim * (c.ndim + 1));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_pool_T, sizeof(double) * (size_t)c.ndim * (c.ndim + 1));
    if (h->buf.AMflag) {
        const size_t nrows = (size_t)c.nwalkers * c.cov_update;
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_rle_ent, sizeof(PoolEnt) * nrows);
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_rle_cnt, sizeof(int32_t) * (size_t)nslab);
    }
    return e;
}

extern "C" {

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

int ptmi_update_de(ptmi_handle h)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    const ptmi_config &c = h->cfg;
    if (!h->buf.DE) return PTMI_OK;
    if (!h->buf.AM) return fail(PTMI_EINVAL, "DE update needs the AM buffer on this GPU");
    const int wc = c.cov_per_walker ? c.nwalkers : 1;
    hipLaunchKernelGGL(de_update_kernel, dim3(c.cov_update, wc), dim3(64), 0, h->stream, h->buf.DE, (const double *)h->buf.AM,
                       c.ndim, c.de_size, c.cov_update, h->de_head, c.nwalkers, c.cov_per_walker ? 0 : 1,
                       de_row_ld(h->G, h->EPL, c.ndim), h->G == 4 ? h->EPL : 0, am_row_epl(h->G, h->EPL));
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

}  // extern "C"
