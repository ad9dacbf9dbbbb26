// ptmi_swap.hip -- the PT swap of libptmi.so and the exchange of rows across the edges of the ladder's blocks: the kernels, then
// their entry points.  They reach the engine through the handle's fields only (ptmi_common.h).
#include <math.h>
#include <stdlib.h>

#include "ptmi_common.h"

// --------------------------------------------------------------------- swap
__global__ void gather_lnl_kernel(const double *lnL, const int32_t *slot_of, double *out, long long n, int nt)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long w = i / nt;
    out[i] = lnL[w * nt + slot_of[i]];
}

// PT:666-686 in two kernels.  swap_prepare_kernel (one thread per position and walker) does everything that does
// not depend on the carried state: the LOGARITHM of the pair's uniform (PT:679's u <= exp(sum) is tested as log u <= sum,
// as the oracle defines it: the transcendental leaves the recurrence) and every quotient of a position's OWN likelihood,
// L[k] / T[k], L[k] / T[k+1] and L[k] / T[k-1].  swap_sweep_kernel (one lane per walker) then runs the hot -> cold
// recurrence with the carried map.  Scratch: one 48-byte record per (position, walker), position-major [n][W], so a pair
// costs the sweep three 16-byte loads per lane from one wave-uniform base and a wave reads 3 KB in a row.  When the whole
// ladder is local (slot_of != nullptr) the slot tables are rewritten in place: position k+1 becomes final at step k and
// positions <= k are still untouched.
struct __attribute__((aligned(16))) SwapPre {
    double lu, L;        // log of the pair's uniform; the position's likelihood
    double a, b;         // -L/T[k], L/T[k+1]
    double c;            // L/T[k-1]
    int32_t row, pad;    // the slot that holds the position (whole ladder local)
};
static_assert(sizeof(SwapPre) == PTMI_SWAP_PRE_BYTES, "three 16-byte loads");
// what a record is made from
struct SwapSrc {
    const double *ladder, *lnL_pos, *lnL_rows;
    const int32_t *slot_of;      // whole ladder local: the slot tables (else nullptr: lnL_pos holds the likelihoods by position)
    long long iter;
    u64 seed;
    int walker0;
    int block_nt;                // > 0: lnL_pos is [n / block_nt][W][block_nt], as all-gathered
    const double *u_over;        // TEST HOOK (ptmi_test_replay): the pair uniforms [W][n - 1] as recorded from the reference, or nullptr
};
__device__ __forceinline__ SwapPre swap_record(const SwapSrc &p, int W, int n, int k, int w)
{
    const bool fused = p.slot_of != nullptr;
    const int row = fused ? p.slot_of[(size_t)w * n + k] : 0;
    const double L = fused ? p.lnL_rows[(size_t)w * n + row]
                   : (p.block_nt > 0 ? p.lnL_pos[((size_t)(k / p.block_nt) * W + w) * p.block_nt + k % p.block_nt] : p.lnL_pos[(size_t)w * n + k]);
    double u = 0.0, b = 0.0, c = 0.0;
    if (k < n - 1) {
        const u32 sid = (u32)((u64)(p.walker0 + w) * (u32)n + 0u);    // rank 0's stream (PT:679)
        u64 w0, w1;
        philox_words(p.seed, (u64)p.iter, sid, SLOT_SWAP + (u32)k, w0, w1);
        u = det_log(p.u_over ? p.u_over[(size_t)w * (n - 1) + k] : w2uniform(w0));   // log of the [0,1) uniform; -inf for u = 0: always accepted
        b = L / p.ladder[k + 1];
    }
    if (k > 0) c = L / p.ladder[k - 1];
    SwapPre r;
    r.lu = u; r.L = L; r.a = -L / p.ladder[k]; r.b = b; r.c = c; r.row = fused ? row : k; r.pad = 0;
    return r;
}
__global__ void swap_prepare_kernel(int W, int n, SwapSrc src, SwapPre *pre)
{
    // grid (walkers, positions); the 2 M records of a 512-rank ladder are 100 MB: this kernel is bound by writing them
    const int k = (int)blockIdx.y, w = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (w >= W) return;
    pre[(size_t)k * W + (size_t)w] = swap_record(src, W, n, k, w);
}

// The recurrence of pair k (positions k, k+1; carried state of likelihood Lc at k+1) is the reference's four-term sum in
// its order, -L[k]/T[k] - Lc/T[k+1] + Lc/T[k] + L[k]/T[k+1], against log u.  The two quotients of Lc are carried along with
// it: if the pair accepts, Lc moves on and pair k-1 needs Lc/T[k] (this pair's third term) and Lc/T[k-1] -- ONE new division,
// independent of this pair's decision, so it runs in the shadow of the sums and the compare; if it rejects, the new carried
// state is position k's own and both quotients come from the prepared arrays (-(-L[k]/T[k]) and L[k]/T[k-1]; negation is
// exact).  Same operations on the same values as the oracle: bit-identical decisions.  Per pair the serial path is three
// sums, a compare and the selects (0.65 us per pair with two divisions and an exp on it, round 2).
// parity >= 0 (odd/even mode): only the pairs with k = parity (mod 2) are tried; an untried pair never accepts, so
// the carried state is always position k+1's own and the recurrence degenerates into independent pair tests.
// STG: the tables the sweep writes are [walker][position] -- a lane per walker scatters 4-byte stores 4 n bytes apart, 64
// memory transactions per store instruction.  So the block (one wave = 64 walkers) keeps its walkers' forward table and
// acceptance flags in LDS (rows of n + 1 ints: a lane per bank) and writes them out at the end with the lanes along the
// position, building the inverse table there.  2 x wpb x (n + 1) ints: 64 walkers per block up to 319 ranks, 32 / 16 / 8
// for longer ladders (512 ranks of an 8-GPU ladder: 32); beyond that the direct stores (STG = false).
#ifndef PTMI_SWEEP_BATCH
#define PTMI_SWEEP_BATCH 8
#endif
// the AM-buffer row of a swap iteration (PT:624-627, 327-328): the state that sits at rank 0 after the sweep
struct SwapAmRow { const double *X, *lnL, *lp; double *AM, *AMaux; int d, cov_update, am_epl; long long iter; AmFlag *AMflag; };
// the post-swap rows are KEY rows (AM row flags, ptmi_common.h)
__device__ __forceinline__ void swap_am_key(const SwapAmRow &amr, int w0, int nw, int tid, int nthreads)
{
    if (amr.AMflag == nullptr) return;
    const int ring = (int)(amr.iter % amr.cov_update);
    for (int wl = tid; wl < nw; wl += nthreads) amr.AMflag[(size_t)(w0 + wl) * amr.cov_update + (size_t)ring] = AMROW_KEY;
}
template <bool STG>
__global__ __launch_bounds__(STG ? 256 : 64) void swap_sweep_kernel(int W, int n, const double *ladder, const SwapPre *pre,
                                  int32_t *slot_of, int32_t *temp_of, int32_t *map, u64 *nswap, int local0, int nlocal,
                                  int parity, int32_t *inv /* with map: inv[w][map[w][j]] = j */,
                                  int wpb /* walkers per block: 64, fewer when a long ladder's tables would not fit the LDS */,
                                  int hop_nt, int32_t *hop_flag /* hop_nt > 0 (STG, map form): set *hop_flag when a state moves beyond a
                                                                 * neighbouring block of hop_nt ranks (ptmi_exchange_multihop) */,
                                  SwapAmRow amr /* STG, fused: the write-out also stores the swap iteration's AM row (am_write_kernel) */)
{
    // STG blocks have four waves: the first runs the recurrence (a lane per walker), all four write the tables out
    extern __shared__ int32_t sw_lds[];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int w = (int)blockIdx.x * wpb + lane;
    const bool fused = slot_of != nullptr;
    const int ld = n + 1;
    int32_t *const l0 = sw_lds + (size_t)lane * ld;                    // slot_of / map of this lane's walker
    int32_t *const lf = sw_lds + (size_t)(wpb + lane) * ld;            // pair k accepted
    if (wave == 0 && lane < wpb && w < W) {
    int32_t *fw = STG ? l0 : (fused ? slot_of + (size_t)w * n : map + (size_t)w * n);     // forward table: row (fused) or source position
    int32_t *bw = STG ? nullptr : (fused ? temp_of + (size_t)w * n : inv + (size_t)w * n); // its inverse (STG: built at write-out)
    const SwapPre top = pre[(size_t)(n - 1) * W + w];
    int crow = top.row;                    // what the forward table says about the state carried at k+1 (its slot, or its position)
    double Lc = top.L;
    double q1 = -top.a;                    // Lc / T[k+1]
    double q0 = top.c;                     // Lc / T[k]
    // Only (Lc, q1, q0) are carried from pair to pair.  The scratch of SW pairs is fetched at once into one of two register
    // sets (this kernel runs one wave per SIMD: registers are free), the NEXT batch being requested before the current one
    // is worked through, so that one memory latency is exposed per launch instead of one per batch (round 2's version
    // requested T[k] through the scalar unit, one waited-for load per pair: 0.5 us per pair whatever the arithmetic).
    // Indices below 0 are clamped, not branched around: their values are never used.
    constexpr int SW = PTMI_SWEEP_BATCH;
    struct Batch { double u[SW], L[SW], a[SW], b[SW], c[SW], T[SW]; int r[SW]; };
    // addresses: the lane's record of position 0 (computed once) + a wave-uniform stride per position
    const char *const lane0 = reinterpret_cast<const char *>(pre + ((size_t)blockIdx.x * wpb + (unsigned)lane));
    const size_t kstride = (size_t)W * sizeof(SwapPre);
    auto fetch = [&](int k0, Batch &B) {
#pragma unroll
        for (int j = 0; j < SW; ++j) {
            const int kk = k0 - j > 0 ? k0 - j : 0;
            const SwapPre r = *reinterpret_cast<const SwapPre *>(lane0 + (size_t)kk * kstride);
            B.u[j] = r.lu; B.L[j] = r.L; B.a[j] = r.a; B.b[j] = r.b; B.c[j] = r.c; B.r[j] = r.row;
            B.T[j] = ladder[kk > 0 ? kk - 1 : 0];                       // T[k-1] (uniform: a scalar load)
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto chain = [&](int k0, const Batch &B) {
#pragma unroll
        for (int j = 0; j < SW; ++j) {
            const int k = k0 - j;
            if (k < 0) break;
            const double spec = Lc / B.T[j];   // Lc / T[k-1]: needed if this pair accepts; does not wait for its decision
            double la = B.a[j];                // -L[k] / T[k]
            la += -q1;                         // -Lc / T[k+1]
            la += q0;                          //  Lc / T[k]
            la += B.b[j];                      //  L[k] / T[k+1]
            const bool acc = (parity < 0 || (k & 1) == parity) && B.u[j] <= la;      // log u <= sum
            // position k+1 is final: it keeps the carried state, or takes position k's
            const int fin = acc ? B.r[j] : crow;
            fw[k + 1] = fin;
            if (!STG) bw[fin] = k + 1;
            if (STG) lf[k] = acc ? 1 : 0;
            else if (acc && k >= local0 && k < local0 + nlocal) atomicAdd((unsigned long long *)&nswap[(size_t)w * n + k], 1ull);   // no-return atomic
            q1 = acc ? q0 : -B.a[j];
            q0 = acc ? spec : B.c[j];
            Lc = acc ? Lc : B.L[j];
            crow = acc ? crow : B.r[j];
        }
    };
    Batch A, B;
    fetch(n - 2, A);
    for (int k0 = n - 2; k0 >= 0; k0 -= 2 * SW) {
        if (k0 - SW >= 0) fetch(k0 - SW, B);
        chain(k0, A);
        if (k0 - SW < 0) break;
        if (k0 - 2 * SW >= 0) fetch(k0 - 2 * SW, A);
        chain(k0 - SW, B);
    }
    fw[0] = crow;
    if (!STG) bw[crow] = 0;
    }
    // block of a position (the multi-hop scan of the write-out): filled by the waves that sit out the recurrence
    int32_t *const blk = sw_lds + (size_t)2 * wpb * ld;
    if (STG && hop_nt > 0 && wave > 0)
        for (int k = (int)threadIdx.x - 64; k < n; k += 192) blk[k] = k / hop_nt;
    if (STG) {
        __syncthreads();
        const int w0 = (int)blockIdx.x * wpb;
        int32_t *g0 = fused ? slot_of : map, *g1 = fused ? temp_of : inv;
        const int nw = W - w0 < wpb ? W - w0 : wpb;
        bool far = false;
        for (int wl = wave; wl < nw; wl += 4) {                        // a wave per walker, the lanes along the position
            const size_t row = (size_t)(w0 + wl) * n;
            for (int k = lane; k < n; k += 64) {
                const int f = sw_lds[(size_t)wl * ld + k];
                g0[row + k] = f;
                g1[row + f] = k;                                       // the inverse table: a scatter inside the walker's own row
                if (hop_nt > 0) { const int hop = blk[f] - blk[k]; far = far || hop > 1 || hop < -1; }
                // a no-return atomic: fire and forget (a read-modify-write would wait for its load in every trip: 37 against 24 us)
                if (k < n - 1 && k >= local0 && k < local0 + nlocal && sw_lds[(size_t)(wpb + wl) * ld + k])
                    atomicAdd((unsigned long long *)&nswap[row + k], 1ull);
            }
        }
        if (hop_nt > 0 && __ballot(far) != 0 && lane == 0) atomicOr(hop_flag, 1);   // once per wave at most
        if (amr.AM != nullptr) {
            // the rows now at rank 0 into the AM ring (am_write_kernel's copy): the block's nw rows as one list of elements, six
            // reads in flight per thread (a wave per walker waited for sixteen round trips in turn)
            constexpr int NB = 6;
            const int tot = nw * amr.d, ring = (int)(amr.iter % amr.cov_update);
            for (int base = (int)threadIdx.x; base < tot; base += 256 * NB) {
                double v[NB];
                size_t dst[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int idx = base + 256 * u, ic = idx < tot ? idx : tot - 1;
                    const int wl = ic / amr.d, i = ic % amr.d;
                    const size_t r = (size_t)(w0 + wl) * n + (size_t)sw_lds[(size_t)wl * ld];
                    v[u] = amr.X[r * amr.d + i];
                    dst[u] = ((size_t)(w0 + wl) * amr.cov_update + (size_t)ring) * amr.d + (size_t)am_pos(i, amr.am_epl);
                }
#pragma unroll
                for (int u = 0; u < NB; ++u)
                    if (base + 256 * u < tot) amr.AM[dst[u]] = v[u];
            }
            if (amr.AMaux)
                for (int wl = (int)threadIdx.x; wl < nw; wl += 256) {
                    const size_t r = (size_t)(w0 + wl) * n + (size_t)sw_lds[(size_t)wl * ld];
                    const size_t arow = (size_t)(w0 + wl) * amr.cov_update + (size_t)ring;
                    amr.AMaux[arow * 2] = amr.lnL[r];
                    amr.AMaux[arow * 2 + 1] = amr.lp[r];
                }
            swap_am_key(amr, w0, nw, (int)threadIdx.x, 256);
        }
    }
}

// The sweep with its records made in the block (no scratch in memory: the 48-byte records of a 512-rank ladder are 100 MB
// written and read back, 34 us of the 160 us a swap epoch takes on one of eight GPUs; with 64 ranks the prepare kernel and its
// launch gap are a third of the epoch).  Blocks of 512 threads: wave 0 runs the recurrence as in swap_sweep_kernel<true>, six
// of the others (not wave 4, which sits on the recurrence's SIMD) make the records of the batch after next (eight pairs) into a
// three-slot LDS ring while it works through the current one and reads the next into its second register set; one barrier
// per batch.  Same records, same recurrence, same write-out: bit-identical.
constexpr int SWF_BLK = 512;
__host__ __device__ inline size_t swf_ring_offset(int wpb, int n) { return ((sizeof(int32_t) * (2 * (size_t)wpb * (size_t)(n + 1) + (size_t)n)) + 15) & ~(size_t)15; }
__host__ __device__ inline size_t swf_lds_bytes(int wpb, int n) { return swf_ring_offset(wpb, n) + sizeof(SwapPre) * (size_t)(3 * PTMI_SWEEP_BATCH + 1) * (size_t)wpb; }
__global__ __launch_bounds__(SWF_BLK) void swap_fused_kernel(int W, int n, SwapSrc src, int32_t *slot_of, int32_t *temp_of, int32_t *map,
                                                          u64 *nswap, int local0, int nlocal, int parity, int32_t *inv, int wpb, int wpb_log2,
                                                          int hop_nt, int32_t *hop_flag, SwapAmRow amr)
{
    extern __shared__ int32_t sw_lds[];
    constexpr int SW = PTMI_SWEEP_BATCH;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w0 = (int)blockIdx.x * wpb, w = w0 + lane;
    const bool fused = slot_of != nullptr;
    const int ld = n + 1;
    int32_t *const fw = sw_lds + (size_t)lane * ld;                    // slot_of / map of this lane's walker
    int32_t *const lf = sw_lds + (size_t)(wpb + lane) * ld;            // pair k accepted
    int32_t *const blk = sw_lds + (size_t)2 * wpb * ld;
    SwapPre *const ring = reinterpret_cast<SwapPre *>(reinterpret_cast<char *>(sw_lds) + swf_ring_offset(wpb, n));   // [3][SW][wpb]
    SwapPre *const topr = ring + (size_t)3 * SW * wpb;                 // [wpb]: the records of position n - 1
    const int NB = (n - 1 + SW - 1) / SW;                              // batches of the pairs n - 2 .. 0
    auto produce = [&](int b, int t0, int nthr) {                      // batch b by the threads t0 .. t0 + nthr - 1
        const int k0 = n - 2 - b * SW;
        for (int idx = tid - t0; idx < SW * wpb; idx += nthr) {
            const int j = idx >> wpb_log2, wl = idx & (wpb - 1), k = k0 - j;
            if (k >= 0 && w0 + wl < W) ring[((size_t)(b % 3) * SW + j) * wpb + wl] = swap_record(src, W, n, k, w0 + wl);
        }
    };
    for (int wl = tid; wl < wpb; wl += SWF_BLK)
        if (w0 + wl < W) topr[wl] = swap_record(src, W, n, n - 1, w0 + wl);
    if (NB > 0) produce(0, 0, SWF_BLK);
    if (NB > 1) produce(1, 0, SWF_BLK);
    if (hop_nt > 0)
        for (int k = tid; k < n; k += SWF_BLK) blk[k] = k / hop_nt;
    __syncthreads();
    const bool chainer = wave == 0 && lane < wpb && w < W;
    if (wave == 0) __builtin_amdgcn_s_setprio(3);                      // the recurrence is the critical path of the block
    int crow = 0;                          // what the forward table says about the state carried at k+1 (its slot, or its position)
    double Lc = 0.0, q1 = 0.0, q0 = 0.0;   // its likelihood, Lc / T[k+1], Lc / T[k]
    if (chainer) {
        const SwapPre top = topr[lane];
        crow = top.row; Lc = top.L; q1 = -top.a; q0 = top.c;
    }
    // The ring holds three batches: while the recurrence works through batch b out of one register set it reads batch b + 1
    // (made during batch b - 1) into the other, and the makers fill the slot of batch b + 2 (last read during batch b - 2).
    struct Batch { SwapPre R[SW]; double T[SW]; };
    auto fetch = [&](int b, Batch &B) {
        const int k0 = n - 2 - b * SW;
        const SwapPre *rb = ring + (size_t)(b % 3) * SW * wpb + lane;
#pragma unroll
        for (int j = 0; j < SW; ++j) {
            const int kk = k0 - j > 0 ? k0 - j : 0;
            B.R[j] = rb[(size_t)(k0 - j >= 0 ? j : 0) * wpb];
            B.T[j] = src.ladder[kk > 0 ? kk - 1 : 0];                  // T[k-1] (uniform: a scalar load)
        }
    };
    auto chain = [&](int b, const Batch &B) {
        const int k0 = n - 2 - b * SW;
#pragma unroll
        for (int j = 0; j < SW; ++j) {
            const int k = k0 - j;
            if (k < 0) break;
            const double spec = Lc / B.T[j];     // Lc / T[k-1]: needed if this pair accepts; does not wait for its decision
            double la = B.R[j].a;                // -L[k] / T[k]
            la += -q1;                           // -Lc / T[k+1]
            la += q0;                            //  Lc / T[k]
            la += B.R[j].b;                      //  L[k] / T[k+1]
            const bool acc = (parity < 0 || (k & 1) == parity) && B.R[j].lu <= la;     // log u <= sum
            fw[k + 1] = acc ? B.R[j].row : crow; // position k+1 is final: it keeps the carried state, or takes position k's
            lf[k] = acc ? 1 : 0;
            q1 = acc ? q0 : -B.R[j].a;
            q0 = acc ? spec : B.R[j].c;
            Lc = acc ? Lc : B.R[j].L;
            crow = acc ? crow : B.R[j].row;
        }
    };
    auto turn = [&](int b, Batch &cur, Batch &nxt) {                   // one batch: every wave passes here, one barrier
        if (wave == 0) {
            if (chainer) {
                if (b + 1 < NB) fetch(b + 1, nxt);
                chain(b, cur);
            }
        } else if (wave != 4 && b + 2 < NB) {                          // wave 4 shares the recurrence's SIMD: it sits the batches out
            produce(b + 2, wave < 4 ? 64 : 128, SWF_BLK - 128);
        }
        __syncthreads();
    };
    Batch A, B;
    if (chainer && NB > 0) fetch(0, A);
    for (int b = 0; b < NB; b += 2) {
        turn(b, A, B);
        if (b + 1 < NB) turn(b + 1, B, A);
    }
    if (chainer) fw[0] = crow;
    __syncthreads();
    // write-out: a wave per walker, the lanes along the position (as swap_sweep_kernel<true>)
    int32_t *g0 = fused ? slot_of : map, *g1 = fused ? temp_of : inv;
    const int nw = W - w0 < wpb ? W - w0 : wpb;
    bool far = false;
    for (int wl = wave; wl < nw; wl += SWF_BLK / 64) {
        const size_t row = (size_t)(w0 + wl) * n;
        for (int k = lane; k < n; k += 64) {
            const int f = sw_lds[(size_t)wl * ld + k];
            g0[row + k] = f;
            g1[row + f] = k;                                           // the inverse table: a scatter inside the walker's own row
            if (hop_nt > 0) { const int hop = blk[f] - blk[k]; far = far || hop > 1 || hop < -1; }
            if (k < n - 1 && k >= local0 && k < local0 + nlocal && sw_lds[(size_t)(wpb + wl) * ld + k])
                atomicAdd((unsigned long long *)&nswap[row + k], 1ull);
        }
    }
    if (hop_nt > 0 && __ballot(far) != 0 && lane == 0) atomicOr(hop_flag, 1);   // once per wave at most
    if (amr.AM != nullptr) {                                           // the rows now at rank 0 into the AM ring (as swap_sweep_kernel<true>)
        constexpr int NB6 = 6;
        const int tot = nw * amr.d, ringrow = (int)(amr.iter % amr.cov_update);
        for (int base = tid; base < tot; base += SWF_BLK * NB6) {
            double v[NB6];
            size_t dst[NB6];
#pragma unroll
            for (int u = 0; u < NB6; ++u) {
                const int idx = base + SWF_BLK * u, ic = idx < tot ? idx : tot - 1;
                const int wl = ic / amr.d, i = ic % amr.d;
                const size_t r = (size_t)(w0 + wl) * n + (size_t)sw_lds[(size_t)wl * ld];
                v[u] = amr.X[r * amr.d + i];
                dst[u] = ((size_t)(w0 + wl) * amr.cov_update + (size_t)ringrow) * amr.d + (size_t)am_pos(i, amr.am_epl);
            }
#pragma unroll
            for (int u = 0; u < NB6; ++u)
                if (base + SWF_BLK * u < tot) amr.AM[dst[u]] = v[u];
        }
        if (amr.AMaux)
            for (int wl = tid; wl < nw; wl += SWF_BLK) {
                const size_t r = (size_t)(w0 + wl) * n + (size_t)sw_lds[(size_t)wl * ld];
                const size_t arow = (size_t)(w0 + wl) * amr.cov_update + (size_t)ringrow;
                amr.AMaux[arow * 2] = amr.lnL[r];
                amr.AMaux[arow * 2 + 1] = amr.lp[r];
            }
        swap_am_key(amr, w0, nw, tid, SWF_BLK);
    }
}

// Odd/even mode with the whole ladder local: one thread per (walker, tried pair), the slot tables rewritten in place
// (the pairs are disjoint).  The pair test is the sweep's, term by term.
__global__ void swap_oddeven_kernel(int W, int n, const double *ladder, const double *lnL_rows, int32_t *slot_of,
                                    int32_t *temp_of, u64 *nswap, long long iter, u64 seed, int walker0, int parity)
{
    const int npairs = (n - parity) / 2;                    // k = parity, parity + 2, ... <= n - 2
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)npairs * W) return;
    const int w = (int)(idx / npairs), k = parity + 2 * (int)(idx % npairs);
    int32_t *so = slot_of + (size_t)w * n, *to = temp_of + (size_t)w * n;
    const int rk = so[k], rk1 = so[k + 1];
    const double Lk = lnL_rows[(size_t)w * n + rk], Lk1 = lnL_rows[(size_t)w * n + rk1];
    const u32 sid = (u32)((u64)(walker0 + w) * (u32)n + 0u);
    u64 w0, w1;
    philox_words(seed, (u64)iter, sid, SLOT_SWAP + (u32)k, w0, w1);
    const double Tk = ladder[k], Tk1 = ladder[k + 1];
    double la = -Lk / Tk;
    la += -Lk1 / Tk1;
    la += Lk1 / Tk;
    la += Lk / Tk1;
    if (det_log(w2uniform(w0)) <= la) {
        so[k] = rk1;
        so[k + 1] = rk;
        to[rk1] = k;
        to[rk] = k + 1;
        nswap[(size_t)w * n + k] += 1;
    }
}

// AM-buffer row of a swap iteration: the state that now sits at rank 0 (PT:624-627, 327-328)
__global__ void am_write_kernel(const double *X, const double *lnL, const double *lp, const int32_t *slot_of, double *AM,
                                double *AMaux, int W, int nt, int d, int cov_update, long long iter, int am_epl, AmFlag *AMflag)
{
    const int w = (int)blockIdx.x;
    const size_t r = (size_t)w * nt + slot_of[(size_t)w * nt];
    const double *row = X + r * d;
    double *am = AM + ((size_t)w * cov_update + (size_t)(iter % cov_update)) * d;
    for (int i = (int)threadIdx.x; i < d; i += (int)blockDim.x) am[am_pos(i, am_epl)] = row[i];
    if (AMaux && threadIdx.x == 0) {
        double *ax = AMaux + ((size_t)w * cov_update + (size_t)(iter % cov_update)) * 2;
        ax[0] = lnL[r];
        ax[1] = lp[r];
    }
    if (AMflag && threadIdx.x == 0) AMflag[(size_t)w * cov_update + (size_t)(iter % cov_update)] = AMROW_KEY;
}

extern "C" {

int ptmi_swap_write_am(ptmi_handle h, int64_t iter)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    if (h->cfg.temp0 != 0 || !h->buf.AM) return PTMI_OK;
    hipLaunchKernelGGL(am_write_kernel, dim3(h->cfg.nwalkers), dim3(64), 0, h->stream, (const double *)h->buf.X,
                       (const double *)h->buf.lnL, (const double *)h->buf.lp, (const int32_t *)h->buf.slot_of, h->buf.AM,
                       h->buf.AMaux, h->cfg.nwalkers, h->cfg.ntemps, h->cfg.ndim, h->cfg.cov_update, (long long)iter, am_row_epl(h->G, h->EPL),
                       (AmFlag *)h->buf.AMflag);
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

// odd/even mode: swap epoch e = iter / tskip tries the pairs (k, k+1) with k = e (mod 2)
static int swap_parity(const ptmi_config &c, int64_t iter)
{
    return (int)((c.tskip > 0 ? iter / c.tskip : iter) & 1);
}

// what ptmi_last_swap_launch reports
static void swap_report(ptmi_engine *h, int kernel, int wpb, size_t lds, bool hop)
{
    h->swap_last[0] = kernel; h->swap_last[1] = wpb; h->swap_last[2] = (int)lds; h->swap_last[3] = hop ? 1 : 0;
}

static int launch_swap_sweep(ptmi_engine *h, int W, int n, const SwapPre *pre, int32_t *slot_of, int32_t *temp_of,
                             int32_t *map, u64 *nswap, int local0, int nlocal, int parity, int32_t *inv, int hop_nt = 0, bool *hop_done = nullptr,
                             const SwapAmRow *amr = nullptr, bool *am_done = nullptr)
{
    if (hop_done) *hop_done = false;
    if (am_done) *am_done = false;
    SwapAmRow none = {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, 0, 0, nullptr};
    int wpb = 64;                                                      // 2 tables of wpb x (n + 1) ints must fit the CU's LDS
    while (wpb > 8 && sizeof(int32_t) * (2 * (size_t)wpb * (size_t)(n + 1) + n) > 160 * 1024) wpb /= 2;
    const size_t lds = sizeof(int32_t) * (2 * (size_t)wpb * (size_t)(n + 1) + n);      // forward table, flags, block of a position
    if (lds <= 160 * 1024) {
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void *)swap_sweep_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return fail(PTMI_EHIP, "hipFuncSetAttribute(%zu B of LDS): %s", lds, hipGetErrorString(e));
        }
        if (hop_nt > 0) {                                              // the multi-hop scan rides on the write-out
            HIPCHK(hipMemsetAsync(h->d_hop, 0, sizeof(int32_t), h->stream));
            if (hop_done) *hop_done = true;
        }
        const bool with_am = amr != nullptr && slot_of != nullptr;
        hipLaunchKernelGGL(swap_sweep_kernel<true>, dim3((unsigned)((W + wpb - 1) / wpb)), dim3(256), lds, h->stream, W, n, h->d_ladder, pre,
                           slot_of, temp_of, map, nswap, local0, nlocal, parity, inv, wpb, hop_nt, h->d_hop, with_am ? *amr : none);
        if (am_done) *am_done = with_am;
        swap_report(h, PTMI_SWL_LDS, wpb, lds, hop_nt > 0);
    } else {
        hipLaunchKernelGGL(swap_sweep_kernel<false>, dim3((unsigned)((W + 63) / 64)), dim3(64), 0, h->stream, W, n, h->d_ladder, pre,
                           slot_of, temp_of, map, nswap, local0, nlocal, parity, inv, 64, 0, (int32_t *)nullptr, none);
        swap_report(h, PTMI_SWL_DIRECT, 64, 0, false);
    }
    return PTMI_OK;
}

// The sweep with its records made in the block (swap_fused_kernel) when its tables and the ring fit the LDS; *used says whether it
// was launched (else the caller runs swap_prepare_kernel + swap_sweep_kernel).  PTMI_SWAP_FUSED=0: the two-kernel form (a
// test hook, same results).
static int launch_swap_fused(ptmi_engine *h, int W, int n, const SwapSrc &src, int32_t *slot_of, int32_t *temp_of, int32_t *map, u64 *nswap,
                             int local0, int nlocal, int parity, int32_t *inv, int hop_nt, bool *hop_done, const SwapAmRow *amr, bool *am_done,
                             bool *used)
{
    *used = false;
    if (hop_done) *hop_done = false;
    if (am_done) *am_done = false;
    if (!ptmi_env("PTMI_SWAP_FUSED", 1)) return PTMI_OK;
    // walkers per block: 16 puts the 4096 walkers of config 2 on every CU (64 per block ran on 64 CUs: 31 -> 24 us per swap epoch
    // at 64 ranks; 8 starve the producers: 38); long ladders are cut further by the LDS their tables need
    int wpb = 64, lg = 6;
    const int want = n <= 128 ? 16 : 32;                           // 256 ranks: 94 us with 32 or 64, 104 with 16
    while (wpb > 8 && wpb > want) { wpb /= 2; --lg; }
    while (wpb > 8 && swf_lds_bytes(wpb, n) > 160 * 1024) { wpb /= 2; --lg; }
    const size_t lds = swf_lds_bytes(wpb, n);
    if (lds > 160 * 1024) return PTMI_OK;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)swap_fused_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return fail(PTMI_EHIP, "hipFuncSetAttribute(%zu B of LDS): %s", lds, hipGetErrorString(e));
    }
    if (hop_nt > 0) {                                              // the multi-hop scan rides on the write-out
        HIPCHK(hipMemsetAsync(h->d_hop, 0, sizeof(int32_t), h->stream));
        if (hop_done) *hop_done = true;
    }
    const SwapAmRow none = {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, 0, 0, nullptr};
    const bool with_am = amr != nullptr && slot_of != nullptr;
    hipLaunchKernelGGL(swap_fused_kernel, dim3((unsigned)((W + wpb - 1) / wpb)), dim3(SWF_BLK), lds, h->stream, W, n, src, slot_of, temp_of, map,
                       nswap, local0, nlocal, parity, inv, wpb, lg, hop_nt, h->d_hop, with_am ? *amr : none);
    if (am_done) *am_done = with_am;
    swap_report(h, PTMI_SWL_FUSED, wpb, lds, hop_nt > 0);
    *used = true;
    return PTMI_OK;
}

int ptmi_swap(ptmi_handle h, int64_t iter)
{
    if (!h) return fail(PTMI_EINVAL, "NULL handle");
    const ptmi_config &c = h->cfg;
    if (c.ntemps != c.ntemps_global) return fail(PTMI_EINVAL, "ptmi_swap needs the whole ladder on this GPU; use the three-piece form");
    if (!h->buf.nswap) return fail(PTMI_EINVAL, "nswap buffer missing");
    if (c.ntemps < 2) return PTMI_OK;
    const int W = c.nwalkers;
    if (c.swap_mode == PTMI_SWAP_ODDEVEN) {
        const int parity = swap_parity(c, iter);
        const long long np = (long long)W * ((c.ntemps - parity) / 2);
        if (np > 0)
            hipLaunchKernelGGL(swap_oddeven_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, h->stream, W, c.ntemps,
                               h->d_ladder, (const double *)h->buf.lnL, h->buf.slot_of, h->buf.temp_of, (u64 *)h->buf.nswap,
                               (long long)iter, c.seed, c.walker0, parity);
        swap_report(h, PTMI_SWL_ODDEVEN, 0, 0, false);
        HIPCHK(hipGetLastError());
        return ptmi_swap_write_am(h, iter);
    }
    const SwapSrc src = {h->d_ladder, (const double *)nullptr, (const double *)h->buf.lnL, (const int32_t *)h->buf.slot_of, (long long)iter, c.seed,
                         c.walker0, 0, h->rp_swap_u};
    // the sweep's write-out also stores the swap iteration's AM row (one kernel and one launch gap less per swap epoch)
    const SwapAmRow amr = {(const double *)h->buf.X, (const double *)h->buf.lnL, (const double *)h->buf.lp, h->buf.AM, h->buf.AMaux,
                           c.ndim, c.cov_update, am_row_epl(h->G, h->EPL), (long long)iter, (AmFlag *)h->buf.AMflag};
    bool am_done = false, used = false;
    if (int rc = launch_swap_fused(h, W, c.ntemps, src, h->buf.slot_of, h->buf.temp_of, (int32_t *)nullptr, (u64 *)h->buf.nswap, 0, c.ntemps, -1,
                                   (int32_t *)nullptr, 0, nullptr, (c.temp0 == 0 && h->buf.AM) ? &amr : nullptr, &am_done, &used)) return rc;
    if (used) {
        HIPCHK(hipGetLastError());
        return am_done ? PTMI_OK : ptmi_swap_write_am(h, iter);
    }
    hipLaunchKernelGGL(swap_prepare_kernel, dim3((unsigned)((W + 255) / 256), (unsigned)c.ntemps), dim3(256), 0, h->stream, W, c.ntemps, src,
                       (SwapPre *)h->d_pre);
    if (int rc = launch_swap_sweep(h, W, c.ntemps, (const SwapPre *)h->d_pre, h->buf.slot_of, h->buf.temp_of,
                                   (int32_t *)nullptr, (u64 *)h->buf.nswap, 0, c.ntemps, -1, (int32_t *)nullptr, 0, nullptr,
                                   (c.temp0 == 0 && h->buf.AM) ? &amr : nullptr, &am_done)) return rc;
    HIPCHK(hipGetLastError());
    return am_done ? PTMI_OK : ptmi_swap_write_am(h, iter);
}

int ptmi_last_swap_launch(ptmi_handle h, int32_t *kernel, int32_t *wpb, int32_t *lds_bytes, int32_t *hop_in_sweep)
{
    if (!h || !kernel || !wpb || !lds_bytes || !hop_in_sweep) return fail(PTMI_EINVAL, "NULL argument");
    *kernel = h->swap_last[0]; *wpb = h->swap_last[1]; *lds_bytes = h->swap_last[2]; *hop_in_sweep = h->swap_last[3];
    return PTMI_OK;
}

int ptmi_swap_gather_lnl(ptmi_handle h, double *out)
{
    if (!h || !out) return fail(PTMI_EINVAL, "NULL argument");
    const long long n = (long long)h->cfg.nwalkers * h->cfg.ntemps;
    hipLaunchKernelGGL(gather_lnl_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->buf.lnL,
                       h->buf.slot_of, out, n, h->cfg.ntemps);
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}

// exchange scratch: inv[W][ntg] (written by the sweep), newslot[W][T], arr_slot[nranks][W], lv_slot[2][W], lv_rank[2][W], err[1]
static size_t xint_count(const ptmi_config &c)
{
    const size_t W = (size_t)c.nwalkers, nr = (size_t)((c.ntemps_global + c.ntemps - 1) / c.ntemps);
    return W * c.ntemps_global + W * c.ntemps + nr * W + 4 * W + 1;
}
static int ensure_xint(ptmi_engine *h)
{
    if (h->d_xint) return PTMI_OK;
    HIPCHK(hipMalloc((void **)&h->d_xint, sizeof(int32_t) * xint_count(h->cfg)));
    HIPCHK(hipMemsetAsync(h->d_xint, 0, sizeof(int32_t) * xint_count(h->cfg), h->stream));
    HIPCHK(hipMalloc((void **)&h->d_hop, sizeof(int32_t)));
    HIPCHK(hipMemsetAsync(h->d_hop, 0, sizeof(int32_t), h->stream));
    HIPCHK(hipHostMalloc((void **)&h->h_hop, sizeof(int32_t), hipHostMallocDefault));
    *h->h_hop = 0;
    HIPCHK(hipEventCreateWithFlags(&h->hop_ev, hipEventDisableTiming));
    return PTMI_OK;
}

static int sweep_global(ptmi_handle h, int64_t iter, const double *lnL, int32_t *map, int block_nt)
{
    if (!h || !lnL || !map) return fail(PTMI_EINVAL, "NULL argument");
    if (!h->buf.nswap) return fail(PTMI_EINVAL, "nswap buffer missing");
    const ptmi_config &c = h->cfg;
    const int W = c.nwalkers;
    if (int rc = ensure_xint(h)) return rc;
    const SwapSrc src = {h->d_ladder, lnL, (const double *)nullptr, (const int32_t *)nullptr, (long long)iter, c.seed, c.walker0, block_nt, h->rp_swap_u};
    const int parity = c.swap_mode == PTMI_SWAP_ODDEVEN ? swap_parity(c, iter) : -1;
    bool used = false;
    if (int rc = launch_swap_fused(h, W, c.ntemps_global, src, (int32_t *)nullptr, (int32_t *)nullptr, map, (u64 *)h->buf.nswap, c.temp0, c.ntemps,
                                   parity, h->d_xint /* inv[W][ntemps_global] */, block_nt, &h->hop_from_sweep, nullptr, nullptr, &used)) return rc;
    if (used) {
        HIPCHK(hipGetLastError());
        return PTMI_OK;
    }
    hipLaunchKernelGGL(swap_prepare_kernel, dim3((unsigned)((W + 255) / 256), (unsigned)c.ntemps_global), dim3(256), 0, h->stream, W, c.ntemps_global,
                       src, (SwapPre *)h->d_pre);
    if (int rc = launch_swap_sweep(h, W, c.ntemps_global, (const SwapPre *)h->d_pre, (int32_t *)nullptr,
                                   (int32_t *)nullptr, map, (u64 *)h->buf.nswap, c.temp0, c.ntemps,
                                   c.swap_mode == PTMI_SWAP_ODDEVEN ? swap_parity(c, iter) : -1, h->d_xint /* inv[W][ntemps_global] */,
                                   block_nt, &h->hop_from_sweep)) return rc;
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}
int ptmi_swap_sweep(ptmi_handle h, int64_t iter, const double *lnL_pos_global, int32_t *map)
{
    return sweep_global(h, iter, lnL_pos_global, map, 0);
}
int ptmi_swap_sweep_blocks(ptmi_handle h, int64_t iter, const double *lnL_blocks, int32_t *map)
{
    if (h && h->cfg.ntemps_global % h->cfg.ntemps) return fail(PTMI_EINVAL, "the ladder is not a whole number of blocks");
    return sweep_global(h, iter, lnL_blocks, map, h ? h->cfg.ntemps : 0);
}

// ---- device-side exchange of the rows that cross a block edge --------------------------------------------------
// One wave per walker, one lane per local position.  From the global map and its inverse (both written by the sweep)
// it (1) lists this block's leaving rows (local source, remote destination) and arriving rows (local destination,
// remote source), both in ascending local position -- the k-th arrival takes the slot the k-th departure frees, the
// rule of sharded.py's plan_exchange -- and (2) rewrites slot_of / temp_of.  A hot -> cold sweep moves at most one
// row of a walker down out of a block (the carried state) and at most one up (displaced by one level), hence the
// fixed [2][W] / [nranks][W] tables.  The work is O(local ranks), whatever the length of the whole ladder.
__global__ __launch_bounds__(256) void exchange_plan_kernel(int W, int nt, int ntg, int temp0, int nranks, const int32_t *map,
                                                            int32_t *slot_of, int32_t *temp_of, const int32_t *inv, int32_t *newslot,
                                                            int32_t *arr_slot, int32_t *lv_slot, int32_t *lv_rank, int32_t *err)
{
    const int lane = (int)(threadIdx.x & 63);
    const int w = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (w >= W) return;
    const int me = temp0 / nt;
    const int32_t *m = map + (size_t)w * ntg + temp0, *iv = inv + (size_t)w * ntg + temp0;
    int32_t *so = slot_of + (size_t)w * nt, *to = temp_of + (size_t)w * nt, *ns = newslot + (size_t)w * nt;
    const u64 lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));            // lanes below this one
    for (int q = lane; q < nranks; q += 64) arr_slot[(size_t)q * W + w] = -1;
    // departures, ascending local position
    int nlv = 0, freed0 = -1, freed1 = -1, lq0 = -1, lq1 = -1;
    for (int base = 0; base < nt; base += 64) {
        const int p = base + lane;
        const bool valid = p < nt;
        const int q = valid ? iv[p] / nt : me;
        const int slot = valid ? so[p] : -1;
        const bool leaving = valid && q != me;
        u64 mask = __ballot(leaving);
        while (mask) {
            const int l = __builtin_ctzll(mask);
            const int fs = __shfl(slot, l, 64), fq = __shfl(q, l, 64);
            if (nlv == 0) { freed0 = fs; lq0 = fq; }
            else if (nlv == 1) { freed1 = fs; lq1 = fq; }
            ++nlv;
            mask &= mask - 1;
        }
    }
    // arrivals, ascending local position; rows that stay keep their slot
    int narr = 0, aq0 = -1;
    bool bad = nlv > 2 || (nlv == 2 && lq0 == lq1);                       // two destinations on one GPU would collide in send[q][w]
    for (int base = 0; base < nt; base += 64) {
        const int j = base + lane;
        const bool valid = j < nt;
        const int src = valid ? m[j] : temp0;
        const int q = src / nt;
        const bool arriving = valid && q != me;
        const u64 mask = __ballot(arriving);
        const int rank = narr + __builtin_popcountll(mask & lt);
        if (valid) {
            int slot;
            if (!arriving) slot = so[src - temp0];
            else {
                slot = rank == 0 ? freed0 : (rank == 1 ? freed1 : -1);
                if (slot >= 0) arr_slot[(size_t)q * W + w] = slot;
                else { bad = true; slot = 0; }
            }
            ns[j] = slot;
        }
        if (mask) {                                                       // two arrivals from one GPU would collide in recv[q][w]
            const int l0 = __builtin_ctzll(mask);
            const int q0 = __shfl(q, l0, 64);
            if (narr == 0) aq0 = q0;
            else if (q0 == aq0) bad = true;
            const u64 rest = mask & (mask - 1);
            if (rest) {
                const int q1 = __shfl(q, __builtin_ctzll(rest), 64);
                if (q1 == aq0) bad = true;
            }
        }
        narr += __builtin_popcountll(mask);
    }
    if (narr != nlv) bad = true;
    if (lane == 0) {                                                      // -1 = no such departure
        lv_slot[w] = freed0; lv_rank[w] = lq0;
        lv_slot[W + w] = freed1; lv_rank[W + w] = lq1;
    }
    if (__any(bad) && lane == 0) atomicAdd(err, 1);
    for (int base = 0; base < nt; base += 64) {
        const int j = base + lane;
        if (j < nt) { const int sl = ns[j]; so[j] = sl; to[sl] = j; }
    }
}
__global__ void exchange_pack_kernel(int W, int nt, int d, const double *X, const double *lnL, const double *lp,
                                     const int32_t *lv_slot, const int32_t *lv_rank, double *send)
{
    const int w = (int)blockIdx.x, k = (int)blockIdx.y;
    const int slot = lv_slot[(size_t)k * W + w];
    if (slot < 0) return;
    const size_t r = (size_t)w * nt + slot;
    double *dst = send + ((size_t)lv_rank[(size_t)k * W + w] * W + w) * (d + 2);
    for (int i = (int)threadIdx.x; i < d; i += (int)blockDim.x) dst[i] = X[r * d + i];
    if (threadIdx.x == 0) { dst[d] = lnL[r]; dst[d + 1] = lp[r]; }
}
// a block per walker looks through the source GPUs (at most two of them sent a row): a block per (walker, GPU) was 32 768
// blocks at eight GPUs, nearly all of which found nothing
__global__ void exchange_apply_kernel(int W, int nt, int d, double *X, double *lnL, double *lp, const int32_t *arr_slot,
                                      const double *recv, int nranks)
{
    const int w = (int)blockIdx.x;
    for (int q = 0; q < nranks; ++q) {
        const int slot = arr_slot[(size_t)q * W + w];
        if (slot < 0) continue;
        const size_t r = (size_t)w * nt + slot;
        const double *src = recv + ((size_t)q * W + w) * (d + 2);
        for (int i = (int)threadIdx.x; i < d; i += (int)blockDim.x) X[r * d + i] = src[i];
        if (threadIdx.x == 0) { lnL[r] = src[d]; lp[r] = src[d + 1]; }
    }
}


// A row travels further than to a neighbouring block when the carried state of the sweep wins every pair of a whole
// block.  Every GPU scans the whole map (identical everywhere), so all of them take the same decision on the transport.
__global__ void exchange_multihop_kernel(int W, int ntg, int nt, const int32_t *map, int32_t *flag)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)W * ntg) return;
    const int j = (int)(idx % ntg);
    const int hop = map[idx] / nt - j / nt;
    if (hop > 1 || hop < -1) atomicOr(flag, 1);
}

int ptmi_exchange_pack(ptmi_handle h, const int32_t *map, double *send)
{
    if (!h || !map || !send) return fail(PTMI_EINVAL, "NULL argument");
    const ptmi_config &c = h->cfg;
    if (c.ntemps_global % c.ntemps) return fail(PTMI_EINVAL, "the ladder is not a whole number of blocks");
    const int W = c.nwalkers, nr = c.ntemps_global / c.ntemps;
    if (int rc = ensure_xint(h)) return rc;
    int32_t *inv = h->d_xint, *newslot = inv + (size_t)W * c.ntemps_global, *arr = newslot + (size_t)W * c.ntemps;
    int32_t *lvs = arr + (size_t)nr * W, *lvr = lvs + 2 * (size_t)W, *err = lvr + 2 * (size_t)W;
    hipLaunchKernelGGL(exchange_plan_kernel, dim3((W + 3) / 4), dim3(256), 0, h->stream, W, c.ntemps, c.ntemps_global, c.temp0, nr,
                       map, h->buf.slot_of, h->buf.temp_of, (const int32_t *)inv, newslot, arr, lvs, lvr, err);
    hipLaunchKernelGGL(exchange_pack_kernel, dim3(W, 2), dim3(64), 0, h->stream, W, c.ntemps, c.ndim, (const double *)h->buf.X,
                       (const double *)h->buf.lnL, (const double *)h->buf.lp, (const int32_t *)lvs, (const int32_t *)lvr, send);
    if (!h->hop_from_sweep) {                                          // the sweep's write-out did not look (tables beyond the LDS)
        HIPCHK(hipMemsetAsync(h->d_hop, 0, sizeof(int32_t), h->stream));
        const long long tot = (long long)W * c.ntemps_global;
        hipLaunchKernelGGL(exchange_multihop_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, W, c.ntemps_global, c.ntemps,
                           map, h->d_hop);
    }
    h->hop_from_sweep = false;
    HIPCHK(hipGetLastError());
    // the flag sets out for the host now, with an event of its own: ptmi_exchange_multihop waits for these four bytes, not for
    // whatever the caller has queued behind the pack step in the meantime (the neighbour exchange)
    HIPCHK(hipMemcpyAsync(h->h_hop, h->d_hop, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipEventRecord(h->hop_ev, h->stream));
    h->hop_pending = true;
    return PTMI_OK;
}
int ptmi_exchange_multihop(ptmi_handle h, int32_t *flag)
{
    if (!h || !flag) return fail(PTMI_EINVAL, "NULL argument");
    *flag = 0;
    if (!h->d_hop) return PTMI_OK;
    if (h->hop_pending) {
        HIPCHK(hipEventSynchronize(h->hop_ev));
        h->hop_pending = false;
    }
    *flag = *h->h_hop;
    return PTMI_OK;
}
int ptmi_exchange_apply(ptmi_handle h, const double *recv)
{
    if (!h || !recv) return fail(PTMI_EINVAL, "NULL argument");
    if (!h->d_xint) return fail(PTMI_EINVAL, "ptmi_exchange_apply without a preceding ptmi_exchange_pack");
    const ptmi_config &c = h->cfg;
    const int W = c.nwalkers, nr = c.ntemps_global / c.ntemps;
    const int32_t *arr = h->d_xint + (size_t)W * c.ntemps_global + (size_t)W * c.ntemps;
    hipLaunchKernelGGL(exchange_apply_kernel, dim3(W), dim3(64), 0, h->stream, W, c.ntemps, c.ndim, h->buf.X, h->buf.lnL,
                       h->buf.lp, arr, recv, nr);
    HIPCHK(hipGetLastError());
    return PTMI_OK;
}
int ptmi_exchange_status(ptmi_handle h, int32_t *violations)
{
    if (!h || !violations) return fail(PTMI_EINVAL, "NULL argument");
    *violations = 0;
    if (!h->d_xint) return PTMI_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(violations, h->d_xint + xint_count(h->cfg) - 1, sizeof(int32_t), hipMemcpyDeviceToHost));
    return PTMI_OK;
}

}  // extern "C"
