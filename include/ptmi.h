/*
 * ptmi.h -- C ABI of libptmi.so, the MI355X (gfx950) engine behind the
 * Metropolis-Hastings inner loop of a PTSampler-compatible parallel-tempering
 * sampler.
 *
 * The reference (nanograv/PTMCMCSampler) has no FFI: its hot path is the Python
 * method PTSampler.PTMCMCOneStep (PTMCMCSampler/PTMCMCSampler.py:530-629) plus
 * PTswap (:631-697), _updateRecursive (:769-803) and _updateDEbuffer (:806-817),
 * one chain per MPI rank.  Each entry point below names the reference code it
 * replaces.  The binding a maintainer would add is a ctypes stub: see
 * INTEGRATION.md and ptmcmcsampler_amd/_lib.py.
 *
 * Conventions
 *   - every call returns 0 on success, a negative PTMI_E* code otherwise; the
 *     message is available from ptmi_last_error() (thread-local);
 *   - no C++ exception crosses this boundary;
 *   - every pointer in ptmi_buffers is DEVICE memory owned by the caller (e.g. a
 *     torch-ROCm tensor's data_ptr(), or ptmi_malloc); pointers in ptmi_config
 *     are HOST memory, copied at create time;
 *   - all arrays are C-contiguous; state rows are float64;
 *   - kernels run asynchronously on the stream given at create time; a handle is
 *     not thread-safe, different handles are independent.
 *
 * Layout ("slots and ranks"): a walker is an independent replica of the whole
 * reference run; it has `ntemps` chains.  State rows never move inside a GPU:
 * row (w, s) -- walker w, SLOT s -- holds whichever state currently sits at
 * temperature RANK temp_of[w][s]; slot_of is the inverse table.  A PT swap only
 * rewrites the two tables.  Per-rank quantities (RNG stream, counters) are
 * indexed by rank, exactly as they belong to an MPI rank in the reference.
 */
#ifndef PTMI_H
#define PTMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_VERSION 1

enum { PTMI_OK = 0, PTMI_EINVAL = -1, PTMI_EHIP = -2, PTMI_EUNSUPPORTED = -3, PTMI_ENODEVICE = -4 };

/* built-in device likelihoods / priors (a Python callback cannot run in a kernel;
 * user callbacks go through ptmi_propose / ptmi_accept instead) */
enum { PTMI_LOGL_ISO = 0,      /* -1/2 sum x^2 */
       PTMI_LOGL_DENSE = 1,    /* -(x-mu)^T P (x-mu) / 2 ; par = mu[d], Pt[d*d] (Pt[j*d+i] = P[i][j]).  P is a precision matrix:
                                * the value is summed over the lower half of its symmetric part (half the products) */
       PTMI_LOGL_CURVED = 2,   /* d/2 copies of examples/curved_likelihood.ipynb's 2-d likelihood */
       PTMI_LOGL_INTERVAL = 3 }; /* the reference's own NUTS workload (tests/test_nuts.py:13-47 GaussianLikelihood inside :50-140 intervalTransform):
                                * N(0, I) on the box (a, b) in the coordinates p of all real numbers, x = (b - a) e^p / (1 + e^p) + a, the
                                * log-Jacobian included: sum_i -x_i^2/2 - log(2 pi)/2 + log(b_i - a_i) + p_i - 2 log(1 + e^p_i);
                                * par = a[d], w[d] = b - a, lw[d] = log w (the host's logarithm: a parameter, not part of the arithmetic).
                                * Served by the fused kernels' shapes of the gradient jumps (ndim <= 512: at most 8 slots per lane) with or without them. */
enum { PTMI_LOGP_FLAT = 0,     /* 0 everywhere */
       PTMI_LOGP_BOX = 1 };    /* 0 inside [lo,hi], -inf outside ; par = lo[d], hi[d] */

/* proposal types; also the index into jstat */
enum { PTMI_J_SCAM = 0, PTMI_J_AM = 1, PTMI_J_DE = 2, PTMI_J_NUTS = 3, PTMI_J_HMC = 4, PTMI_J_NTYPES = 5 };

/* ptmi_config.swap_mode.  SWEEP is PTswap as the reference runs it: every adjacent pair is tried, hottest first, and
 * a state can travel several ranks in one call.  ODDEVEN tries, at swap epoch e = iter / tskip, only the pairs
 * (k, k+1) with k = e (mod 2): the pairs are disjoint, so all of them are decided at once on the device and a
 * sharded ladder moves at most one row per walker across each block edge.  Same pair test, same uniform (the one the
 * sweep would have used for pair k); it is a different, equally valid, Markov kernel -- not a replica of a
 * reference run. */
enum { PTMI_SWAP_SWEEP = 0, PTMI_SWAP_ODDEVEN = 1 };

/* ptmi_config.pick_mode: who draws the entry of the proposal cycle (_jump, PTMCMCSampler.py:1058).  CHAIN: every chain
 * draws its own from its rank's stream, as every MPI rank of the reference does -- a walker is then a replica of a
 * reference run.  WALKER: one draw per (walker, iteration), taken from the stream of the walker's rank 0, decides the
 * proposal TYPE for all temperature ranks of the walker (everything else -- group, scale branch, direction, normals,
 * accept uniform -- stays per chain).  The choice is independent of the state, so every chain still runs a valid
 * Metropolis-Hastings kernel with the same mixture weights; on the device the proposal type becomes wave-uniform
 * (no divergence, the matrix-core AM product runs only on AM steps).  Not a replica of a reference run. */
enum { PTMI_PICK_CHAIN = 0, PTMI_PICK_WALKER = 1 };

typedef struct ptmi_config {
    int32_t ndim;            /* parameters per chain */
    int32_t ntemps;          /* temperature ranks held by THIS handle (a contiguous block) */
    int32_t nwalkers;        /* walkers held by this handle */
    int32_t ntemps_global;   /* ranks in the whole ladder (== ntemps on one GPU) */
    int32_t temp0;           /* first global rank of this block */
    int32_t walker0;         /* first global walker index (RNG stream ids are global) */
    int32_t logl_kind, logp_kind;
    int32_t w_host;          /* cycle entries served by host callbacks (custom / gradient jumps added with
                              * addProposalToCycle before SCAM/AM, :988-1014); split path only, 0 for the fused kernel */
    int32_t w_scam, w_am, w_de;   /* proposal-cycle weights, PTMCMCSampler.py:261-264, 579-585 */
    int32_t de_size;         /* rows of a DE buffer (= burn, :221) */
    int32_t cov_update;      /* rows of an AM buffer (= covUpdate, :220) */
    int32_t tskip;           /* swap period (:624); 0 = never */
    int32_t cov_per_walker;  /* 1: Ut/S/DE/cov per walker (faithful replicas); 0: one pooled set */
    int32_t device;          /* HIP device ordinal */
    int32_t ngroups;         /* parameter groups (PTMCMCSampler.py:129-145); 0 or 1 = one group of all parameters */
    int32_t swap_mode;       /* PTMI_SWAP_SWEEP (the reference's hot -> cold sweep, :666-686) or PTMI_SWAP_ODDEVEN */
    /* Gradient jumps on the built-in likelihoods (the reference adds them when logl_grad / logp_grad are given,
     * :225-258; nutsjump.py): cycle += [NUTS]*w_nuts + [HMC]*w_hmc.  The engine shares a chain among ptmi_lanes_for_grad(ndim)
     * lanes, which fixes the summation orders.  ndim <= 512 (at most 8 register slots per lane) for the fused kernels (ptmi_mh_steps),
     * for NUTS and for the interval family; 512 < ndim <= 2048: w_hmc alone (w_nuts == 0) on a split handle (ptmi_buffers.Q), served by
     * ptmi_gj_begin / ptmi_gj_step with the whitening products on the matrix cores -- the proposal kernels then run in the ordinary
     * 64-lane shape and ptmi_mh_steps refuses the handle (PTMI_EUNSUPPORTED).  With parameter
     * groups (ngroups > 1; not the interval family) SCAM / AM / DE move one group's parameters with that group's tables, a NUTS or
     * HMC pick draws no group and moves every parameter with the whitening tables of the full initial covariance (gj_tab). */
    int32_t w_nuts, w_hmc;
    int32_t gj_nburn;        /* nburn of the jump objects (= burn, :227,238,251) */
    int32_t hmc_min, hmc_max;/* HMC takes randint(hmc_min, hmc_max) leapfrogs (:240-241: 2, HMCsteps) */
    int32_t nuts_maxdepth;   /* tree heights 0..nuts_maxdepth per call, <= 24.  The reference doubles without a cap
                              * (nutsjump.py:716-802): 24 (2^24 leapfrogs in one call) is never reached, i.e. its behaviour */
    int32_t pick_mode;       /* PTMI_PICK_CHAIN or PTMI_PICK_WALKER (below) */
    double hmc_eps;          /* HMCstepsize (:239) */
    double nuts_delta;       /* target acceptance of NUTS' dual averaging (0.6, :256) */
    uint64_t seed;
    void *stream;            /* hipStream_t to launch on; NULL = the null stream */
    const double *ladder;    /* host [ntemps_global]  temperatures used by the swap (:658) */
    const double *temps_mh;  /* host [ntemps] temperature each local rank samples at (:278-282; hot chain = 1e80) */
    const double *logl_par;  /* host, per logl_kind */
    int64_t logl_par_len;
    const double *logp_par;  /* host, per logp_kind */
    int64_t logp_par_len;
    const int32_t *group_size;  /* host [ngroups] parameters per group (ngroups > 1 only) */
    const double *group_mask;   /* host [ngroups][ndim] 1.0 where a parameter belongs to the group (ngroups > 1 only) */
    const double *gj_tab;       /* host [3][ndim][ndim] whitening tables of the gradient jumps from L = cholesky(cov)
                                 * (nutsjump.py:53-54), each used as out[i] = sum_k T[k][i] v[k]: backward T = L
                                 * (x = L^T q), forward T = L^-1 (q = L^-T x), gradient T = L^T.  NULL without them */
} ptmi_config;

/* Device buffers, caller-owned.  W = nwalkers, T = ntemps, d = ndim,
 * Wc = cov_per_walker ? W : 1.  Optional ones may be NULL when unused. */
typedef struct ptmi_buffers {
    double *X;          /* [W][T][d]   state rows by slot */
    double *lnL;        /* [W][T]      log-likelihood of the row in a slot */
    double *lp;         /* [W][T]      log-prior of the row in a slot */
    int32_t *temp_of;   /* [W][T]      local rank held by a slot */
    int32_t *slot_of;   /* [W][T]      slot holding a local rank */
    double *Ut;         /* [Wc][Ng][d][d]  eigenvectors, one per ROW (Ut[k][i] = U[i][k] of :145,803); Ng = max(ngroups,1);
                         *              a group's vectors are embedded in the full space (zero outside the group, zero rows
                         *              beyond its size) */
    double *S;          /* [Wc][Ng][d]  eigenvalues (zero beyond the group's size) */
    double *DE;         /* [Wc][de_size][stride]  DE history ring (optional); row format: ptmi_de_row_stride */
    double *AM;         /* [W][cov_update][d] samples of the rank-0 chain (:327-328); only where temp0 == 0; row format: ptmi_am_row_format */
    uint64_t *nacc;     /* [W][T]      accepted MH updates per rank (:621) */
    uint64_t *jstat;    /* [W][T][PTMI_J_NTYPES][2]  proposed, accepted per jump type (:602,622) */
    uint64_t *nswap;    /* [W][ntemps_global]  accepted swaps credited to the lower rank (:681) */
    double *mu;         /* [Wc][d]     running mean of the rank-0 chain (:148); pooled: of all walkers' rank-0 samples */
    double *M2;         /* [Wc][d][d]  running sum of outer products about the mean (:147) */
    double *cov;        /* [Wc][d][d]  published covariance (:794) */
    double *Q;          /* [W][T][d]   proposals, split path only (optional) */
    double *qaux;       /* [W][T][4]   split path: qxy, jump type (>= PTMI_J_NTYPES: host entry index + PTMI_J_NTYPES),
                         *              accept uniform, log(accept uniform) (optional) */
    double *AMaux;      /* [W][cov_update][2]  lnL and lp of the rank-0 chain beside each AM row: the
                         *              _lnlike/_lnprob columns of updateChains (:331-335) (optional) */
    double *gj;         /* [W][T][8]   by RANK: the attributes of a rank's NUTSJump / HMCJump object (nutsjump.py:379-433):
                         *              epsilon, mu, Hbar, epsilonbar (starts at 1), NUTS calls, HMC calls, have-epsilon flag, leapfrogs taken so far
                         *              (needed with w_nuts + w_hmc > 0) */
    uint64_t *AMflag;   /* [W][cov_update] one flag word beside every AM row (optional; ptmi_am_flags_ok): bit 0 NEW = the step was accepted,
                         *              bit 1 KEY = the row is stored whatever the step did (first step of a launch, ring rows 0 and 1, the swap's
                         *              post-swap row, rows the caller writes).  With it the step kernels store the rank-0 chain's row
                         *              (updateChains, :327-328) only when it is NEW or KEY -- a rejected proposal leaves the chain where it
                         *              was, its row repeats the one before -- and ptmi_update_cov takes every stored row once, weighted by
                         *              the length of its run.  Readers that want every row call ptmi_am_expand first.  The caller
                         *              initialises every word to KEY (2) and marks rows it writes itself as KEY */
    double *Q2;         /* [W][T][d]   a SECOND proposal buffer (optional, with sloc): ptmi_accept_propose then writes the next proposals to
                         *              the buffer that does NOT hold the current ones (ptmi_proposals says which is which), an accepted
                         *              proposal stays where it is as the chain's state, and rows are copied to X only when their buffer
                         *              is about to be overwritten or at ptmi_accept (csrc/ptmi_split.hip) */
    int32_t *sloc;      /* [W][T]      with Q2: where a chain's state lives between ptmi_propose and ptmi_accept (0 = X, 1 = Q, 2 = Q2);
                         *              all zero outside such a span -- the caller zeroes it once */
} ptmi_buffers;

typedef struct ptmi_engine *ptmi_handle;

const char *ptmi_last_error(void);
int ptmi_version(void);
int ptmi_device_count(int *count);
/* lanes of a wavefront that share one chain for a given ndim (fixes the summation order) */
int ptmi_lanes_for(int ndim);
/* the same with gradient jumps in the cycle (w_nuts + w_hmc > 0); 0 = not supported */
int ptmi_lanes_for_grad(int ndim);

/* temperatureLadder (PTMCMCSampler.py:699-720), host arithmetic: out[i] = Tmin * tstep^i, i < nchain, with
 * tstep = the argument if > 0, else exp(log(Tmax/Tmin)/(nchain-1)) if Tmax > 0, else 1 + sqrt(2/ndim); a single chain
 * gets {1}.  `out` is HOST memory [nchain]. */
int ptmi_temperature_ladder(int nchain, int ndim, double Tmin, double Tmax, double tstep, double *out);

/* Row format of the DE buffer for a given ndim (grad != 0: with gradient jumps in the cycle): *stride doubles per row;
 * *epl == 0: a row holds the parameters in order (stride == ndim); *epl > 0 (4 lanes per chain, *epl slots per lane): the
 * row is dealt to the lanes in 16-byte pieces, row[8 * (e / 2) + 2 * lane + e % 2] = parameter lane + 4 e (zero past ndim
 * and for e >= *epl), stride == 8 * ((*epl + 1) / 2) -- one read instruction of the kernel takes 64 contiguous bytes per chain. */
int ptmi_de_row_stride(int ndim, int grad, int *stride, int *epl);

/* Row format of the AM buffer for a given ndim (grad != 0: with gradient jumps in the cycle).  *epl == 0: a row holds the parameters
 * in order.  *epl > 0 (the exact 4-lane shape: ndim = 4 * *epl = 100): the lanes' order -- position 8 * (e / 2) + 2 * lane + e % 2
 * holds parameter lane + 4 e, the odd last slot e = *epl - 1 at 8 * (*epl / 2) + lane -- so that the rank-0 chain's four lanes store
 * their row 16 bytes at a time.  Every kernel that reads the buffer goes through the same map. */
int ptmi_am_row_format(int ndim, int grad, int *epl);

int ptmi_create(const ptmi_config *cfg, const ptmi_buffers *buf, ptmi_handle *out);
int ptmi_destroy(ptmi_handle h);
int ptmi_sync(ptmi_handle h);

/* lnL and lp of every row from X: the initial evaluation of sample(), PTMCMCSampler.py:479-487 */
int ptmi_eval_state(ptmi_handle h);

/* DE enters the proposal cycle after burn (PTMCMCSampler.py:574-585) */
int ptmi_set_de_active(ptmi_handle h, int on);

/* `nsteps` fused Metropolis-Hastings updates of every chain for iterations
 * iter0 .. iter0+nsteps-1: _jump + SCAM/AM/DE (:1048-1067, :820-985), logp/logl +
 * tempering (:605-612), the Hastings test (:615-622) and the AM-buffer write of
 * updateChains (:327-328).  The caller splits the run at swap / covariance / DE
 * epochs (none may fall strictly inside the range). */
int ptmi_mh_steps(ptmi_handle h, int64_t iter0, int32_t nsteps);

/* Which instantiation of the fused kernel the most recent ptmi_mh_steps launched (the parity tests assert that they
 * reached the one they mean to test): a combination of the flags below, plus lanes per chain in bits 12-19 and register
 * slots per lane in bits 20-27 (PTMI_VAR_UTPAD sits above them). */
enum { PTMI_VAR_STAGED = 1,    /* strided lane layout, tables in LDS, products on the f64 matrix cores */
       PTMI_VAR_FULL = 2,      /* the cycle holds AM and / or an active DE (else SCAM only) */
       PTMI_VAR_LDS_UT = 4,    /* staged: the eigenvector table is in LDS too */
       PTMI_VAR_GROUPS = 8,    /* parameter groups */
       PTMI_VAR_GRADJUMP = 16, /* the kernel with the NUTS / HMC branch */
       PTMI_VAR_UNIFORM = 32,  /* wave-uniform cycle pick (pick_mode = PTMI_PICK_WALKER) */
       PTMI_VAR_AMQ = 64,      /* staged full kernel: AM increments queued 16 at a time for the matrix cores */
       PTMI_VAR_LDS_BOX = 128, /* box prior: the bounds table is in LDS */
       PTMI_VAR_LDS_DRAWT = 256, /* the tables of the draws (log slices, base angles) are in LDS */
       PTMI_VAR_DENSE_SCAM = 512, /* mh_dense_scam_kernel: dense likelihood + SCAM-only cycle, P and Ut unpadded in LDS, 512-thread
                                  * blocks (two waves per SIMD over one copy of the tables) -- what bench.py --logl dense times */
       PTMI_VAR_PERSISTENT = 1024, /* SCAM-only cycle, one eigenvector table for the launch (pooled covariance): persistent blocks, one
                                    * per CU over one LDS copy of the table, each wave walking over units of 16 chains -- what bench.py times */
       PTMI_VAR_PC = 2048,     /* cycles with AM entries, per-chain picks: stepper and AM-producer waves paired per SIMD (mh_pc_kernel) */
       PTMI_VAR_UTPAD = 268435456 /* = 1 << 28, above the shape bits: 16- / 64-lane shapes, SCAM-only cycle, one table for the launch: wide draw batches (all lanes of a chain
                                 * draw), the direction read from the library's zero-padded copy of the table -- what bench.py --ndim 1000 times */ };
int ptmi_last_mh_variant(ptmi_handle h, int32_t *variant);

/* What the most recent gradient-jump launch of ptmi_mh_steps was (PTMI_VAR_GRADJUMP says no more than that there was one): all
 * layouts of the kernel give the same results, so only this report tells a test which one it ran.  `layout` is one of
 * PTMI_GJL_WAVE .. PTMI_GJL_CHAIN or-ed with the flags behind them, `lds_levels` the heights of the NUTS tree stack kept in LDS,
 * `lds_bytes` the dynamic LDS of a block, `nslots` the chain slots of the launch (with the launch order: the chains, the empty
 * slots beside the chains that have a wave of their own, and the last wave's padding).  All four are 0 before the first such launch. */
enum { PTMI_GJL_WAVE = 1,      /* a jump takes the whole wave, one chain at a time: the 4-lane shapes */
       PTMI_GJL_PAIR = 2,      /* 4-lane shapes, diagonal whitening, no dense likelihood: two jumps at a time, a half-wave each */
       PTMI_GJL_W16 = 3,       /* the 16-lane shape at ndim <= 64: a jump takes the whole wave, one element per lane */
       PTMI_GJL_CHAIN = 4,     /* a jump runs in the chain's own 16 or 64 lanes */
       PTMI_GJL_LAYOUT_MASK = 15,
       PTMI_GJL_DIAG = 16,     /* the whitening tables are diagonal */
       PTMI_GJL_GRP = 32,      /* the instantiation for parameter groups */
       PTMI_GJL_BOX_LDS = 64,  /* box prior: the bounds table sits behind the layout's other tables in LDS */
       PTMI_GJL_ORDERED = 128, /* chains dealt over the waves by NUTS step size (cycles with NUTS) */
       PTMI_GJL_AM_AHEAD = 256 /* the launch was a piece behind the matrix product that computes its AM increments */ };
int ptmi_last_gj_launch(ptmi_handle h, int32_t *layout, int32_t *lds_levels, int32_t *lds_bytes, int32_t *nslots);

/* Which kernels the most recent swap launched (ptmi_swap, ptmi_swap_sweep, ptmi_swap_sweep_blocks): every route gives the same
 * tables, so only this report tells a test which one it ran.  The route follows from the ladder's length alone (the tables of a
 * block's walkers must fit 160 KB of LDS), from the swap mode and from the test hook PTMI_SWAP_FUSED.  `kernel` is one of the values
 * below, `wpb` the walkers per block (0 for PTMI_SWL_ODDEVEN, whose blocks are not made of walkers), `lds_bytes` the dynamic LDS of a block, `hop_in_sweep` 1 when the sweep's write-out did the
 * multi-hop scan itself (sharded form only; with 0 ptmi_exchange_pack runs the standalone scan).  All four are 0 before the first swap. */
enum { PTMI_SWL_FUSED = 1,     /* swap_fused_kernel: the pairs' records made in the block, the tables in LDS */
       PTMI_SWL_LDS = 2,       /* swap_prepare_kernel + swap_sweep_kernel with the tables in LDS */
       PTMI_SWL_DIRECT = 3,    /* swap_prepare_kernel + swap_sweep_kernel storing straight to memory: ladders whose tables do not fit the
                                * LDS with 8 walkers per block; the AM row and the multi-hop scan are kernels of their own */
       PTMI_SWL_ODDEVEN = 4    /* odd/even mode with the whole ladder local: one thread per tried pair, no LDS */ };
int ptmi_last_swap_launch(ptmi_handle h, int32_t *kernel, int32_t *wpb, int32_t *lds_bytes, int32_t *hop_in_sweep);

/* PTswap (:631-697) for iteration `iter` when the whole ladder is on this GPU. */
int ptmi_swap(ptmi_handle h, int64_t iter);

/* The same in three pieces for a ladder sharded over GPUs (the caller all-gathers
 * lnL between 1 and 2 and exchanges the rows that cross a block edge after 2):
 *  1. lnL by local rank:  lnL_pos[w][t] = lnL[w][slot_of[w][t]]
 *  2. the sweep over the global ladder -> map[w][j] = position whose state moves to j
 *     (every GPU computes the identical map; credits go to nswap for local ranks only)
 *  3. the caller rewrites the tables and exchanges the rows that cross a block edge
 *     (ptmcmcsampler_amd/sharded.py: plan_exchange + one all-to-all), then
 *     ptmi_swap_write_am stores the AM row of the state that now sits at rank 0. */
int ptmi_swap_gather_lnl(ptmi_handle h, double *lnL_pos_local /* dev [W][T] */);
int ptmi_swap_sweep(ptmi_handle h, int64_t iter, const double *lnL_pos_global /* dev [W][ntemps_global] */,
                    int32_t *map /* dev [W][ntemps_global] */);
int ptmi_swap_write_am(ptmi_handle h, int64_t iter);

/* Device-side form of pieces 2 and 3, with no host synchronisation (what ShardedPTEngine uses on GPUs):
 *  - ptmi_swap_sweep_blocks: the sweep reading lnL exactly as an all-gather delivers it, [nranks][W][T];
 *  - ptmi_exchange_pack: rewrites slot_of / temp_of for this block from the map and copies the rows that leave
 *    into send[q][w][0..d+1] (state, lnL, lp), q = destination GPU.  One sweep moves at most one row of a walker
 *    to a colder block and at most one to the next hotter block, so [nranks][W] slots are always enough;
 *  - (caller) all-to-all with equal splits: send[q] goes to GPU q, recv[q] comes from GPU q;
 *  - ptmi_exchange_apply: stores the rows that arrived (the pack step recorded where each one goes).
 * ptmi_exchange_status reports (after a sync) whether a plan ever exceeded those bounds (must stay 0). */
int ptmi_swap_sweep_blocks(ptmi_handle h, int64_t iter, const double *lnL_blocks /* dev [nranks][W][T] */,
                           int32_t *map /* dev [W][ntemps_global] */);
int ptmi_exchange_pack(ptmi_handle h, const int32_t *map, double *send /* dev [nranks][W][d+2] */);
int ptmi_exchange_apply(ptmi_handle h, const double *recv /* dev [nranks][W][d+2] */);
int ptmi_exchange_status(ptmi_handle h, int32_t *violations);
/* After ptmi_exchange_pack: 1 if some row of the sweep moves further than to a neighbouring block (possible only when the
 * carried state wins every pair of a whole block), else 0 -- the same answer on every GPU, computed from the global map.
 * With 0 only send[rank-1] and send[rank+1] hold rows: the caller exchanges those two segments with its neighbours
 * (RCCL send/recv over one xGMI link each way) and skips the all-to-all.  The four bytes set out for (pinned) host memory at
 * the end of ptmi_exchange_pack; this call waits for THEM only (an event recorded behind the copy), not for the stream: work the
 * caller queued behind the pack step -- the neighbour exchange, which every epoch needs -- runs meanwhile. */
int ptmi_exchange_multihop(ptmi_handle h, int32_t *flag);

/* _updateRecursive (:769-794) for every walker at iteration `iter` (= the multiple of
 * cov_update just completed): updates mu, M2 and cov.  With cov_per_walker == 0 ONE set
 * (mu[0], M2[0], cov[0]) is adapted from all walkers' buffered rows: shifted sums of outer products on the matrix
 * cores, slab by slab, combined with the running statistics by Chan's formula (the sample covariance of every
 * rank-0 sample so far; oracle: orc_pool_update; with AMflag: over the stored rows, each scaled by the square root of its run
 * length, oracle: orc_pool_update_rle).  The eigendecomposition (:797-803) is a
 * separate step: on the host (LAPACK, as the reference) or ptmi_eig_jacobi. */
int ptmi_update_cov(ptmi_handle h, int64_t iter);
/* The same on `stream` (NULL: the handle's) from the ring AM / AMflag (AM NULL: the handle's; AMflag NULL with AM given: every row
 * is stored): the statistics of a covariance period that is OVER need nothing the next launches touch once those write another
 * ring, so a caller that keeps two rings (ptmi_set_am_buffers at every epoch) runs them on a side stream BESIDE the launches of
 * the next period (PTEngine stats_async; :545-560 with the table taking effect eig_lag launches late).  mu / M2 / cov and the
 * scratch are the handle's: one statistics call at a time. */
int ptmi_update_cov_on(ptmi_handle h, int64_t iter, void *stream, const double *AM, const uint64_t *AMflag);
/* The ring (updateChains' buffer, :327-328) the step kernels, the swap and ptmi_update_de use from now on: a caller with two rings
 * switches at a covariance epoch.  AMaux / AMflag exactly when the handle was created with them.  Takes effect for the calls that
 * follow (host-side pointers of the handle; nothing is queued). */
int ptmi_set_am_buffers(ptmi_handle h, double *AM, double *AMaux, uint64_t *AMflag);

/* AM row flags (ptmi_buffers.AMflag; updateChains' buffer, :327-328).  ptmi_am_flags_ok: 1 when the configuration can keep them --
 * pooled covariance, rank 0 on this GPU (the per-walker recurrence of :778-794 takes every row in turn).  ptmi_am_expand copies, in
 * the AM buffer itself, every row that was not stored from the row before it, for iterations iter_lo .. iter_hi of walkers
 * w0 .. w0 + nw - 1: what a flag-free run would have stored.  Both iterations lie in the current covariance period
 * [E, E + cov_update], E = the last multiple of cov_update below iter_hi (once the ring wraps, the stored row an older repeat hangs on
 * is overwritten; the statistics read a period when it is complete).  With AMflag a launch of ptmi_mh_steps may not cross a period. */
int ptmi_am_flags_ok(const ptmi_config *cfg);
int ptmi_am_expand(ptmi_handle h, int32_t w0, int32_t nw, int64_t iter_lo, int64_t iter_hi);

/* The eigendecomposition of _updateRecursive (:797-803, np.linalg.svd of the covariance) for every covariance the handle
 * holds (Wc matrices), on the device: Ut and S are overwritten from cov.  One-sided Jacobi, one block per matrix, both
 * tables in LDS (ndim <= 101, one parameter group); eigenvalues descending, every eigenvector (a row of Ut) with its
 * largest component positive.  Same subspaces as LAPACK, but not its column signs: a run adapted this way is not a
 * bit-replica of one adapted through the host.  Asynchronous on the handle's stream. */
int ptmi_eig_jacobi(ptmi_handle h);
/* The same by Householder tridiagonalization + implicit QL iterations (oracle: orc_eig_ql; ndim <= 1024, parameter groups included: one
 * factorization per group's block, a group may not repeat a parameter).  The choice for thousands of per-walker covariances: a
 * 100 x 100 matrix takes a quarter of the Jacobi kernel's time on the nearly degenerate spectra an isotropic target adapts to.
 * Eigenvalues in absolute value, descending; sign rule as ptmi_eig_jacobi.  Asynchronous on the handle's stream.  Two forms, the same
 * bits (a matrix here is the full covariance or a group's block):
 *  - up to 128 x 128 the matrix lives in LDS: one block of two waves per matrix, two per CU at ndim = 100; from 64 matrices on as
 *    three kernels, reduce -> the scalar chains of all matrices at once -> apply (PTMI_QL_SPLIT = 1 / 0 forces either, a test hook);
 *  - beyond, up to 1024 x 1024 (csrc/ptmi_eig_wide.hip), always as reduce -> chains -> apply with the matrix in a global scratch, the
 *    apply step tiled over matrices x rows.  The scratch is some 7 n^2 doubles per matrix (15 MB at 512, 59 MB at 1024): the
 *    matrices are factorized in batches that fit 4096 MB (at least one matrix per batch), queued one after another on the stream;
 *    results do not depend on the batch.  A matrix whose rotations do not fit the record (3 n^2) is redone with the chain and the
 *    rows together; PTMI_QL_SPLIT = 0 (the same test hook) sends every matrix that way.
 * ndim > 1024: PTMI_EUNSUPPORTED. */
int ptmi_eig_ql(ptmi_handle h);
/* ptmi_eig_ql on `stream` (NULL: the handle's), reading `cov_in` (NULL: the cov buffer) and writing `Ut_out` / `S_out` (NULL: the Ut / S
 * buffers), one parameter group: the engine's eig_lag with per-walker covariances runs the factorization of a covariance epoch
 * (:797-803) on a side stream beside the step launches that follow and puts its tables into force a fixed number of launches later
 * (oracle: OracleEngine(eig_lag=L)).  Both forms of ptmi_eig_ql, ndim <= 1024; the scratch is the handle's: one call at a time per
 * handle. */
int ptmi_eig_ql_from(ptmi_handle h, void *stream, const double *cov_in, double *Ut_out, double *S_out);
/* The same for ONE large pooled covariance (3 <= ndim <= 1024; the engine's eig_mode "sytrd"), all of it the library's own kernels:
 * Householder tridiagonalization in ONE kernel with the matrix in the LDS of its blocks (csrc/ptmi_eig.hip sytrd_lds_kernel), the
 * tridiagonal matrix's eigenvectors by divide and conquer (csrc/ptmi_dc.inc.h: QL on leaves of 16 rows, rank-one merges with
 * deflation, roots of the secular equation by bisection, Gu / Eisenstat weights), back-transformed through the reflectors.
 * Replaces the np.linalg.svd of :797-803 where the ROCm library's eigensolver (torch.linalg.eigh: 35 ms of small kernels at
 * 1000 x 1000) is the epoch.  On `stream` (NULL: the handle's), results into Ut_out [ndim][ndim] / S_out [ndim] (NULL: the handle's
 * Ut / S): eigenvalues in absolute value, descending; no sign rule.  A merge deflates by LAPACK dlaed2's test with a tolerance
 * that carries the matrix's own norm (csrc/ptmi_dc.inc.h), so the factorization commutes with a power of two times cov: the same Ut,
 * that power of two times S, bit for bit.  Its last bits are its own; what holds it: oracle/eig_dc.py restates the algorithm on the
 * CPU (tests/test_eig_dc.py, against LAPACK), tests/test_eig_dc_gpu.py drives the reduction, the tridiagonal solver and the whole
 * pipeline one by one against LAPACK and that restatement -- residual, orthogonality and eigenvalues within a measured multiple of
 * LAPACK's own, U diag(+-S) U^T = cov at 1e-12 max|cov| from 2^-300 to 2^300 times the matrix, indefinite and singular input
 * included -- and tests/test_device_tables_gpu.py steps the ORACLE's chains with the tables it makes. */
int ptmi_eig_sytrd(ptmi_handle h, void *stream, double *Ut_out, double *S_out);
/* The same from the covariance `cov_in` [ndim][ndim] (device; NULL: the handle's cov): a caller that runs the factorization BESIDE
 * later work -- the statistics of the next covariance epoch overwrite the handle's cov -- hands in its own copy (PTEngine: eig_lag
 * with the statistics of the next epoch ahead of the pending table, :545-560). */
int ptmi_eig_sytrd_from(ptmi_handle h, void *stream, const double *cov_in, double *Ut_out, double *S_out);
/* The convergence word of the most recent ptmi_eig_sytrd whose result has reached the host: 0 = converged; k > 0 = leaf k - 1 of the
 * divide-and-conquer tree did not split off an eigenvalue within 60 QL sweeps.  It
 * follows the factorization on its stream into pinned memory, so the call never waits; check it once that stream has been waited for
 * (the engine does at its next covariance epoch and in sync()).  Non-zero: Ut / S of that epoch are not to be trusted. */
int ptmi_eig_sytrd_info(ptmi_handle h, int32_t *info);
/* The stages of ptmi_eig_sytrd on their own, for tests.
 * ptmi_eig_dc_tridiag: the divide-and-conquer kernels on the caller's symmetric tridiagonal matrix, no back-transformation.  The order
 * is the handle's ndim and nothing else -- the tree of the solver is built once per handle for that order, so the call takes no
 * order of its own -- 1 <= ndim <= 1024 (1 and 2 included, below ptmi_eig_sytrd's 3).  All pointers are device memory: d
 * [ndim] the diagonal, e [ndim - 1] the off-diagonal (unused at ndim = 1), W [ndim] the eigenvalues ascending, Z [ndim][ndim] the
 * eigenvectors, vector-major (row v belongs to W[v]); cnt (may be NULL) [2 * merges]: for every merge of the tree, bottom level
 * first and left to right within a level, the number of secular roots it found and the number of eigenvalues it deflated (their sum
 * is the merge's order).  On `stream` (NULL: the handle's); the convergence word goes where ptmi_eig_sytrd_info reads it.  The call
 * uses the scratch and the convergence word of ptmi_eig_sytrd: it must not overlap a factorization of the same handle on another
 * stream (an engine with eig_lag: wait for the pending table first), nor another call of itself.
 * ptmi_eig_sytrd_reduction: copies what the tridiagonalization of the handle's most recent ptmi_eig_sytrd[_from] left in the scratch
 * to the caller's device buffers, on `stream` (NULL: the handle's; a stream other than the factorization's must wait for it first):
 * D [ndim], E [ndim - 1], tau [ndim - 1], A [ndim][ndim] in LAPACK dsytrd's column-major lower storage -- reflector m is (1 at
 * m + 1, A[m * ndim + i] for i >= m + 2); every other entry of A is still the input's (d and e come in D and E only).  Before any
 * factorization: PTMI_EINVAL. */
int ptmi_eig_dc_tridiag(ptmi_handle h, void *stream, const double *d, const double *e, double *W, double *Z, int32_t *cnt);
int ptmi_eig_sytrd_reduction(ptmi_handle h, void *stream, double *D, double *E, double *tau, double *A);

/* _updateDEbuffer (:806-817): drop the oldest cov_update rows of each DE history and
 * append the AM buffer (pooled mode: row r comes from walker r mod W). */
int ptmi_update_de(ptmi_handle h);

/* Position of the logical row 0 inside the DE ring; a GPU that does not hold rank 0 receives
 * the new rows from the one that does and then advances its ring by hand. */
int ptmi_set_de_head(ptmi_handle h, int32_t head);

/* Split path for host (Python) likelihood callbacks, one iteration per call:
 * propose writes Q and qaux for every chain; the caller evaluates logp/logl on Q;
 * accept applies the Hastings test with the caller's values (NaN-safe, -inf prior). */
int ptmi_propose(ptmi_handle h, int64_t iter);
int ptmi_accept(ptmi_handle h, int64_t iter, const double *newlnL /* dev [W][T] */, const double *newlp /* dev [W][T] */);
/* ptmi_accept(iter) and ptmi_propose(iter + 1) in ONE launch (csrc/ptmi_split.hip): a chain's row comes in once -- the accepted
 * proposal or the old state -- and goes out once as the next proposal (and to X where accepted), where the two calls moved it twice;
 * the inner loop of a run whose likelihood is a batched device callback (PTMCMCSampler.py:601-622 between epochs).  The caller calls
 * it only where NOTHING sits between the two iterations: no swap (iter a multiple of Tskip: refused), no covariance / DE epoch
 * and no DE activation at iter + 1 (the caller's schedule; PTEngine.run_callback).  qaux[.][2] then holds the next iteration's
 * accept uniform, not this one's decision (nacc / jstat count it).  Same results as the two calls, bit for bit. */
int ptmi_accept_propose(ptmi_handle h, int64_t iter, const double *newlnL /* dev [W][T] */, const double *newlp /* dev [W][T] */);
/* Cycles with AM entries on the split path: the increments U (cd sqrt(S) z) of the AM picks (:879-933) of iterations iter0 .. iter0 +
 * nsteps - 1 are made AHEAD on the matrix cores (one matrix product for all picks of the piece) with the tables as they are at this call;
 * ptmi_propose / ptmi_accept_propose then read them.  nsteps <= ptmi_split_am_piece (0 there: this handle's AM proposals come from the
 * shape kernels and no call is needed).  A proposal for an iteration no prepared piece covers prepares that one iteration itself, so
 * the call is an optimisation -- the caller makes it at the head of a span of iterations between which NOTHING changes the tables or
 * the cycle (PTEngine.callback_segment). */
int ptmi_split_am_piece(ptmi_handle h, int32_t *piece);
int ptmi_split_am_prepare(ptmi_handle h, int64_t iter0, int32_t nsteps);
/* The split path's inner loop in a hipGraph (launch-bound at small batches: two launches of a few microseconds per iteration).
 * ptmi_set_stream retargets the handle's stream (to the stream a graph is being captured on, and back).  With ptmi_device_iter(h, 1)
 * the `iter` argument of ptmi_propose / ptmi_accept / ptmi_accept_propose is an OFFSET from an iteration counter in device memory that
 * ptmi_set_device_iter writes on the stream -- so a captured span [ptmi_propose(0), callback, ptmi_accept_propose(0), ..., ptmi_accept(L - 1)]
 * replays for any first iteration: set the counter, launch the graph (PTEngine.run_callback(graph=True)).  The kernels derive the
 * ring row and the swap-iteration test from the counter; the host-side checks of those calls are off in this mode; cycles with AM
 * entries are refused (their increments are listed on the host's iteration).  Whatever the captured launches bake in -- the DE
 * ring's head, whether DE is in the cycle -- must hold at replay: the caller captures again when it changes. */
int ptmi_set_stream(ptmi_handle h, void *stream);
/* (a replayed graph does not move the host's record of which buffer holds the current proposals: the caller restores what the capture
 * ended with -- 0 = Q, 1 = Q2 -- for ptmi_proposals' sake) */
int ptmi_set_proposals(ptmi_handle h, int32_t which);
int ptmi_device_iter(ptmi_handle h, int32_t on);
int ptmi_set_device_iter(ptmi_handle h, int64_t value);
/* The buffer that holds the current proposals: Q after ptmi_propose; after ptmi_accept_propose Q or Q2 in turn when the handle has
 * both (ptmi_buffers.Q2: X is then authoritative again only after ptmi_accept), else Q.  The callback reads THIS buffer. */
int ptmi_proposals(ptmi_handle h, double **q);
/* The handle's built-in likelihood of n rows [n][ndim] anywhere on the device (the proposals, say), with the BITS the fused kernels
 * give it (the same lanes, the same summation order): a likelihood "callback" that is a device kernel behind the C ABI -- with it
 * the split path reproduces the fused path bit for bit at any size (tests), and bench.py times the split path with a callback that
 * costs one pass over the proposals.  PTMI_LOGL_ISO (oracle/ptmcmc_oracle.c eval_logl: -lane_dot(x, x) / 2) and PTMI_LOGL_DENSE
 * (eval_logl; the reference's tests/test_simple.py:14-41: r = x - mu, v = the k-ascending fma chains of r through the half table Tl,
 * -lane_dot(r, v) -- on the matrix cores, csrc/ptmi_dense_rows.hip; any ndim the handle takes, rows with inf / NaN as the oracle
 * gives them); the other families: PTMI_EUNSUPPORTED.  On the handle's stream, no host synchronisation, graph-capturable. */
int ptmi_rows_logl(ptmi_handle h, const double *rows /* dev [n][ndim] */, int64_t n, double *out /* dev [n] */);
/* ... and its gradient with it (oracle: eval_logl_grad, exported as orc_logl_grad): PTMI_LOGL_ISO -x (the reference's
 * tests/test_nuts.py:22-25), PTMI_LOGL_DENSE -(Pt r), the FULL product with P as given, one k-ascending fma chain per element.
 * (lnl, dlnl) is the form ptmi_gj_step takes.  Same stream rules. */
int ptmi_rows_logl_grad(ptmi_handle h, const double *rows /* dev [n][ndim] */, int64_t n, double *lnl /* dev [n] */, double *dlnl /* dev [n][ndim] */);
/* The handle's built-in prior of n rows (oracle: eval_logp; the reference's tests/test_simple.py:36-41): PTMI_LOGP_FLAT 0;
 * PTMI_LOGP_BOX -inf unless lo <= x <= hi in every element (a NaN element: -inf).  dlp (or NULL): its gradient, zeros (func_grad_white
 * of the oracle: "gradient of the built-in priors is zero").  Same stream rules. */
int ptmi_rows_logp(ptmi_handle h, const double *rows /* dev [n][ndim] */, int64_t n, double *lp /* dev [n] */, double *dlp /* dev [n][ndim] or NULL */);

/* HMC and NUTS with the caller's batched GRADIENT callbacks on the split path (csrc/ptmi_gjcb.hip): HMCJump.__call__ (NJ:238-291,
 * NJ = PTMCMCSampler/nutsjump.py; whitening NJ:51-54, 71-90; leapfrog NJ:149-169) and NUTSJump.__call__ (NJ:654-840) of the reference
 * for every chain whose pick of the iteration is HMC or NUTS, with beta logL + logp and its gradient from the caller instead of a
 * built-in family.  A split handle with w_nuts + w_hmc > 0 draws the pick over w_scam + w_am + w_de + w_nuts + w_hmc (PT:225-258, as
 * ptmi_mh_steps does); an HMC or NUTS pick's proposal row is the state itself until the stage below replaces it.  Per proposal launch
 * (ptmi_propose(iter), or the propose half of ptmi_accept_propose(iter - 1)):
 *
 *     ptmi_gj_begin(h, iter, work, rows, &n);
 *     while (n > 0) {
 *         callback on rows[0..n): lnL[n], dlnL[n][ndim] (and lnp[n], dlnp[n][ndim], or NULL NULL: a flat prior)
 *         ptmi_gj_step(h, work, lnL, dlnL, lnp, dlnp, rows, &n);
 *     }
 *     likelihood callback on the proposals (ptmi_proposals), then ptmi_accept / ptmi_accept_propose
 *
 * ptmi_gj_begin lists the HMC and NUTS chains in ascending chain slot (w * T + s: a stable compaction, no atomics: the rows come in the
 * same order on every run) and writes backward(forward(x)) of each into rows [n][ndim] -- L^T L^-T x, not x bitwise: the reference
 * evaluates func_grad_white(q0).  Each ptmi_gj_step is one round: it takes the callback's values for the n rows of the round before
 * and advances each listed chain to its next gradient evaluation or the end of its call.  HMC: the momenta and nsteps = randint(hmc_min,
 * hmc_max) at a chain's first round, then per round one leapfrog and the energy guard (joint1 - 1000 < joint0, NJ:284-286); at the end
 * backward(q) into its row of the current proposal buffer, qxy = joint1 - joint0 into qaux[.][0], its calls / leapfrogs into
 * gj[.][GJ_HITER] / [GJ_NLEAP].  NUTS: one round per leapfrog of the call -- on a chain's first NUTS call (gj[.][GJ_HAVE_EPS] = 0) the
 * step-size search's (find_reasonable_epsilon, NJ:435-463, both loops bounded at 100 turns: up to ~200 rounds), then one per leaf of
 * the doublings (NJ:716-802; heights 0..nuts_maxdepth); the merges with the pending left subtrees, the stop criteria and the draws run
 * between them; at the end the dual averaging into gj[.][GJ_EPS..GJ_NITER], backward(sample) into the proposal buffer, qxy = logp0 -
 * lnprob into qaux[.][0], the leapfrogs into gj[.][GJ_NLEAP].  The stage is over when n comes back 0.  The arithmetic is GradJump::hmc /
 * ::nuts of csrc/ptmi_gj.inc.h operation for operation, the same Philox slots: given the oracle's values and gradients the proposals
 * and the jump state are the bits of the fused kernels (tests/test_gj_callback_gpu.py, tests/test_gj_nuts_callback_gpu.py).
 *
 * work: caller-owned device memory of ptmi_gj_work_bytes bytes (the chains' whitened q and p, their stage scalars, the round's chain
 * list; with w_nuts > 0 also every chain's NUTS call and tree stack).  With nch = nwalkers * ntemps, d = ndim, al(b) = b rounded up to
 * 16 bytes and L = nuts_maxdepth + 1:
 *     HMC only:    al(8 nch d) * 3 + al(8 nch) + al(16 nch) + al(4 nch) + al(4 ceil(nch / 1024)) + 16
 *     w_nuts > 0:  the above + al(8 (10 + 3 L) nch d) + al(72 nch) + al(40 nch) + al(32 L nch)
 * i.e. 10 + 3 L vectors of d doubles per chain for NUTS (the call's initial point, gradient and search momenta, the sample, both ends
 * of the trajectory with their momenta and gradients; per stack height a pending left subtree's far end, its momentum and candidate)
 * -- 88 vectors with the HMC ones at nuts_maxdepth = 24: 1.85 GB at 64 x 1024 chains of 40 parameters.  rows: device [W*T][ndim] (a
 * round lists at most every chain).  Each call reads n back to the host: one stream synchronisation per round, the only one the stage
 * adds.  ptmi_accept / ptmi_accept_propose refuse (PTMI_EINVAL) while the stage of the current proposals has not ended; so do these
 * calls out of sequence.  The shape kernels' split path (PTMI_SPLIT_ROWS=0, or a handle ptmi_split_rows_ok does not take) and
 * ptmi_device_iter mode are refused (PTMI_EUNSUPPORTED); parameter groups are fine (the proposal launch draws the group of a SCAM /
 * AM / DE pick and hands a gradient pick back unchanged; the stage never looks at groups: a gradient jump moves every parameter with the
 * whitening tables of the full initial covariance).  On the handle's stream.
 *
 * 512 < ndim <= 2048 (csrc/ptmi_gjcb_wide.hip; HMC only): the same calls, sequencing, work area (the HMC-only formula above: the
 * whitened gradient of a round lives in the chains' row slots, which are free between the listing and the backward product) and bits.
 * ptmi_gj_begin lists the HMC picks first and runs the forward and backward products over the listed chains only; a round is the
 * gradient product, the step (one wave per listed chain), the backward product and the listing.  A product is n rows times one d x d
 * table on v_mfma_f64_16x16x4_f64, every element one k-ascending fma chain from +0.0 as below 512-d (diagonal tables: d
 * multiplications). */
int ptmi_gj_work_bytes(ptmi_handle h, size_t *bytes);
int ptmi_gj_begin(ptmi_handle h, int64_t iter, void *work, double *rows /* dev [W*T][ndim] */, int64_t *n);
int ptmi_gj_step(ptmi_handle h, void *work, const double *lnl /* dev [n] */, const double *dlnl /* dev [n][ndim] */,
                 const double *lp /* dev [n] or NULL */, const double *dlp /* dev [n][ndim] or NULL */, double *rows, int64_t *n);

/* Custom jump proposals in the cycle as BATCHED device callbacks on the split path (csrc/ptmi_cj.hip): addProposalToCycle(func, weight)
 * of the reference (PT:988-1014, PT = PTMCMCSampler/PTMCMCSampler.py) and its dispatch q, qxy = func(x, iter, beta) (PT:1058-1059), for
 * every chain whose pick of the iteration is one of the handle's w_host entries at once.  The proposal launch hands such a chain's state
 * back as its proposal row with qaux[.][1] = PTMI_J_NTYPES + pick; per proposal launch (ptmi_propose(iter), or the propose half of
 * ptmi_accept_propose(iter - 1)):
 *
 *     ptmi_cj_begin(h, iter, work, rows, beta, offs);
 *     for every function f with offs[f] < offs[f + 1]:
 *         callback f on rows[offs[f] .. offs[f + 1]) with beta[...]: the proposals written over the rows, qxy[offs[f] .. offs[f + 1])
 *         (or ptmi_cj_box_draw(h, work, f, lo, hi, rows + offs[f] * ndim): qxy = 0)
 *     ptmi_cj_end(h, work, rows, qxy);
 *     likelihood callback on the proposals (ptmi_proposals), then ptmi_accept / ptmi_accept_propose
 *
 * ptmi_cj_attach (once, before the first ptmi_propose) declares that the w_host entries are served this way: fun_of_pick (HOST [w_host])
 * maps each pick index to a function 0 .. nfun - 1 (the weight copies of one function share an index; nfun <= 32, else
 * PTMI_EUNSUPPORTED), cjstat (DEVICE [W][T][w_host][2], by RANK like jstat, zeroed by the caller) takes proposed / accepted per pick index
 * (PT:602,622) from ptmi_accept / ptmi_accept_propose.  With AM entries in the cycle it makes the scratch for their increments that
 * ptmi_create leaves out for w_host > 0: ptmi_split_am_piece > 0 afterwards, the row kernels serve the handle.  A handle with w_host > 0
 * that is never attached behaves as before (the caller rewrites the proposals itself).
 * ptmi_cj_begin lists the chains with qaux[.][1] >= PTMI_J_NTYPES sorted by (function, chain slot w * T + s) -- a stable compaction, no
 * atomics: the same order on every run -- copies each one's row of the CURRENT proposal buffer (ptmi_proposals; for these picks the row
 * is the chain's state, wherever sloc says the state lives) into rows [n][ndim], writes beta[k] = 1 / T of the chain as the kernels use
 * it, and returns the spans: function f owns rows offs[f] .. offs[f + 1] - 1 (offs: HOST [nfun + 1]).  One stream synchronisation: the
 * offsets' read-back, the only one the stage adds per iteration.  ptmi_cj_end scatters the rows back into the listed chains' rows of the
 * proposal buffer and qxy [n] (NULL: zeros) into qaux[.][0].  Row copies are contiguous 16-byte pieces (8-byte for odd ndim).
 * ptmi_cj_box_draw is the reference's UniformJump (tests/test_simple.py:44-62: every parameter redrawn uniformly in [lo, hi], qxy = 0)
 * for function fun's span, from the library's own generator: parameter i of a listed chain = lo[i] + (hi[i] - lo[i]) * u, u =
 * (word >> 11) 2^-53 of word i & 1 of Philox at (seed, iter, the chain's stream id (walker0 + w) * ntemps_global + temp0 + rank,
 * 0x4000000 + (i >> 1)); lo / hi: DEVICE [ndim]; rows: that function's span.
 * work: caller-owned device memory of ptmi_cj_work_bytes bytes, 16-byte aligned (the list, the listing's block counts, the offsets);
 * rows: device [W*T][ndim]; beta: device [W*T].  ptmi_accept / ptmi_accept_propose refuse (PTMI_EINVAL) while the stage of the current
 * proposals of an attached handle has not ended; so do these calls out of sequence.  Not in ptmi_device_iter mode
 * (PTMI_EUNSUPPORTED); parameter groups are fine (the stage never looks at them).
 * Beside gradient jumps: a split handle (ptmi_buffers.Q) takes w_host > 0 together with w_nuts + w_hmc > 0 -- the reference's cycle
 * [custom entries, HMC, NUTS, SCAM, AM, DE] (PT:225-264, 988-1014), here in the pick order [custom, SCAM, AM, DE, NUTS, HMC] that propose()
 * and the oracle's mh_one define.  Per proposal launch BOTH stages then run, ptmi_gj_begin / ptmi_gj_step ... and ptmi_cj_begin / ... /
 * ptmi_cj_end, in either order: they serve disjoint chains (qaux[.][1] is PTMI_J_NUTS / PTMI_J_HMC, or >= PTMI_J_NTYPES), each writes
 * its own chains' rows of the proposal buffer and their qaux[.][0] only, and ptmi_accept / ptmi_accept_propose refuse until both have
 * ended.  Without the split buffers ptmi_create keeps refusing the combination, and ptmi_mh_steps refuses w_host > 0 as before.  On
 * the handle's stream. */
int ptmi_cj_attach(ptmi_handle h, uint64_t *cjstat /* dev [W][T][w_host][2] */, const int32_t *fun_of_pick /* host [w_host] */, int32_t nfun);
int ptmi_cj_work_bytes(ptmi_handle h, size_t *bytes);
int ptmi_cj_begin(ptmi_handle h, int64_t iter, void *work, double *rows /* dev [W*T][ndim] */, double *beta /* dev [W*T] */, int64_t *offs /* host [nfun+1] */);
int ptmi_cj_end(ptmi_handle h, void *work, const double *rows /* dev [n][ndim] */, const double *qxy /* dev [n] or NULL: zeros */);
int ptmi_cj_box_draw(ptmi_handle h, void *work, int32_t fun, const double *lo, const double *hi /* dev [ndim] */, double *rows /* dev: that function's span */);

/* Auxiliary jumps as BATCHED device callbacks on the split path (csrc/ptmi_aux.hip): addAuxilaryJump(func) of the reference (PT:1017-1028)
 * and the loop that runs every auxiliary jump on the result of the cycle entry, q, qxy_aux = aux(x, q, iter, beta); qxy += qxy_aux
 * (PT:1062-1065), for EVERY chain at once.  Per proposal launch (ptmi_propose(iter), or the propose half of ptmi_accept_propose(iter - 1)),
 * behind the gradient stage and the custom-jump stage where the handle has them:
 *
 *     ptmi_aux_begin(h, iter, xrows, beta);
 *     ptmi_proposals(h, &Q);
 *     for every auxiliary function, in the order they were added: (Q, qxy) = aux(xrows, Q, iter, beta), the qxy summed
 *     ptmi_aux_end(h, Q or NULL, qxy or NULL);
 *     likelihood callback on the proposals (ptmi_proposals), then ptmi_accept / ptmi_accept_propose
 *
 * ptmi_aux_attach (once, before the first ptmi_propose; a split handle: Q and qaux) declares that every proposal launch is followed by
 * this stage: ptmi_accept / ptmi_accept_propose then refuse (PTMI_EINVAL) while the stage of the current proposals is pending or open.
 * ptmi_aux_begin writes, for every chain slot ch = w * T + s in slot order, the chain's STATE row into xrows[ch] -- read from X, Q or Q2
 * as sloc[ch] says (between a proposal launch and the accept test a state lives where its accepted proposal was written,
 * ptmi_buffers.sloc; X on handles without Q2 / sloc and on the shape kernels' split path) -- and beta[ch] = 1 / T of the chain as the
 * kernels use it (the table ptmi_cj_begin reads).  No listing, no atomics, no host read-back: every chain takes part.  It refuses
 * (PTMI_EINVAL) while the gradient or the custom-jump stage of the current proposals has not ended -- the reference runs the auxiliary
 * jumps on the jump's result -- and when called twice or for another iteration.  q is the CURRENT PROPOSAL BUFFER itself
 * (ptmi_proposals), [W*T][ndim] in the same slot order: zero copy; a function may edit it in place or return rows of its own.
 * ptmi_aux_end copies qrows [W*T][ndim] into the proposal buffer unless it is NULL or the buffer itself, ADDS qxy [W*T] (NULL: nothing)
 * to qaux[.][0], and ends the stage; its arguments are checked before anything is launched, so a refused call (a misaligned qrows)
 * leaves the stage open and a correct call -- ptmi_aux_end(h, NULL, NULL) at the least -- ends it.  Row copies are contiguous 16-byte pieces (8-byte for odd ndim); xrows and qrows 16-byte aligned.
 * Not in ptmi_device_iter mode (PTMI_EUNSUPPORTED: the stage is not captured).  Parameter groups are fine (the stage never looks at
 * them).  State lives in the handle: ptmi_config and ptmi_buffers are unchanged.  On the handle's stream. */
int ptmi_aux_attach(ptmi_handle h);
int ptmi_aux_begin(ptmi_handle h, int64_t iter, double *xrows /* dev [W*T][ndim] */, double *beta /* dev [W*T] */);
int ptmi_aux_end(ptmi_handle h, const double *qrows /* dev [W*T][ndim], or NULL: the proposal buffer was edited in place */,
                 const double *qxy /* dev [W*T] or NULL */);

/* The likelihood callback only inside the prior's support, on the split path's batched callbacks (csrc/ptmi_sup.hip).  The reference
 * reads lp = logp(y) and calls logl(y) only when lp != -inf (PT:605-612; the first evaluation the same, PT:479-487).  Between the prior
 * callback and the likelihood callback over n_in rows of ndim doubles -- the proposal buffer, or any other row tensor:
 *
 *     lp = prior callback on rows_in [n_in][ndim]
 *     ptmi_sup_begin(h, work, lp, n_in, &n);
 *     n == n_in: vals = likelihood callback on rows_in itself (no copy);  out = vals
 *     n == 0:    no likelihood call;                                      ptmi_sup_end(h, work, NULL, out)
 *     else:      ptmi_sup_rows(h, work, rows_in, rows);  vals = likelihood callback on rows[0 .. n);  ptmi_sup_end(h, work, vals, out)
 *
 * ptmi_sup_begin lists the rows k with lp[k] != -inf in ascending k -- NaN and +inf are listed: the reference tests lp == -inf and
 * nothing else -- and leaves pos[k], the row's rank in the list or -1, in the work area: counts per block of 1024 rows, ONE block that
 * scans the block counts once, the ranks by ballots inside each block.  No atomics: the same order on every run.  *n (HOST) is the
 * number of listed rows: one stream synchronisation, the only read-back the stage adds.  A new ptmi_sup_begin replaces an open stage; one that is
 * REFUSED (a NULL or misaligned argument, n_in out of range, ptmi_device_iter mode) has launched nothing and changed nothing: a stage that
 * was open stays open, as it does behind a refused ptmi_sup_rows / ptmi_sup_end.
 * ptmi_sup_rows copies listed row j to rows[j] (launched behind the read-back: its grid is sized from n, a row to a wave; contiguous
 * 16-byte pieces, 8-byte for odd ndim); nothing is launched when n == 0.  ptmi_sup_end writes out[k] = pos[k] >= 0 ? vals[pos[k]] : -inf
 * for all n_in rows (vals == NULL: -inf everywhere) and ends the stage.
 * work: caller-owned device memory of ptmi_sup_work_bytes(n_in) bytes, 16-byte aligned (pos, the list, the block counts and starts, the
 * total); rows_in and rows 16-byte aligned (8-byte for odd ndim).  ptmi_sup_rows / ptmi_sup_end refuse (PTMI_EINVAL) without a
 * ptmi_sup_begin on the same work area; n_in outside [1, 2^31) and misaligned pointers are refused too.  Not in ptmi_device_iter
 * mode (PTMI_EUNSUPPORTED: the count is read on the host).  The accept test never reads the likelihood of a row whose prior is -inf,
 * so a run with the stage equals a run without it bit for bit for any row-wise callback.  State lives in the handle: ptmi_config and
 * ptmi_buffers are unchanged.  On the handle's stream. */
int ptmi_sup_work_bytes(ptmi_handle h, int64_t n_in, size_t *bytes);
int ptmi_sup_begin(ptmi_handle h, void *work, const double *lp /* dev [n_in] */, int64_t n_in, int64_t *n /* host */);
int ptmi_sup_rows(ptmi_handle h, void *work, const double *rows_in /* dev [n_in][ndim] */, double *rows /* dev [n][ndim] */);
int ptmi_sup_end(ptmi_handle h, void *work, const double *vals /* dev [n] or NULL */, double *out /* dev [n_in] */);

/* Marginal posterior histograms of EVERY cold chain, accumulated on the device (csrc/ptmi_hist.hip).  The AM ring holds the rank-0 row
 * of every walker for every iteration of the current covariance period (updateChains, :327-328: the post-swap row at swap iterations,
 * the repeated row behind a rejection); these calls bin every element of it.  For parameter j the caller fixes lo[j] < hi[j], nbins
 * and scale[j] = nbins / (hi[j] - lo[j]) in double precision; an element x that stands for n iterations is counted as
 *
 *     t = (x - lo[j]) * scale[j]              one subtraction, one multiplication, no fma
 *     if not (t >= 0.0):  under[j] += n       x < lo, and NaN
 *     elif t >= nbins:    over[j]  += n       x >= hi (as scale rounds), +inf
 *     else:               counts[j][(int)t] += n
 *
 * counts: DEVICE uint64 [ndim][nbins + 2] in PARAMETER order whatever the ring's row format (ptmi_am_row_format): columns
 * 0 .. nbins - 1 the bins, column nbins = under, column nbins + 1 = over; caller-owned, zeroed by the caller, 8-byte aligned.
 * ptmi_hist_attach (once per handle) takes it with lo / scale (HOST [ndim]; lo finite, scale finite and positive; the library keeps
 * device copies) and 2 <= nbins <= 1024; anything else: PTMI_EINVAL.  State lives in the handle: ptmi_config and ptmi_buffers are
 * unchanged, and a handle that never attaches launches what it launched before.
 * ptmi_hist_update adds iterations iter_lo .. iter_hi of every walker from the handle's CURRENT ring (ptmi_set_am_buffers): both in one
 * covariance period, E < iter_lo <= iter_hi <= E + cov_update with E = ((iter_hi - 1) / cov_update) * cov_update (PTMI_EINVAL for a
 * range that crosses a period, and before ptmi_hist_attach; the message says which); iter_hi < iter_lo: nothing to do.  Without AMflag
 * every row counts once; with it a row without NEW / KEY repeats the last stored row before it (ptmi_am_expand's rule; ring row 1 of
 * a period is a KEY row, so the walk back never leaves the period): every stored row is read once and carries the length of its run
 * clipped to [iter_lo, iter_hi].  The caller counts every iteration once (ranges that do not overlap) and calls before the ring
 * wraps; the ring is only read.  On a handle with temp0 != 0: PTMI_OK, nothing done (as ptmi_update_cov).  Rings of 2^32 rows or more:
 * PTMI_EUNSUPPORTED.  Asynchronous on the handle's stream, no host synchronisation; no atomics per element (a block adds its private
 * tile to counts once). */
int ptmi_hist_attach(ptmi_handle h, uint64_t *counts /* dev [ndim][nbins+2], caller-owned, caller-zeroed */,
                     const double *lo /* host [ndim] */, const double *scale /* host [ndim] */, int32_t nbins);
int ptmi_hist_update(ptmi_handle h, int64_t iter_lo, int64_t iter_hi);

/* The ladder's summaries for the log-evidence, accumulated on the device (csrc/ptmi_ev.hip): per walker and LOCAL RANK r the moments
 * of lnL that thermodynamic integration needs and the running log-sum-exp of dbeta[r] * lnL that the stepping-stone estimator needs.
 * Every call of ptmi_ev_update takes one sample of every cell (w, r) from the handle's state as it stands:
 *
 *     l = lnL[w][slot_of[w][r]];   a = dbeta[r] * l
 *     !isfinite(l)            -> skipped += 1, nothing else
 *     first sample of a cell  -> c = l; s1 = 0; s2 = 0; m = a; es = 1
 *     else                    -> t = l - c; s1 += t; s2 += t * t
 *                                a <= m: es += exp(a - m)        else: es = es * exp(m - a) + 1; m = a
 *     taken += 1
 *
 * every operation rounded on its own (no fma), exp the library's deterministic exponential (ptmi_selftest_math op 1).  So after n
 * samples mean lnL = c + s1 / n, sum (lnL - c)^2 = s2, and sum exp(dbeta[r] lnL) = exp(m) * es.  The caller decides WHEN to sample:
 * behind ptmi_swap the state is the post-swap one of that iteration, the row the reference's chain files hold for it.
 * acc: DEVICE double [5][W][T], planes c, s1, s2, m, es; cnt: DEVICE uint64 [2][W][T], planes taken, skipped; both plane-major and
 * indexed by local rank (not by slot), caller-owned, zeroed by the caller, 8-byte aligned.  dbeta: HOST [T] (the library keeps a
 * device copy), dbeta[r] = beta of the next colder rank - beta of rank r for r >= 1, computed by the caller in double precision from
 * temps_mh (beta = 1 / T); dbeta[0] is the caller's too: 0 where rank 0 is the coldest of the whole ladder, the gap to the
 * neighbouring block's hottest rank on a sharded ladder.  Every entry finite and >= 0.  ptmi_ev_attach: once per handle; a second
 * attach, NULL or misaligned buffers, a bad dbeta: PTMI_EINVAL, the message says which.  State lives in the handle: ptmi_config and
 * ptmi_buffers are unchanged, and a handle that never attaches launches what it launched before.
 * ptmi_ev_update (PTMI_EINVAL before ptmi_ev_attach): one thread per cell on the handle's stream, no host synchronisation, no atomics,
 * graph-capturable; it reads slot_of and lnL and touches nothing else of the handle.  Every cell is a sequential recurrence in time:
 * the result does not depend on the launch geometry. */
int ptmi_ev_attach(ptmi_handle h, double *acc /* dev [5][W][T] */, uint64_t *cnt /* dev [2][W][T] */,
                   const double *dbeta /* host [T] */);
int ptmi_ev_update(ptmi_handle h);

/* Convergence diagnostics of EVERY cold chain, accumulated on the device (csrc/ptmi_diag.hip): the streaming sums from which the host
 * computes Gelman-Rubin R-hat and a batch-means autocorrelation time / effective sample size over all nwalkers replicas
 * (ptmcmcsampler_amd/diagnostics.py).  The reference's one convergence check is the neff stop rule, PTMCMCSampler.py:510-521: acor on
 * the host over one kept chain read back from its file; these calls serve the same rule from every walker's cold chain, which the AM
 * ring holds for the current covariance period (as ptmi_hist_update reads it).  One independent stream per (walker w, parameter j) over
 * the cold row x of every counted iteration, in iteration order; n (samples folded so far) is the same for all streams:
 *
 *     if n == 0: c = x                         the stream's shift: its first counted sample
 *     y = x - c
 *     S1 += y;  S2 += y * y;  A += y;  n += 1
 *     if n % batch0 == 0:
 *         k = n / batch0;  t = A;  A = 0.0
 *         for l = 0 .. nlevels - 1:
 *             Q[l] += t * t                    sum of squared batch sums at level l, batch length batch0 << l
 *             if l == nlevels - 1: break
 *             if (k >> l) & 1: H[l] = t; break        first half of a pair: wait for its partner
 *             t = H[l] + t                     the pair is a level l + 1 batch
 *
 * every operation rounded on its own, in this order (no fma); non-finite samples are not special-cased (they poison their stream's
 * sums and no other's).  With AMflag a row without NEW / KEY repeats the last stored row before it (ptmi_am_expand's rule) and is added
 * once per iteration: the sums do not depend on the ring mode, on how a period is cut into calls or on the launch geometry.
 * acc: DEVICE double [2 * nlevels + 3][W][ndim], plane-major, in PARAMETER order whatever the ring's row format (ptmi_am_row_format):
 * plane 0 c, 1 S1, 2 S2, 3 A, planes 4 .. 4 + nlevels - 1 Q, planes 4 + nlevels .. 2 nlevels + 2 H[0 .. nlevels - 2]; caller-owned,
 * zeroed by the caller, 8-byte aligned.  ptmi_diag_attach (once per handle): 1 <= nlevels <= 16, batch0 >= 1; anything else
 * PTMI_EINVAL.  State lives in the handle: ptmi_config and ptmi_buffers are unchanged, and a handle that never attaches launches what
 * it launched before.  The library keeps no count: n_done, the samples folded before iter_lo, comes in with every call (a
 * checkpoint is acc plus one integer).
 * ptmi_diag_update folds iterations iter_lo .. iter_hi of every walker from the handle's CURRENT ring (ptmi_set_am_buffers), with the
 * contract of ptmi_hist_update: both in one covariance period (PTMI_EINVAL for a range that crosses one, for n_done < 0, before
 * ptmi_diag_attach and on a cold handle without an AM buffer); iter_hi < iter_lo: nothing to do; temp0 != 0: PTMI_OK, nothing done.
 * The caller folds every iteration once, in order, and calls before the ring wraps; the ring is only read.  One thread per stream,
 * asynchronous on the handle's stream, no host synchronisation, no atomics. */
int ptmi_diag_attach(ptmi_handle h, double *acc /* dev [2*nlevels+3][W][ndim], caller-owned, caller-zeroed */, int32_t nlevels,
                     int32_t batch0);
int ptmi_diag_update(ptmi_handle h, int64_t iter_lo, int64_t iter_hi, int64_t n_done);

/* The temperature ladder adapted on the device from EVERY walker's accepted swaps (csrc/ptmi_ladder.hip).  The reference's ladder is
 * fixed (temperatureLadder, :699-720); nswap [W][n] (n = ntemps_global; column k = pair (k, k + 1), credited to the lower rank, :681)
 * holds what every pair accepted.  State of the whole ladder, with n1 = n - 1 pairs: g[k] = ln T[k + 1] - ln T[k], the log gaps; T[k],
 * the ladder; seen[k], the accepted swaps of pair k already consumed.  One ptmi_ladder_update(h, kappa, tries_even, tries_odd):
 *
 *     acc[k] = sum_w nswap[w][k]                                 uint64, exact
 *     A[k]   = (double)(acc[k] - seen[k]) / ((double)W * (double)(k even ? tries_even : tries_odd))     k = 0 .. n1 - 1
 *                                                                (the difference in integers; one product, one division)
 *     h[k]   = g[k] * exp(kappa * A[k])
 *     s = 0.0; for k ascending: s = s + h[k]
 *     G = 0.0; for k ascending: G = G + g[k]
 *     g'[k]  = G * (h[k] / s)
 *     c = 0.0; for k = 1 .. n - 2:  c = c + g'[k - 1];  T[k] = T[0] * exp(c)
 *     seen[k] = acc[k]; g = g'                                   T[0] and T[n - 1] are never rewritten
 *
 * every operation rounded on its own, in this order (no fma), exp the library's deterministic exponential (ptmi_selftest_math op 1),
 * the division IEEE's (op 4).  A pair that accepted more than the others gets a wider gap, the sum of the gaps and both ends of the
 * ladder stay; only differences of A matter; the fixed point is equal acceptance on every pair.  tries_even / tries_odd: how often
 * the window tried the pairs with even / odd k (PTMI_SWAP_SWEEP: every swap epoch counts for both; PTMI_SWAP_ODDEVEN: epoch e tries
 * k = e mod 2).  With two temperatures there is no interior rank: the update writes A and seen only.
 * The publish step -- ptmi_ladder_publish, and the end of every update -- makes the handle's tables those of plane T:
 * d_ladder[k] = T[k] (what ptmi_swap reads); for every local rank r that sampled at its ladder entry when ptmi_ladder_attach was
 * called (temps_mh[r] == ladder[temp0 + r]: not a hot chain at 1e80) temps_mh[r] = T[temp0 + r] and beta[r] = 1.0 / temps_mh[r] (what
 * every step, split, gradient and callback kernel reads); with ptmi_ev_attach done, dbeta[r] = beta[r - 1] - beta[r] for r >= 1
 * (dbeta[0] stays).  lnL and lp are stored apart and no tempered value is cached: nothing is re-evaluated, and captured graphs stay valid.
 * lad: DEVICE double [3][n], planes g, A (of the last window), T; seen: DEVICE uint64 [n]; caller-owned, 8-byte aligned; the caller
 * fills g and T from its ladder and zeroes A and seen (entry n - 1 of g, A and seen is not used).  A caller that overwrites plane T
 * (a restored checkpoint, a ladder of its own -- with g to match) calls ptmi_ladder_publish.  ptmi_ladder_attach: once per handle
 * (it waits for the stream once, to read the tables); a second attach, NULL or misaligned buffers, ntemps_global < 2: PTMI_EINVAL, the
 * message says which; ntemps != ntemps_global (a sharded ladder: the sums would need a reduction across blocks): PTMI_EUNSUPPORTED.
 * ptmi_ladder_update refuses (PTMI_EINVAL, nothing launched) before an attach, kappa not finite or outside [0, 8], tries_even < 1, and
 * tries_odd < 1 with three temperatures or more; ptmi_ladder_publish and ptmi_ladder_read refuse before an attach.  State lives in the
 * handle: ptmi_config and ptmi_buffers are unchanged, and a handle that never attaches launches what it launched before.
 * Update (two launches: column sums of the walkers' slabs, read rank-fastest; one finishing block) and publish (one launch) run
 * asynchronously on the handle's stream: no host synchronisation, no atomics, graph-capturable.  The walker sums are integer sums and
 * the floating-point part is one sequential pass in ascending k: the result does not depend on the launch geometry.
 * ptmi_ladder_read copies the handle's tables to HOST memory; it is the one entry point that waits (for the handle's stream). */
int ptmi_ladder_attach(ptmi_handle h, double *lad /* dev [3][ntemps_global]: planes g, A (last window), T */,
                       uint64_t *seen /* dev [ntemps_global] */);
int ptmi_ladder_update(ptmi_handle h, double kappa, int64_t tries_even, int64_t tries_odd);
int ptmi_ladder_publish(ptmi_handle h);
int ptmi_ladder_read(ptmi_handle h, double *ladder /* host [ntemps_global] */, double *temps_mh /* host [T] */, double *beta /* host [T] */);

/* Joint posterior histograms of parameter PAIRS from EVERY cold chain, accumulated on the device (csrc/ptmi_pairs.hip): the
 * off-diagonal panels of a corner plot, from the ring that ptmi_hist_update reads.  The caller fixes npairs pairs (i, j) of different
 * parameters (order matters: (j, i) is the transpose), lo[k] < hi[k], nbins per axis and scale[k] = nbins / (hi[k] - lo[k]) in double
 * precision.  A ring row x that stands for n iterations is counted once per pair p = (i, j):
 *
 *     ti = (x[i] - lo[i]) * scale[i];  tj = (x[j] - lo[j]) * scale[j]      ptmi_hist_update's rule per axis: no fma
 *     inside(t) = (t >= 0.0) and not (t >= nbins)                          NaN, x < lo, x >= hi (as scale rounds), +-inf: outside
 *     if inside(ti) and inside(tj):  counts[p][(int)ti * nbins + (int)tj] += n
 *     else:                          counts[p][nbins * nbins] += n         one "outside" cell per pair
 *
 * counts: DEVICE uint64 [npairs][nbins * nbins + 1]; caller-owned, zeroed by the caller, 8-byte aligned.  ptmi_pairs_attach (once per
 * handle) takes it with pairs (HOST int32 [npairs][2]), lo / scale (HOST [ndim]; the library keeps device copies of what it needs),
 * 1 <= npairs <= 8192 and 2 <= nbins <= 128.  PTMI_EINVAL, the message says which: NULL or misaligned counts, npairs or nbins out of
 * range, an index outside 0 .. ndim - 1, i == j, a lo that is not finite, a scale that is not finite and positive, a second attach.
 * State lives in the handle and is freed with it: ptmi_config and ptmi_buffers are unchanged, a handle that never attaches launches
 * what it launched before, and ptmi_hist_attach may stand beside it.
 * ptmi_pairs_update adds iterations iter_lo .. iter_hi of every walker from the handle's CURRENT ring with the contract of
 * ptmi_hist_update: both in one covariance period (PTMI_EINVAL for a range that crosses one, and before ptmi_pairs_attach);
 * iter_hi < iter_lo: nothing to do; the run-length weights of rings with AMflag are ptmi_hist_update's, so every iteration of every
 * walker counts once per pair and a pair's cells grow by nwalkers * (iter_hi - iter_lo + 1).  temp0 != 0: PTMI_OK, nothing done.  Rings
 * of 2^32 rows or more: PTMI_EUNSUPPORTED.  Asynchronous on the handle's stream, no host synchronisation, the ring is only read; no
 * global atomics per element (a block adds its private tile of pair tables to counts once). */
int ptmi_pairs_attach(ptmi_handle h, uint64_t *counts, const int32_t *pairs, int32_t npairs, const double *lo, const double *scale,
                      int32_t nbins);
int ptmi_pairs_update(ptmi_handle h, int64_t iter_lo, int64_t iter_hi);

/* Thinned SAMPLES of EVERY cold chain, kept on the device (csrc/ptmi_samples.hip): what corner plots, derived parameters, posterior
 * predictive draws and importance reweighting take, where the calls above yield fixed summaries.  The reference keeps the thinned rows
 * of its one chain on the host (updateChains, :331-335); these calls keep a bounded set of snapshots of all nwalkers cold chains, read
 * from the ring that ptmi_hist_update reads.  The caller owns the schedule (which iteration goes to which slot:
 * ptmcmcsampler_amd/samples.py SlotPlan); the library gathers.  For walker w, iteration E + k of the period the ring holds and slot s:
 *
 *     r = k                                       without AMflag: every row is stored
 *     r = the nearest k' <= k with NEW | KEY      with AMflag (ptmi_am_expand's rule; ring row 1 of a period is a KEY row, so the
 *                                                 walk back never leaves the period)
 *     rows[s][w][i]     = the element of parameter i in ring row r % cov_update        (k == cov_update sits in ring row 0)
 *     aux[s][w][0 .. 1] = AMaux[w][k % cov_update][0 .. 1]                             lnL and lp of iteration E + k itself: AMaux
 *                                                                                     is written at every iteration, stored or not
 *
 * moved as 64-bit words: NaN, infinities and -0.0 arrive bit for bit.
 * rows: DEVICE double [nslots][W][ndim] in PARAMETER order whatever the ring's row format (ptmi_am_row_format); aux: DEVICE double
 * [nslots][W][2] (lnL, lp), or NULL; both caller-owned, 8-byte aligned.  ptmi_samples_attach (once per handle): 1 <= nslots <= 65535;
 * PTMI_EINVAL, the message says which: NULL or misaligned rows, misaligned aux, aux on a handle without AMaux, nslots out of range, a
 * second attach ("already attached").  State lives in the handle and is freed with it: ptmi_config and ptmi_buffers are unchanged,
 * and a handle that never attaches launches what it launched before.
 * ptmi_samples_take gathers n (iteration, slot) pairs from the handle's CURRENT ring (ptmi_set_am_buffers): iters HOST [n] strictly
 * ascending and all in one covariance period, E < iters[0], iters[n - 1] <= E + cov_update with E = ((iters[n - 1] - 1) / cov_update) *
 * cov_update; slots HOST [n], distinct, 0 <= slot < nslots, so no two pairs of a call write the same cell.  PTMI_EINVAL, the message says
 * which: before ptmi_samples_attach, n < 0, iterations that are not ascending, a repeated slot, a slot out of range, a range that
 * crosses a period.  n == 0, or a handle with temp0 != 0: PTMI_OK, nothing done (as ptmi_update_cov).  The caller takes an iteration
 * before the ring wraps; the ring is only read.  The host arrays are consumed before the call returns (the pairs travel as kernel
 * arguments, 256 per launch): nothing on the host has to outlive the call.  One wave per (pair, walker); asynchronous on the handle's
 * stream, no host synchronisation, no atomics. */
int ptmi_samples_attach(ptmi_handle h, double *rows /* dev [nslots][W][ndim], PARAMETER order, caller-owned */,
                        double *aux /* dev [nslots][W][2] (lnL, lp) or NULL */, int32_t nslots);
int ptmi_samples_take(ptmi_handle h, const int64_t *iters /* host [n], strictly ascending */,
                      const int32_t *slots /* host [n], distinct, 0 <= slot < nslots */, int32_t n);

/* The BEST-FIT row of EVERY cold chain over ALL iterations (csrc/ptmi_best.hip): the maximum a posteriori (MAP) and the maximum
 * likelihood (ML) point -- the reference value of a corner plot, the start of an optimiser or a Fisher estimate, the lnL_max of an
 * information criterion.  They replace the arg-max a user of the reference takes over the lnprob / lnlike columns of the chain file
 * that _writeToFile writes (chain[np.argmax(chain[:, -4])], chain[np.argmax(chain[:, -3])]): that file holds the thinned rows of one
 * chain, these calls see every iteration of all nwalkers cold chains, read from the ring that ptmi_hist_update reads.  Per walker w two
 * planes keep a running best each, with the score
 *
 *     plane 0 (MAP):  s = beta0 * lnL + lp        the product rounded, then the sum: no fused multiply-add (the lnprob of the chain files)
 *     plane 1 (ML):   s = lnL
 *
 * lnL, lp = AMaux[w][k % cov_update][0 .. 1] of iteration E + k itself (AMaux is written at every iteration, stored or not).  Going
 * through the iterations in ascending order a candidate replaces the held best iff s is not NaN AND (nothing is held OR s > held), the
 * strict IEEE comparison: the earliest iteration with the maximum wins, 0.0 and -0.0 tie, a NaN never wins and never poisons, -inf
 * wins only against "nothing held" -- so the state does not depend on how a run is cut into calls.  Where plane p of walker w improves:
 *
 *     rows[p][w][i]      = the element of parameter i in ring row r % cov_update, r = k without AMflag, else the nearest k' <= k with
 *                          NEW | KEY (ptmi_am_expand's rule, clamped to the period; k == cov_update sits in ring row 0)
 *     val[p][w][0 .. 2]  = s, lnL, lp
 *     iters[p][w]        = E + k
 *
 * rows, lnL and lp moved as 64-bit words: payloads arrive as they were.
 * rows: DEVICE double [2][W][ndim] in PARAMETER order whatever the ring's row format (ptmi_am_row_format); val: DEVICE double
 * [2][W][3]; iters: DEVICE int64 [2][W], set to -1 (= nothing held) by the caller; all caller-owned, 8-byte aligned.  ptmi_best_attach
 * (once per handle): PTMI_EINVAL, the message says which: NULL or misaligned rows / val / iters, a handle without AMaux, beta0 not
 * finite or not positive, a second attach ("already attached").  State lives in the handle and is freed with it: ptmi_config and
 * ptmi_buffers are unchanged, and a handle that never attaches launches what it launched before.
 * ptmi_best_update takes iterations iter_lo .. iter_hi of the handle's CURRENT ring (ptmi_set_am_buffers), all in one covariance
 * period: E < iter_lo, iter_hi <= E + cov_update with E = ((iter_hi - 1) / cov_update) * cov_update.  PTMI_EINVAL: before
 * ptmi_best_attach, a range that crosses a period, a handle with no AM buffer.  iter_hi < iter_lo, or a handle with temp0 != 0:
 * PTMI_OK, nothing launched (as ptmi_update_cov).  The caller takes an iteration before the ring wraps; the ring is only read
 * (16 * W * (iter_hi - iter_lo + 1) bytes), at most 2 * W * (ndim + 4) * 8 bytes are written.  One wave per walker, one launch;
 * asynchronous on the handle's stream, no host synchronisation, no atomics. */
int ptmi_best_attach(ptmi_handle h, double *rows /* dev [2][W][ndim], PARAMETER order, caller-owned */,
                     double *val /* dev [2][W][3]: score, lnL, lp */, int64_t *iters /* dev [2][W], -1 = nothing held */, double beta0);
int ptmi_best_update(ptmi_handle h, int64_t iter_lo, int64_t iter_hi);

/* Self-test hooks used by the parity tests: evaluate the device's deterministic math on
 * n inputs (op: 0 log, 1 exp, 2 cos2pi, 3 sqrt, 4 reciprocal-free divide a/b with b=in2). */
int ptmi_selftest_math(int device, int op, const double *in, const double *in2, double *out, int64_t n);
int ptmi_selftest_philox(int device, const uint32_t *ctr_key /* [n][6] */, uint32_t *out /* [n][4] */, int64_t n);
/* Replay hook of the parity tests (tests/test_gpu_replay.py): the reference's RECORDED draws go into the production kernels in
 * place of the Philox ones.  swap_uniforms (dev [W][ntemps_global - 1], index [w][k] = the uniform of pair (k, k+1), :679) feeds
 * ptmi_swap / ptmi_swap_sweep*; draws (dev [W][T][4] 64-bit words per chain: P0 = cycle pick << 32 | scale-branch word, Q0, Q1 as
 * DESIGN.md section 4 lays them out, and the bits of a double: the SCAM normal, :873, or DE's scale uniform, :976) feeds ptmi_propose.
 * NULL switches a hook off. */
int ptmi_test_replay(ptmi_handle h, const double *swap_uniforms, const uint64_t *draws);

/* plain device memory helpers, so that a C caller needs nothing but this library */
int ptmi_malloc(void **p, size_t bytes);
int ptmi_free(void *p);
int ptmi_memcpy_h2d(void *dst, const void *src, size_t bytes);
int ptmi_memcpy_d2h(void *dst, const void *src, size_t bytes);
int ptmi_memset(void *dst, int value, size_t bytes);

/* HIP-event stopwatch on the handle's stream (bench.py's kernel timing) */
int ptmi_timer_start(ptmi_handle h);
int ptmi_timer_stop_ms(ptmi_handle h, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_H */
