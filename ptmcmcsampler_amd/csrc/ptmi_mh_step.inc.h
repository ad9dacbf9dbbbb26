// ptmi_mh_step.inc.h -- the body of ONE Metropolis-Hastings step of mh_steps_kernel (ptmi_mh.inc.h), included as text where a step runs:
// in the rolled step loop (PTMI_STEP_S = -1) and, in the persistent exact-shape kernel (PIPE), once for each of the four straight-line
// steps of a full pass (PTMI_STEP_S = 0..3: the step's index in the pass, a compile-time constant).  Text and not a lambda, so that the
// kernels that only have the rolled loop compile to what they compiled to before there was a second place.  Expects `k` (the step of the
// launch) and everything mh_steps_kernel has declared by then.
#ifndef PTMI_STEP_S
#error "define PTMI_STEP_S (-1, or the step's index in a straight-line pass) before including ptmi_mh_step.inc.h"
#endif
        constexpr int SV = PTMI_STEP_S;
        const long long it = a.iter0 + k;
        if constexpr (AMQ) {
            if (amq_on) {
                const int s4 = k & 3, c16 = lane & 15;
                if (s4 == 0) {
                    // the picks of the block of four steps that starts at step kb; its events take ranks from `base` on
                    auto look = [&](int kb, u64 &mask, int &rank, double &cdv, int base) {
                        bool ev = false;
                        cdv = 0.0;
                        if (kb + gl < a.nsteps) {
                            u64 p0, p1;
                            philox_words(a.seed, (u64)(a.iter0 + kb + gl), sid, 0u, p0, p1);
                            const int w_de = a.de_on ? a.w_de : 0;
                            const int ind = (int)h2index((u32)(p0 >> 32), (u32)(a.w_host + a.w_scam + a.w_am + w_de)) - a.w_host;   // as propose()
                            ev = live && ind >= a.w_scam && ind < a.w_scam + a.w_am;
                            constexpr u32 T97 = (u32)(0.97 * 4294967296.0), T90 = (u32)(0.9 * 4294967296.0);
                            const u32 plo = (u32)p0;
                            cdv = a.gcn[0] * cc.sc(plo > T97 ? 0 : (plo > T90 ? 1 : 2));                                    // PT:928
                        }
                        mask = __ballot(ev);
                        rank = base + (int)__popcll(mask & ((1ull << lane) - 1ull));
                        if (ev) PTMI_AMQ_IDX[rank & 127] = lane | (((kb >> 2) & 1) << 6);
                    };
                    if (k == 0) look(0, mask_n, rank_n, cd_n, 0);
                    mask_c = mask_n; rank_c = rank_n; cd_c = cd_n; base_c = base_n;
                    base_n = base_c + (int)__popcll(mask_c);
                    look(k + 4, mask_n, rank_n, cd_n, base_n);
                    asm volatile("" ::: "memory");                       // LDS serves a wave in order; this orders the compiler
                }
                const int cons = base_c + (int)__popcll(mask_c & ((1ull << (16 * s4)) - 1ull));                             // events of the steps before this one
                const int need = base_c + (int)__popcll(mask_c & (s4 == 3 ? ~0ull : ((1ull << (16 * s4 + 16)) - 1ull)));    // ... up to and including it
                if (q_done < need) {                                     // wave-uniform: a matrix pass for ranks [q_done, hi)
                    const int known = base_n + (int)__popcll(mask_n);
                    const int hi = known < cons + 16 ? known : cons + 16;
                    const int r = q_done + c16;
                    const bool valid = r < hi;
                    const int entry = PTMI_AMQ_IDX[(valid ? r : q_done) & 127];
                    const int owner = entry & 63;
                    const bool of_cur = (entry >> 6) == ((k >> 2) & 1);
                    const u32 sid_ev = (u32)__shfl((int)sid, owner, 64);
                    const double cdc = __shfl(cd_c, owner, 64), cdn = __shfl(cd_n, owner, 64);
                    const double cd_ev = of_cur ? cdc : cdn;
                    const long long it_ev = a.iter0 + (k - s4) + (of_cur ? 0 : 4) + (owner >> 4);
                    MfmaAcc<EPL> acc;
                    if (UT_ALWAYS_LDS || a.lds_u) am_mfma_product<EPL>(a, valid, sid_ev, it_ev, cd_ev, d, PTMI_UL, true, mfma_ld(EPL), PTMI_SQ, true, acc, tsm);
                    else am_mfma_product<EPL>(a, valid, sid_ev, it_ev, cd_ev, d, UtBlock, false, d, PTMI_SQ, true, acc, tsm);
                    if (valid) {
#pragma unroll
                        for (int e = 0; e < EPL; ++e) PTMI_AMQ(r & 15)[gl * EPL + e] = acc.at(e);
                    }
                    q_done = hi;
                    asm volatile("" ::: "memory");
                }
            }
        }
        double log_u;
        int jt = PTMI_J_SCAM;
        double scam_amp = 0.0, box_reach = 0.0;
        if constexpr (SCAMFAST) {
            ScamDraw sd;
            if constexpr (SV >= 0) {
                // log u and the amplitude from the chain's lane SV; the row was requested a step ahead
                constexpr int QP = (SV & 3) * 0x55;               // quad_perm [SV,SV,SV,SV]
                sd.log_u = dppf64<QP>(sbatch.lg);
                sd.amp = dppf64<QP>(sbatch.amp);
                sd.k = 0;
            } else {
                scam_draws_for_step<STR, STM, GW>(sbatch, sd, a, k, sid, gl, cc, d, scam_root_s, smem);
            }
            log_u = sd.log_u;
            if constexpr (SV >= 0) {
#pragma unroll
                for (int e = 0; e < EPL; ++e) dq[e] = sd.amp * urow[e];
                if constexpr (SV < 3) {
                    // the loads return long after the products have read their operands: the same registers
                    constexpr int QN = ((SV + 1) & 3) * 0x55;
                    __builtin_amdgcn_sched_barrier(0);
                    row_request((int)dpp32<QN>((u32)koff));
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else if constexpr (PAIRED) {
                const double *row = smem + (size_t)sd.k * d;
                const ptmi_d2 *rp = reinterpret_cast<const ptmi_d2 *>(row) + gl;
#pragma unroll
                for (int e2 = 0; e2 < EPL / 2; ++e2) { const ptmi_d2 v = rp[4 * e2]; dq[2 * e2] = v.x; dq[2 * e2 + 1] = v.y; }
                if (EPL & 1) dq[EPL - 1] = row[8 * (EPL / 2) + gl];
            } else {
                if constexpr (ULDS) {
#pragma unroll
                    for (int e = 0; e < EPL; ++e) PTMI_ROW_LOAD(dq[e], smem + (size_t)sd.k * d, e);
                } else {
                    if constexpr (UPAD) {                          // the library's zero-padded copy: no bounds to check
                        // a base per 4 KB of the row (wave-uniform at 64 lanes: scalar adds), so that every load is base + the
                        // lane's offset + an immediate; beyond the 13-bit immediate the compiler kept one offset register per slot
                        const double *col = a.UtPad + (size_t)sd.k * (G * EPL) + gl;
                        constexpr int SPB = 512 / G;                // slots per 4 KB
#pragma unroll
                        for (int e = 0; e < EPL; ++e) {
                            const double *base = col + (e / SPB) * 512;
                            dq[e] = base[G * (e % SPB)];
                        }
                        // every request of the row goes out before the first product: left alone the scheduler, short of registers,
                        // issued ten of the sixteen loads one at a time, each behind a wait for the one before
                        __builtin_amdgcn_sched_barrier(0);
                    } else {
                        const double *col = UtBlock + (size_t)sd.k * d;
#pragma unroll
                        for (int e = 0; e < EPL; ++e) PTMI_ROW_LOAD(dq[e], col, e);
                    }
                }
            }
            if constexpr (SV < 0) {
#pragma unroll
                for (int e = 0; e < EPL; ++e) dq[e] = sd.amp * dq[e];
            }
            scam_amp = sd.amp;
        } else {
        Draws dr;
        draws_for_step<STR, FULL, TM, GW>(batch, dr, a, k, sid, sid0, gl, tsm);
        log_u = dr.log_u;
        if (ULDS && ulds_box) jt = propose<G, EPL, FULL, STR, GRP>(a, it, sid, gl, cc, dr, smem, false, S, DE, dq, false);
        else if (ULDS) jt = propose<G, EPL, FULL, STR, GRP>(a, it, sid, gl, cc, dr, smem, false, smem + d * d, DE, dq, true);
        else if (STAGE && FULL && (UT_ALWAYS_LDS || a.lds_u)) jt = propose<G, EPL, FULL, STR, GRP>(a, it, sid, gl, cc, dr, PTMI_UL, true, PTMI_SQ, DE, dq, true, !amq_on, tsm);
        else if (STAGE && FULL) jt = propose<G, EPL, FULL, STR, GRP>(a, it, sid, gl, cc, dr, UtBlock, false, PTMI_SQ, DE, dq, true, !amq_on, tsm);
        else jt = propose<G, EPL, FULL, STR, GRP>(a, it, sid, gl, cc, dr, UtBlock, false, S, DE, dq, false, true, nullptr, &am_next);
        }
        if constexpr (AMQ) {
            // the rank of this chain's event of this step is held by its lane of row (k & 3)
            const int rk = __shfl(rank_c, 16 * (k & 3) + (lane & 15), 64);
            if (amq_on && jt == PTMI_J_AM) {
#pragma unroll
                for (int e = 0; e < EPL; ++e) dq[e] = PTMI_AMQ(rk & 15)[gl * EPL + e];
            }
        }
        if (FULL) {
#pragma unroll
            for (int j = 0; j < PTMI_J_FUSED; ++j) jp[j] += (jt == j);
        }
        // PT:605-612
        double nlp, nlnL = 0.0, nlnprob;
        {
            double q[EPL];
#pragma unroll
            for (int e = 0; e < EPL; ++e) q[e] = x[e] + dq[e];
            if constexpr (PRI == PTMI_LOGP_FLAT) nlp = 0.0;
            else if constexpr (BOXFAST) {
                box_reach = __builtin_fabs(scam_amp) * box_umax;
                bool inside = box_reach < box_margin;
                if (!inside) {                   // (divergent between the wave's chains; rare in a box wider than the jumps)
                    bool in1;
                    double mg, bm;
                    box_test_and_margin<G, EPL>(smem, a.box_off, gl, x, dq, in1, mg, bm);
                    inside = grp_all<G, STR>(in1);
                    box_margin = grp_min<G, STR>(mg) * (1.0 - 0x1.0p-40);
                    box_guard = -grp_min<G, STR>(-bm) * 0x1.0p-52;
                }
                nlp = inside ? 0.0 : -__builtin_inf();
            }
            else if constexpr (PERS != 0 && PRI == PTMI_LOGP_BOX)
                nlp = grp_all<G, STR>(box_inside_lds<G, EPL>(smem, a.box_off, gl, [&](int e) { return q[e]; })) ? 0.0 : -__builtin_inf();
            else nlp = eval_logp<G, EPL, STR>(a, q, gl, smem);
            // the reference skips logl when the prior is -inf (PT:607-608); the value is unused then, and the
            // matrix-core path needs every lane, so it is evaluated unconditionally
            if (STAGE) nlnL = eval_logl<G, EPL, LOGL, STR>(a, q, gl, PTMI_PL);
            else nlnL = eval_logl<G, EPL, LOGL, STR>(a, q, gl, PtG);
            nlnprob = nlp == -__builtin_inf() ? -__builtin_inf() : beta * nlnL + nlp;
        }
        // PT:615-622
        const double lnprob0 = beta * lnL + lp;
        const double diff = nlnprob - lnprob0 + 0.0;
        const bool accepted = diff > log_u;
        if (accepted) {
            // x + dq again (bit-identical to q); keeping q alive instead would cost EPL more registers
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                double inc = dq[e];
                asm volatile("" : "+v"(inc));
                x[e] = x[e] + inc;
            }
            lnL = nlnL;
            lp = nlp;
            nacc += 1;
            if (FULL) {
#pragma unroll
                for (int j = 0; j < PTMI_J_FUSED; ++j) ja[j] += (jt == j);
            }
            // no element moved further than the reach plus the rounding of its sum (relative to the ELEMENT, which a bound limits: the
            // slack factors alone are relative to the margin, and a narrow box far from the origin has a margin far below |x| 2^-13)
            if constexpr (BOXFAST) box_margin = (box_margin - box_reach - box_guard) * (1.0 - 0x1.0p-40);
        }
        // PT:327-328 (the post-swap row of a swap iteration is written by the swap).  These 25 stores of four active lanes, in ONE
        // wave of every block, are 15 % of the config-2 kernel (0.90 -> 0.77 ms without them, in a measurement build): the wave is
        // its block's straggler.  Sending the row through LDS and out as two coalesced stores of the whole wave was built twice -- stored
        // in the same step, and one step late so that no wait sits on the critical path -- and measured slower both times (1.00 ms).
        // Round 3 (persistent blocks, cold-first walk): 0.783 ms with the stores, 0.751 with every row of a walker sent to ONE
        // cache-resident row, 0.697 without them.  Units of 16 rank-0 chains of 16 different walkers -- the
        // same rows as 13 stores of a FULL wave in one unit of 64 instead of 13 four-lane stores in one unit of four -- measured
        // 0.780 against 0.778: the cost is the bytes through the CU's store path (1.28 MB per CU and launch) and the scattered
        // 64-byte writes behind it, not the issue slots of the instructions.
        if (cold && !(a.swap_last && k == a.nsteps - 1)) {
            am_store_step<G, EPL>(a, w, am_row, k, x, gl, d, accepted);
            if (a.AMaux && gl == 0) {
                double *ax = a.AMaux + ((size_t)w * a.cov_update + (size_t)am_row) * 2;
                ax[0] = lnL;
                ax[1] = lp;
            }
        }
        am_row = am_row + 1 == a.cov_update ? 0 : am_row + 1;
