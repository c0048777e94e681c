/* ssw_k5_firstpass.inc -- device: first_pass_kernel, first_pass_big_kernel, first_pass_win_kernel.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */
/* ---------------------------------------------------------------------------------- */
/* K5: first pass of forced alignment (SURVEY 8(f) row 4)                               */
/*   fsg_search_start / _step      src/fsg_search.c:747-802, 665-745                     */
/*   fsg_search_hmm_eval, _hmm_prune_prop, _pnode_trans, _pnode_exit, _word_trans        */
/*                                 src/fsg_search.c:331-402, 498-541, 404-435, 437-490, 598-662 */
/*   fsg_search_find_exit, fsg_search_seg_iter   src/fsg_search.c:854-925, 1085-1143     */
/* One workgroup per utterance, one thread per phone-tree HMM (ssw_fsg.c; texts of more    */
/* than 1024 HMMs take the long-text kernels below), its state in registers; a frame is    */
/* three phases with two LDS-only workgroup barriers between them:                         */
/*   A  hmm_vit_eval of the active nodes, best score of the frame                        */
/*   B  every node offers its exit score to its successors, leaves that pass the word     */
/*      beam publish a word exit                                                         */
/*   C  every node looks at its ONE predecessor (phone transition into it), every word-   */
/*      initial node takes the best exit that entered its FSG state (cross-word           */
/*      transition, context sets checked), then the node settles whether it stays active, */
/*      as the reference's active lists would have it                                     */
/* Node-centric instead of list-driven: a node has one predecessor in the tree, and a      */
/* word-initial node takes the best compatible exit, which is what the reference's        */
/* "first strictly better score wins" loops compute.  Exact score ties that do occur --    */
/* alternates pronounced alike -- follow the reference's list order (twin_first_in_list,  */
/* ssw_search_common.inc, which holds the decisions the three kernels of this file share); */
/* any other tie goes to the entering leaf with the lowest (context phone, ordinal).       */
/* The reference's history table drops exits whose right contexts are covered              */
/* by better ones (src/fsg_history.c:129-205); that only removes candidates that could not */
/* win, so here every exit keeps a slot: entry id = 1 + frame * n_leaves + leaf.           */
/* ---------------------------------------------------------------------------------- */
struct FirstPassParams {
    const int16_t *senscr; /* [n_frames][n_sen] */
    const int *utt_off, *node_off, *leaf_off, *state_off;
    const uint16_t *senid; /* [n_nodes][4] */
    const int *pen, *parent;
    const uint32_t *info;
    const unsigned long long *ctxt;
    const int *leaf_ord, *leaf_wid, *leaf_to, *leaf_node, *in_off, *in_leaf;
    const int *tw, *tw_off, *twin_ref, *tw_rk; /* alternates pronounced alike, ssw_internal.h */
    const uint32_t *tp; /* [n_tmat][3] rows of 4 uint8 */
    int2 *hist;              /* (predecessor entry, exit score) of every (frame, leaf) slot */
    const long long *hist_off; /* [n_utts] */
    int *n_seg;
    ssw_word_seg_t *seg;
    int n_sen, max_seg, beam, pbeam, wbeam, sil;
    int *big_ws;              /* first_pass_big_kernel: node state and exchange arrays in HBM */
    const long long *big_off; /* [n_utts] offset (ints) of the utterance's part of big_ws */
    int hist_band;            /* first_pass_big_kernel<.., true>: history entries per frame (budget) */
    const int *only;          /* NULL, or the utterances this launch searches (one workgroup each):
                               * what a level left unfinished, searched again one level down */
    /* first_pass_kernel<.., EXPORT> (the default configuration as a batch, ssw_host_fpactive.inc):
     * the set of HMMs every frame evaluates -- what fsg_search_sen_active hands acmod before the
     * frame is scored (src/fsg_search.c:310-325, :677-680) -- a bit per phone-tree HMM,
     * [n_frames_u][(N_u + 63) / 64] words at act_off[u] */
    unsigned long long *act_mask;
    const long long *act_off; /* [n_utts] */
};

/* threads: at most TPB phone-tree HMMs; EXPORT: the sets of active HMMs written out */
template <int TPB, bool EXPORT = false>
__global__ void __launch_bounds__(TPB)
first_pass_kernel(FirstPassParams P)
{
    extern __shared__ int fp_lds[];
    const int u = P.only != NULL ? P.only[blockIdx.x] : (int)blockIdx.x, tid = threadIdx.x;
    const int nb = P.node_off[u], N = P.node_off[u + 1] - nb;
    const int lb = P.leaf_off[u], NL = P.leaf_off[u + 1] - lb;
    const int sb = P.state_off[u], NS = P.state_off[u + 1] - sb;
    const int f0 = P.utt_off[u], T = P.utt_off[u + 1] - f0;
    const int W = SSW_WORST_SCORE;
    /* A node's HMM lives in its thread's registers.  LDS only carries what another node
     * reads: XS / XH, the exit score and history a node offers its successors this frame
     * (INT_MIN when it does not pass the beams); EXJ, the word exits of the frame in the order
     * of the per-state entering lists; IL, three ints per list entry (il_pack). */
    int *XS = fp_lds, *XH = XS + N, *EXJ = XH + N, *IL = EXJ + NL;
    /* FLG: how each node came through the frame (for the twins' order bookkeeping); TW: the
     * utterance's twin records; RK: their rank buffers */
    const int NTW = P.tw_off[u + 1] - P.tw_off[u], NRK = P.tw_rk[u];
    int *FLG = IL + 3 * NL, *TW = FLG + N, *RK = TW + NTW;
    /* SMAX: best word exit into each FSG state this frame, double-buffered by frame parity */
    int *SMAX = RK + NRK;
    __shared__ int s_red[TPB / 64], s_any[2], s_final_id;
    const uint16_t *senid = P.senid + (size_t)nb * 4;
    const int *pen = P.pen + nb, *parent = P.parent + nb, *leaf_ord = P.leaf_ord + nb;
    const uint32_t *info = P.info + nb;
    const unsigned long long *ctxt = P.ctxt + nb;
    const int *leaf_node = P.leaf_node + lb;
    const int *in_off = P.in_off + sb;
    const int j_base = in_off[0];
    int2 *hist = P.hist + P.hist_off[u];

    /* list slot of every leaf (EXJ is used as scratch for the inverse map) */
    for (int j = tid; j < NL; j += TPB) {
        const int lo = P.in_leaf[j_base + j], ln = leaf_node[lo];
        il_pack(IL, j, (uint32_t)lo, info[ln], ctxt[ln]);
        EXJ[lo] = j;
    }
    search_tables_init<TPB>(TW, P.tw + P.tw_off[u], NTW, RK, NRK, SMAX, 2 * NS, tid);
    if (tid == 0) {
        s_final_id = -1;
        s_any[0] = s_any[1] = 0;
    }
    if (tid < TPB / 64)
        s_red[tid] = W; /* waves that leave below never write their slot */
    __syncthreads();

    /* the thread's node: constants, HMM, and the two sets of score dwords in flight */
    const int n = tid;
    const bool v = n < N;
    const int nn = v ? n : 0;
    const int r_parent = v ? parent[nn] : -1, r_pen = pen[nn], r_leaf = v ? leaf_ord[nn] : -1;
    const int r_slot = r_leaf >= 0 ? EXJ[r_leaf] : 0, r_to = r_leaf >= 0 ? P.leaf_to[lb + r_leaf] : 0;
    const uint32_t r_info = v ? info[nn] : 0u;
    const unsigned long long r_ctxt = ctxt[nn];
    const int r_st = (int)(r_info >> 16);
    const int r_j0 = (r_info & FP_ROOT) ? in_off[r_st] - j_base : 0;
    const int r_j1 = (r_info & FP_ROOT) ? in_off[r_st + 1] - j_base : 0;
    const uint16_t *sn = senid + (size_t)nn * 4;
    const uint32_t sen01 = (uint32_t)sn[0] | ((uint32_t)sn[1] << 16);
    const uint32_t sen2t = (uint32_t)sn[2] | ((uint32_t)sn[3] << 16);
    const uint32_t *tp = P.tp + (size_t)sn[3] * 3;
    const uint32_t tpa = tp[0], tpb = tp[1], tpc = tp[2];
    uint32_t nx0 = 0, nx1 = 0, nx2 = 0, ny0 = 0, ny1 = 0, ny2 = 0;
    if (T > 0) { /* (uniform) */
        scores_request(P.senscr, f0, 0, T, P.n_sen, sen01, sen2t, nx0, nx1, nx2);
        scores_request(P.senscr, f0, 1, T, P.n_sen, sen01, sen2t, ny0, ny1, ny2);
    }
    int s0 = W, s1 = W, s2 = W, os = W, bsc = W, h0 = -1, h1 = -1, h2 = -1, oh = -1;
    const int r_twin = v ? P.twin_ref[nb + nn] : -1; /* offset of the node's twin record in TW, -1 */
    bool act = v && search_start_text(r_info, r_ctxt, r_pen, P.sil, P.beam, s0, h0);
    if (v)
        FLG[n] = act ? (FP_F_NEXT | FP_F_ENTW) : 0;
    __syncthreads(); /* EXJ scratch has been read */
    /* The workgroup is sized for the batch's largest utterance; waves without a single HMM of
     * THIS utterance leave now, so the frame loop's barriers wait for fewer waves (a finished
     * wave no longer counts at s_barrier). */
    if ((tid & ~63) >= N)
        return;

    auto frame = [&](const int f, uint32_t &q0, uint32_t &q1, uint32_t &q2) {
        if (EXPORT) { /* (every wave that is still here owns a word of the frame's mask) */
            const unsigned long long bm = __ballot(act);
            if ((tid & 63) == 0)
                P.act_mask[P.act_off[u] + (long long)f * ((N + 63) >> 6) + (tid >> 6)] = bm;
        }
        int c0, c1, c2;
        scores_take(P.senscr, f0, f, T, P.n_sen, sen01, sen2t, q0, q1, q2, c0, c1, c2);
        /* A: hmm_vit_eval of the active nodes, best score of the frame */
        int bs = W;
        if (act) {
            bsc = vit_eval_3st(s0, s1, s2, h0, h1, h2, os, oh, -c0, -c1, -c2, tpa, tpb, tpc);
            bs = bsc;
        }
        beams_publish(s_red, bs, tid);
        lds_barrier();
        const FrameBeams bm = beams_read<TPB>(s_red, P.beam, P.pbeam, P.wbeam);
        const int thresh = bm.thresh, pth = bm.pth, wth = bm.wth;

        /* B: every node offers its exit to its successors; leaves that pass the word beam
         * publish a word exit (fsg_search_hmm_prune_prop) */
        const bool keep = act && bsc >= thresh;
        int any = 0;
        if (n < NS)
            SMAX[((f + 1) & 1) * NS + n] = FP_NO_EXIT; /* next frame's buffer */
        if (v) {
            XS[n] = (keep && os >= pth) ? os : INT_MIN;
            XH[n] = oh;
            if (r_leaf >= 0) {
                bool ex = keep && os >= wth;
                if (r_twin >= 0)
                    ex = twin_first_in_list(TW + r_twin, RK, FLG, f) && ex;
                EXJ[r_slot] = ex ? os : FP_NO_EXIT;
                if (ex) {
                    hist[(size_t)f * NL + r_leaf] = make_int2(oh, os);
                    atomicMax(&SMAX[(f & 1) * NS + r_to], os);
                    any = 1;
                }
            }
        }
        if (any)
            s_any[f & 1] = 1;
        lds_barrier();

        /* C: phone transition into every node from its one predecessor, cross-word
         * transition into every word-initial node from the exits that entered its state, then
         * the node settles whether it stays active */
        if (v) {
            const int p = r_parent >= 0 ? r_parent : 0;
            const int mx = (r_info & FP_ROOT) ? SMAX[(f & 1) * NS + r_st] : FP_NO_EXIT;
            const int ent = node_enter(r_parent >= 0, XS[p], XH[p], mx, r_pen, thresh, 1 + f * NL, s0, h0,
                                       [&](int &be, int &bid) {
                                           best_entry<false>(EXJ, IL, r_j0, r_j1, r_ctxt,
                                                             (int)((r_info >> 8) & 0xff), be, bid);
                                       });
            settle_regs(act, keep, ent, FLG[n], s0, s1, s2, h0, h1, h2, os, oh, bsc);
        }
        /* fsg_search_find_exit looks at the LAST frame that has any exit, and only at exits
         * into the final state */
        if (tid == 0) {
            if (s_any[f & 1]) {
                int be;
                const int bid = final_exit<false>(EXJ, IL, in_off[NS - 1] - j_base, in_off[NS] - j_base, be);
                s_final_id = bid >= 0 ? 1 + f * NL + bid : -1;
            }
            s_any[(f + 1) & 1] = 0;
        }
        /* no barrier here: the next frame writes XS / EXJ only after its own first barrier,
         * which every reader above has to reach first */
    };
    for (int f = 0; f < T; f += 2) { /* (T is the same in every wave of the group: barriers) */
        frame(f, nx0, nx1, nx2);
        if (f + 1 < T)
            frame(f + 1, ny0, ny1, ny2);
    }
    __syncthreads(); /* the exits written to HBM during the loop are read back below */

    if (tid == 0) /* (the identity map: every (frame, leaf) has its slot) */
        P.n_seg[u] = fp_write_segments(hist, [](int k) { return (size_t)(k - 1); }, s_final_id, NL,
                                       P.leaf_wid + lb, P.seg + (size_t)u * P.max_seg, P.max_seg);
}

/* K5 for texts beyond what one workgroup holds in registers and LDS (more than 4096 phone-tree
 * HMMs, or exchange arrays beyond 160 KB): the same three phases per frame, same decisions in
 * the same order, but every thread walks its nodes (n = tid, tid + TPB, ...) and the node state
 * and the exchange arrays live in a per-utterance HBM workspace (L2-resident: ~70 bytes per
 * HMM).  The barriers are full __syncthreads() here: they order the global traffic of the
 * workgroup as well.  Layout of the workspace (ints): 13 arrays of N (s0 s1 s2 h0 h1 h2 os oh
 * bsc act xs xh flg) | EXJ[NL] | IL[3 NL] | SLOT[NL] | TW | RK | SMAX[2 NS].
 * A 2,000-word page is ~19 K HMMs and ~8 K word-final ones. */
/* BAND (round 3, VERDICT r2 item 7): a frame walks only the nodes of the grammar states between
 * the first and the last state that had an active node in the previous frame, plus one state
 * (the grammar is linear: a word leads to the next state, a filler stays; nodes and word-final
 * HMMs are numbered state by state), and the history table keeps, per frame, only the word-final
 * HMMs of those states: FBASE[f] + leaf - FLLO[f] instead of f * n_leaves + leaf.  A 2,000-word
 * page walked 19,443 nodes per frame for an active band of a few hundred, and its [frame][leaf]
 * table took 6 GB.  Entry ids stay 1 + frame * n_leaves + leaf.  When the banded table's budget
 * (P.hist_band entries per frame on average) runs out the utterance reports n_seg = -(1 << 30)
 * and the host runs the batch again with BAND = false. */
template <int TPB, bool BAND>
__global__ void __launch_bounds__(TPB)
first_pass_big_kernel(FirstPassParams P)
{
    const int u = P.only != NULL ? P.only[blockIdx.x] : (int)blockIdx.x, tid = threadIdx.x;
    const int nb = P.node_off[u], N = P.node_off[u + 1] - nb;
    const int lb = P.leaf_off[u], NL = P.leaf_off[u + 1] - lb;
    const int sb = P.state_off[u], NS = P.state_off[u + 1] - sb;
    const int f0 = P.utt_off[u], T = P.utt_off[u + 1] - f0;
    const int W = SSW_WORST_SCORE;
    const int NTW = P.tw_off[u + 1] - P.tw_off[u], NRK = P.tw_rk[u];
    int *ws = P.big_ws + P.big_off[u];
    int *S0 = ws, *S1 = S0 + N, *S2 = S1 + N, *H0 = S2 + N, *H1 = H0 + N, *H2 = H1 + N;
    int *OS = H2 + N, *OH = OS + N, *BSC = OH + N, *ACT = BSC + N;
    int *XS = ACT + N, *XH = XS + N, *FLG = XH + N;
    int *EXJ = FLG + N, *IL = EXJ + NL, *SLOT = IL + 3 * NL;
    int *TW = SLOT + NL, *RK = TW + NTW, *SMAX = RK + NRK;
    /* BAND: first node / first word-final HMM of every state (+ 2 sentinels), per-frame base
     * and first leaf of the history rows */
    int *SFIRST = SMAX + 2 * NS, *LFIRST = SFIRST + NS + 2, *FBASE = LFIRST + NS + 2, *FLLO = FBASE + T + 1;
    __shared__ int s_red[TPB / 64], s_any[2], s_final_id, s_blo[2], s_bhi[2], s_ovf;
    const uint16_t *senid = P.senid + (size_t)nb * 4;
    const int *pen = P.pen + nb, *parent = P.parent + nb, *leaf_ord = P.leaf_ord + nb;
    const uint32_t *info = P.info + nb;
    const unsigned long long *ctxt = P.ctxt + nb;
    const int *leaf_node = P.leaf_node + lb, *leaf_to = P.leaf_to + lb;
    const int *twin_ref = P.twin_ref + nb;
    const int *in_off = P.in_off + sb;
    const int j_base = in_off[0];
    int2 *hist = P.hist + P.hist_off[u];

    for (int j = tid; j < NL; j += TPB) {
        const int lo = P.in_leaf[j_base + j], ln = leaf_node[lo];
        il_pack(IL, j, (uint32_t)lo, info[ln], ctxt[ln]);
        SLOT[lo] = j;
        EXJ[j] = FP_NO_EXIT;
    }
    search_tables_init<TPB>(TW, P.tw + P.tw_off[u], NTW, RK, NRK, SMAX, 2 * NS, tid);
    if (tid == 0) {
        s_final_id = -1;
        s_any[0] = s_any[1] = 0;
        s_blo[0] = s_blo[1] = INT_MAX;
        s_bhi[0] = s_bhi[1] = -1;
        s_ovf = 0;
    }
    if (BAND) {
        for (int i = tid; i < NS + 2; i += TPB) {
            SFIRST[i] = N;
            LFIRST[i] = NL;
        }
        __syncthreads();
        for (int n = tid; n < N; n += TPB) {
            const int st = (int)(info[n] >> 16);
            atomicMin(&SFIRST[st], n);
            if (leaf_ord[n] >= 0)
                atomicMin(&LFIRST[st], leaf_ord[n]);
        }
        __syncthreads();
        if (tid == 0) /* a state without nodes / leaves of its own starts where the next one does */
            for (int i = NS - 1; i >= 0; --i) {
                SFIRST[i] = SFIRST[i] < SFIRST[i + 1] ? SFIRST[i] : SFIRST[i + 1];
                LFIRST[i] = LFIRST[i] < LFIRST[i + 1] ? LFIRST[i] : LFIRST[i + 1];
            }
    }
    for (int n = tid; n < N; n += TPB) {
        int s0 = W, h0 = -1;
        const int a = search_start_text(info[n], ctxt[n], pen[n], P.sil, P.beam, s0, h0);
        S0[n] = s0;
        S1[n] = S2[n] = OS[n] = BSC[n] = W;
        H0[n] = h0;
        H1[n] = H2[n] = OH[n] = -1;
        ACT[n] = a;
        XS[n] = INT_MIN;
        XH[n] = -1;
        FLG[n] = a ? (FP_F_NEXT | FP_F_ENTW) : 0;
    }
    __syncthreads();

    /* BAND: the states walked in this frame, [blo, bhi] (bhi already includes the state a word of
     * the last active state leads to); node n stays with thread n % TPB whatever the band */
    int blo = 0, bhi = NS > 1 ? 1 : 0;
    long long hbase = 0; /* history entries used by the frames before this one */
    const long long hcap = BAND ? (long long)T * P.hist_band : 0;
    for (int f = 0; f < T; ++f) {
        const int nbeg = BAND ? (SFIRST[blo] / TPB) * TPB : 0;
        const int nend = BAND ? SFIRST[bhi + 1 < NS + 1 ? bhi + 1 : NS + 1] : N;
        const int llo = BAND ? LFIRST[blo] : 0;
        const int lw = BAND ? LFIRST[bhi + 1 < NS + 1 ? bhi + 1 : NS + 1] - llo : NL;
        if (BAND && tid == 0) {
            FBASE[f] = (int)hbase;
            FLLO[f] = llo;
            if (hbase + lw > hcap)
                s_ovf = 1;
        }
        /* A: hmm_vit_eval of the active nodes, best score of the frame */
        const uint16_t *urow =
            reinterpret_cast<const uint16_t *>(P.senscr + (size_t)(f0 + f) * P.n_sen);
        int bs = W;
        int alo = INT_MAX, ahi = -1; /* states of this thread's active nodes */
        for (int n = nbeg + tid; n < nend; n += TPB) {
            if (!(ACT[n] & 1))
                continue;
            if (P.act_mask != nullptr) /* (rows cleared before the launch) */
                atomicOr(P.act_mask + P.act_off[u] + (long long)f * ((N + 63) >> 6) + (n >> 6),
                         1ull << (n & 63));
            if (BAND) {
                const int st = (int)(info[n] >> 16);
                alo = st < alo ? st : alo;
                ahi = st > ahi ? st : ahi;
            }
            const uint16_t *sn = senid + (size_t)n * 4;
            const uint32_t *tp = P.tp + (size_t)sn[3] * 3;
            int s0 = S0[n], s1 = S1[n], s2 = S2[n], h0 = H0[n], h1 = H1[n], h2 = H2[n];
            int os = OS[n], oh = OH[n];
            const int c0 = (int)(short)urow[sn[0]], c1 = (int)(short)urow[sn[1]],
                      c2 = (int)(short)urow[sn[2]];
            const int b = vit_eval_3st(s0, s1, s2, h0, h1, h2, os, oh, -c0, -c1, -c2, tp[0], tp[1],
                                       tp[2]);
            S0[n] = s0, S1[n] = s1, S2[n] = s2, H0[n] = h0, H1[n] = h1, H2[n] = h2;
            OS[n] = os, OH[n] = oh, BSC[n] = b;
            bs = b > bs ? b : bs;
        }
        beams_publish(s_red, bs, tid);
        if (BAND) {
            alo = -wave_max_dpp(-alo);
            ahi = wave_max_dpp(ahi);
            if ((tid & 63) == 0 && ahi >= 0) {
                atomicMin(&s_blo[f & 1], alo);
                atomicMax(&s_bhi[f & 1], ahi);
            }
        }
        __syncthreads();
        if (BAND && s_ovf)
            break; /* (uniform) the banded history table is full: reported below */
        /* the next frame's band: the states active in this one, and one more */
        const int nblo = BAND ? s_blo[f & 1] : 0, nbhi = BAND ? s_bhi[f & 1] : 0;
        if (BAND && tid == 0) {
            s_blo[(f + 1) & 1] = INT_MAX;
            s_bhi[(f + 1) & 1] = -1;
        }
        const FrameBeams bm = beams_read<TPB>(s_red, P.beam, P.pbeam, P.wbeam);
        const int thresh = bm.thresh, pth = bm.pth, wth = bm.wth;

        /* B: exits offered to successors, word exits published */
        int any = 0;
        if (BAND) /* the exit maxima the next frame collects: only these states can get one */
            for (int st = blo + tid; st <= bhi + 1 && st < NS; st += TPB)
                SMAX[((f + 1) & 1) * NS + st] = FP_NO_EXIT;
        for (int n = nbeg + tid; n < nend; n += TPB) {
            if (!BAND && n < NS)
                SMAX[((f + 1) & 1) * NS + n] = FP_NO_EXIT;
            const int a = ACT[n] & 1;
            const int lo = leaf_ord[n];
            if (!a) { /* nothing to offer; a leaf's slot may still hold last frame's exit */
                XS[n] = INT_MIN;
                if (lo >= 0) {
                    EXJ[SLOT[lo]] = FP_NO_EXIT;
                    if (twin_ref[n] >= 0) /* every member keeps the group's order up to date */
                        (void)twin_first_in_list(TW + twin_ref[n], RK, FLG, f);
                }
                continue;
            }
            const int os = OS[n], oh = OH[n];
            const bool keep = BSC[n] >= thresh;
            ACT[n] = 1 | (keep ? 2 : 0);
            XS[n] = (keep && os >= pth) ? os : INT_MIN;
            XH[n] = oh;
            if (lo >= 0) {
                bool ex = keep && os >= wth;
                const int tw = twin_ref[n];
                if (tw >= 0)
                    ex = twin_first_in_list(TW + tw, RK, FLG, f) && ex;
                EXJ[SLOT[lo]] = ex ? os : FP_NO_EXIT;
                if (ex) {
                    hist[BAND ? (size_t)(hbase + lo - llo) : (size_t)f * NL + lo] = make_int2(oh, os);
                    atomicMax(&SMAX[(f & 1) * NS + leaf_to[lo]], os);
                    any = 1;
                }
            }
        }
        if (!BAND && NS > N) /* cannot happen (every state has a filler HMM), kept for safety */
            for (int n = N + tid; n < NS; n += TPB)
                SMAX[((f + 1) & 1) * NS + n] = FP_NO_EXIT;
        if (any)
            s_any[f & 1] = 1;
        __syncthreads();

        /* C: phone transitions, cross-word transitions, activity */
        for (int n = nbeg + tid; n < nend; n += TPB) {
            const int par = parent[n];
            const uint32_t inf = info[n];
            const int actf = ACT[n];
            const bool act = actf & 1, keep = (actf & 2) != 0;
            int xs = INT_MIN, xh = -1;
            if (par >= 0) {
                xs = XS[par];
                xh = XH[par];
            }
            int mx = FP_NO_EXIT;
            if (inf & FP_ROOT)
                mx = SMAX[(f & 1) * NS + (int)(inf >> 16)];
            if (!act && xs == INT_MIN && mx == FP_NO_EXIT) {
                if (FLG[n] != 0)
                    FLG[n] = 0;
                continue;
            }
            const int pn = pen[n];
            int s0 = S0[n], h0 = H0[n];
            const int ent = node_enter(par >= 0, xs, xh, mx, pn, thresh, 1 + f * NL, s0, h0,
                                       [&](int &be, int &bid) {
                                           const int d = (int)(inf >> 16);
                                           best_entry<false>(EXJ, IL, in_off[d] - j_base, in_off[d + 1] - j_base,
                                                             ctxt[n], (int)((inf >> 8) & 0xff), be, bid);
                                       });
            const bool stay = settle(keep, ent, FLG[n]);
            if (ent) {
                S0[n] = s0;
                H0[n] = h0;
            }
            if (act && !stay) { /* fsg_psubtree_pnode_deactivate -> hmm_clear */
                S0[n] = S1[n] = S2[n] = OS[n] = BSC[n] = W;
                H0[n] = H1[n] = H2[n] = OH[n] = -1;
            }
            ACT[n] = stay ? 1 : 0;
        }
        if (tid == 0) {
            if (s_any[f & 1]) {
                int be;
                const int bid = final_exit<false>(EXJ, IL, in_off[NS - 1] - j_base, in_off[NS] - j_base, be);
                s_final_id = bid >= 0 ? 1 + f * NL + bid : -1;
            }
            s_any[(f + 1) & 1] = 0;
        }
        /* the next frame's phase A touches a thread's own nodes only; XS / EXJ are rewritten
         * after its barrier, which every reader above has to reach first */
        if (BAND) {
            hbase += lw;
            if (nbhi >= 0) {
                blo = nblo;
                bhi = nbhi + 1 < NS ? nbhi + 1 : NS - 1;
            } else { /* nothing was active: nothing can be entered any more */
                blo = 0;
                bhi = -1;
            }
        }
    }
    __syncthreads();

    if (tid == 0) {
        auto at = [&](int k) -> size_t { /* entry id -> its slot */
            if (!BAND)
                return (size_t)(k - 1);
            const int fr = (k - 1) / NL, lo = (k - 1) % NL;
            return (size_t)(FBASE[fr] + lo - FLLO[fr]);
        };
        P.n_seg[u] = (BAND && s_ovf) ? -(1 << 30)
                                     : fp_write_segments(hist, at, s_final_id, NL, P.leaf_wid + lb,
                                                         P.seg + (size_t)u * P.max_seg, P.max_seg);
    }
}

/* Round 3: K5 for long texts with the HMMs IN REGISTERS -- first_pass_kernel's frame on a sliding
 * window of TPB nodes.  first_pass_big_kernel keeps every node's state in HBM and pays three
 * dependent round trips to L2 per frame (3.6 us per frame on a 2,000-word page, whose active
 * band is a few dozen nodes of 19,443).  Here thread tid holds the one node n of the window
 * [wlo, wlo + TPB) with n = tid (mod TPB): constants and HMM in registers, the senone scores of
 * the next two frames in flight, as in first_pass_kernel.  The grammar is linear and nodes are
 * numbered state by state, so the active nodes only move up: once the lowest active state has
 * passed a wave's nodes (wlo = first node of the lowest active state, rounded down to a
 * multiple of 64) its threads take the nodes TPB further on -- constants reloaded, HMM cleared.
 * What other nodes read goes through LDS RINGS: XS / XH / FLG by node (slot = n mod TPB = tid),
 * the word exits EXJ by list slot (mod 2 TPB), the per-state exit maximum by state (mod TPB);
 * a slot that leaves the window holds "no exit" (its node was inactive in its last frame there),
 * so a slot that enters needs no clearing.  The history table is banded as in
 * first_pass_big_kernel<.., true> (FBASE / FLLO).  Whatever does not fit -- active nodes
 * further apart than TPB, entering lists beyond 2 TPB slots, the history budget -- ends the
 * utterance with n_seg = -(1 << 30), and the host runs the batch through first_pass_big_kernel.
 * Workspace (the big kernel's layout, only these parts used): IL | SLOT | TW | RK | SFIRST |
 * LFIRST | FBASE | FLLO. */
template <int TPB>
__global__ void __launch_bounds__(TPB)
first_pass_win_kernel(FirstPassParams P)
{
    constexpr int NM = TPB - 1, EW = 2 * TPB, EM = EW - 1;
    __shared__ int XS[TPB], XH[TPB], FLG[TPB], EXJ[EW], SMAX[2 * TPB];
    __shared__ int s_red[TPB / 64], s_any[2], s_anyf[2], s_final_id, s_ovf;
    __shared__ int s_nlo[2], s_nhi[2];        /* lowest / highest active node of the frame */
    __shared__ int s_b[2][6];                 /* its bounds: wlo whi llo lhi jlo jhi */
    const int u = P.only != NULL ? P.only[blockIdx.x] : (int)blockIdx.x, tid = threadIdx.x;
    const int nb = P.node_off[u], N = P.node_off[u + 1] - nb;
    const int lb = P.leaf_off[u], NL = P.leaf_off[u + 1] - lb;
    const int sb = P.state_off[u], NS = P.state_off[u + 1] - sb;
    const int f0 = P.utt_off[u], T = P.utt_off[u + 1] - f0;
    const int W = SSW_WORST_SCORE;
    const int NTW = P.tw_off[u + 1] - P.tw_off[u], NRK = P.tw_rk[u];
    int *ws = P.big_ws + P.big_off[u];
    int *IL = ws + 13 * (size_t)N + NL, *SLOT = IL + 3 * NL;
    int *TW = SLOT + NL, *RK = TW + NTW, *SFIRST = RK + NRK + 2 * NS, *LFIRST = SFIRST + NS + 2,
        *FBASE = LFIRST + NS + 2, *FLLO = FBASE + T + 1;
    const uint16_t *senid = P.senid + (size_t)nb * 4;
    const int *pen = P.pen + nb, *parent = P.parent + nb, *leaf_ord = P.leaf_ord + nb;
    const uint32_t *info = P.info + nb;
    const unsigned long long *ctxt = P.ctxt + nb;
    const int *leaf_node = P.leaf_node + lb, *leaf_to = P.leaf_to + lb;
    const int *in_off = P.in_off + sb;
    const int j_base = in_off[0];
    int2 *hist = P.hist + P.hist_off[u];

    /* workspace tables, as in first_pass_big_kernel */
    for (int j = tid; j < NL; j += TPB) {
        const int lo = P.in_leaf[j_base + j], ln = leaf_node[lo];
        il_pack(IL, j, (uint32_t)lo, info[ln], ctxt[ln]);
        SLOT[lo] = j;
    }
    search_tables_init<TPB>(TW, P.tw + P.tw_off[u], NTW, RK, NRK, SMAX, 2 * TPB, tid);
    for (int i = tid; i < NS + 2; i += TPB) {
        SFIRST[i] = N;
        LFIRST[i] = NL;
    }
    for (int i = tid; i < EW; i += TPB)
        EXJ[i] = FP_NO_EXIT;
    FLG[tid] = 0;
    XS[tid] = INT_MIN;
    XH[tid] = -1;
    if (tid == 0) {
        s_final_id = -1;
        s_any[0] = s_any[1] = s_anyf[0] = s_anyf[1] = 0;
        s_nlo[0] = s_nlo[1] = INT_MAX;
        s_nhi[0] = s_nhi[1] = -1;
        s_ovf = 0;
    }
    if (tid < TPB / 64)
        s_red[tid] = W;
    __syncthreads();
    for (int n = tid; n < N; n += TPB) {
        const int st = (int)(info[n] >> 16);
        atomicMin(&SFIRST[st], n);
        if (leaf_ord[n] >= 0)
            atomicMin(&LFIRST[st], leaf_ord[n]);
    }
    __syncthreads();
    if (tid == 0)
        for (int i = NS - 1; i >= 0; --i) {
            SFIRST[i] = SFIRST[i] < SFIRST[i + 1] ? SFIRST[i] : SFIRST[i + 1];
            LFIRST[i] = LFIRST[i] < LFIRST[i + 1] ? LFIRST[i] : LFIRST[i + 1];
        }
    __syncthreads();

    /* the thread's node */
    int n = tid;
    bool v = false, act = false, had_exit = false;
    int s0 = W, s1 = W, s2 = W, h0 = -1, h1 = -1, h2 = -1, os = W, oh = -1, bsc = W;
    int r_twin = -1, r_parent = -1, r_pen = 0, r_leaf = -1, r_slot = 0, r_j0 = 0, r_j1 = 0, r_to = 0;
    int r_st = 0, r_wlo = 0, r_whi = 0, r_llo = 0, r_lhi = 0, r_jlo = 0, r_jhi = 0;
    uint32_t r_info = 0, sen01 = 0, sen2t = 0, tpa = 0, tpb = 0, tpc = 0;
    unsigned long long r_ctxt = 0;
    uint32_t nx0 = 0, nx1 = 0, nx2 = 0, ny0 = 0, ny1 = 0, ny2 = 0;
    auto load_node = [&](int nn_) { /* constants in, hmm_clear; FLG / SMAX slots of a fresh node */
        n = nn_;
        v = n < N;
        const int nn = v ? n : 0;
        r_parent = v ? parent[nn] : -1;
        r_pen = pen[nn];
        r_leaf = v ? leaf_ord[nn] : -1;
        r_slot = r_leaf >= 0 ? SLOT[r_leaf] : 0;
        r_to = r_leaf >= 0 ? leaf_to[r_leaf] : 0;
        r_info = v ? info[nn] : 0u;
        r_ctxt = ctxt[nn];
        r_st = (int)(r_info >> 16);
        /* list slots a frame can touch when this is its lowest / highest active node: the lists
         * of this state .. of the state three further on (an active leaf's word exits one state
         * on, the frame after it may have moved one more state on and still clears a slot) */
        const int d = r_st, d2 = d + 2 < NS + 1 ? d + 2 : NS + 1, dj2 = d + 4 < NS ? d + 4 : NS;
        r_j0 = (r_info & FP_ROOT) ? in_off[d] - j_base : 0;
        r_j1 = (r_info & FP_ROOT) ? in_off[d + 1] - j_base : 0;
        r_wlo = SFIRST[d];
        r_whi = SFIRST[d2];
        r_llo = LFIRST[d];
        r_lhi = LFIRST[d2];
        r_jlo = in_off[d] - j_base;
        r_jhi = in_off[dj2] - j_base;
        const uint16_t *sn = senid + (size_t)nn * 4;
        sen01 = (uint32_t)sn[0] | ((uint32_t)sn[1] << 16);
        sen2t = (uint32_t)sn[2] | ((uint32_t)sn[3] << 16);
        const uint32_t *tp = P.tp + (size_t)sn[3] * 3;
        tpa = tp[0];
        tpb = tp[1];
        tpc = tp[2];
        r_twin = v ? P.twin_ref[nb + nn] : -1;
        s0 = s1 = s2 = os = bsc = W;
        h0 = h1 = h2 = oh = -1;
        act = false;
        had_exit = false;
    };
    auto load_scores = [&](int f, uint32_t &q0, uint32_t &q1, uint32_t &q2) {
        scores_request(P.senscr, f0, f, T, P.n_sen, sen01, sen2t, q0, q1, q2);
    };
    load_node(n);
    if (T > 0) {
        load_scores(0, nx0, nx1, nx2);
        load_scores(1, ny0, ny1, ny2);
    }
    act = v && search_start_text(r_info, r_ctxt, r_pen, P.sil, P.beam, s0, h0);
    FLG[tid] = act ? (FP_F_NEXT | FP_F_ENTW) : 0;
    /* the band the first frame's exits can come from: states 0 and 1 */
    int llo = 0, lw = LFIRST[NS > 2 ? 2 : NS] - 0;
    long long hbase = 0;
    const long long hcap = (long long)T * P.hist_band;
    int wlo = 0; /* the window's first node (a multiple of 64) */
    __syncthreads();
    /* (a start that needs more than the window: let the big kernel do it) */
    if (SFIRST[NS > 2 ? 2 : NS] > TPB || in_off[NS > 2 ? 2 : NS] - j_base > EW) {
        if (tid == 0)
            P.n_seg[u] = -(1 << 30);
        return;
    }

    auto frame = [&](const int f, uint32_t &q0, uint32_t &q1, uint32_t &q2, uint32_t &o0,
                     uint32_t &o1, uint32_t &o2) {
        const int par = f & 1;
        int c0, c1, c2;
        scores_take(P.senscr, f0, f, T, P.n_sen, sen01, sen2t, q0, q1, q2, c0, c1, c2);
        if (tid == 0) {
            FBASE[f] = (int)hbase;
            FLLO[f] = llo;
            if (hbase + lw > hcap)
                s_ovf = 1;
            s_nlo[par ^ 1] = INT_MAX;
            s_nhi[par ^ 1] = -1;
        }
        /* A */
        int bs = W;
        if (act) {
            bsc = vit_eval_3st(s0, s1, s2, h0, h1, h2, os, oh, -c0, -c1, -c2, tpa, tpb, tpc);
            bs = bsc;
        }
        beams_publish(s_red, bs, tid);
        /* a wave's nodes are consecutive (whole waves move on together): n = n0 + lane */
        const unsigned long long am = __ballot(act);
        const int n0 = n - (tid & 63);
        const int amin = am ? n0 + __builtin_ctzll(am) : INT_MAX;
        const int amax = am ? n0 + 63 - __builtin_clzll(am) : -1;
        if ((tid & 63) == 0 && amax >= 0) {
            atomicMin(&s_nlo[par], amin);
            atomicMax(&s_nhi[par], amax);
            /* the frame's set of active HMMs (ssw_host_fpactive.inc; the rows were cleared
             * before the launch: a word no wave writes stays 0) */
            if (P.act_mask != nullptr)
                P.act_mask[P.act_off[u] + (long long)f * ((N + 63) >> 6) + (n0 >> 6)] = am;
        }
        lds_barrier();
        const FrameBeams bm = beams_read<TPB>(s_red, P.beam, P.pbeam, P.wbeam);
        const int thresh = bm.thresh, pth = bm.pth, wth = bm.wth;
        const int nlo = s_nlo[par], nhi = s_nhi[par];
        const bool stop = s_ovf != 0;
        if (v && n == nlo) {
            s_b[par][0] = r_wlo;
            s_b[par][2] = r_llo;
            s_b[par][4] = r_jlo;
        }
        if (v && n == nhi) {
            s_b[par][1] = r_whi;
            s_b[par][3] = r_lhi;
            s_b[par][5] = r_jhi;
        }

        /* B */
        const bool keep = act && bsc >= thresh;
        int any = 0, anyf = 0;
        if (v) {
            SMAX[(par ^ 1) * TPB + (r_st & NM)] = FP_NO_EXIT; /* next frame's buffer */
            XS[tid] = (keep && os >= pth) ? os : INT_MIN;
            XH[tid] = oh;
            if (r_leaf >= 0) {
                bool ex = keep && os >= wth;
                if (r_twin >= 0)
                    ex = twin_first_in_list(TW + r_twin, RK, FLG, f, NM) && ex;
                /* the slot is written by an active leaf and cleared the frame after its last
                 * exit; an idle leaf leaves the ring alone (its slot may be another's by now) */
                if (act || had_exit)
                    EXJ[r_slot & EM] = ex ? os : FP_NO_EXIT;
                had_exit = ex;
                if (ex && !stop) {
                    hist[(size_t)(hbase + r_leaf - llo)] = make_int2(oh, os);
                    atomicMax(&SMAX[par * TPB + (r_to & NM)], os);
                    any = 1;
                    anyf = r_to == NS - 1;
                }
            }
        } else
            XS[tid] = INT_MIN;
        if (any)
            s_any[par] = 1;
        if (anyf)
            s_anyf[par] = 1;
        lds_barrier();

        /* C */
        if (v) {
            const int pp = r_parent >= 0 ? (r_parent & NM) : 0;
            const int mx = (r_info & FP_ROOT) ? SMAX[par * TPB + (r_st & NM)] : FP_NO_EXIT;
            const int ent = node_enter(r_parent >= 0, XS[pp], XH[pp], mx, r_pen, thresh, 1 + f * NL, s0, h0,
                                       [&](int &be, int &bid) {
                                           best_entry<false>(EXJ, IL, r_j0, r_j1, r_ctxt,
                                                             (int)((r_info >> 8) & 0xff), be, bid, EM);
                                       });
            settle_regs(act, keep, ent, FLG[tid], s0, s1, s2, h0, h1, h2, os, oh, bsc);
        }
        if (tid == 0) {
            if (s_any[par]) {
                int be, bid = -1;
                if (s_anyf[par]) /* (then the final state's entering list is inside the ring) */
                    bid = final_exit<false>(EXJ, IL, in_off[NS - 1] - j_base, in_off[NS] - j_base, be, EM);
                s_final_id = bid >= 0 ? 1 + f * NL + bid : -1;
            }
            s_any[par ^ 1] = 0;
            s_anyf[par ^ 1] = 0;
        }
        /* the next frame's band and window, from the nodes that were active in this one */
        hbase += lw;
        if (nhi >= 0) {
            const int b_wlo = s_b[par][0], b_whi = s_b[par][1], b_jlo = s_b[par][4],
                      b_jhi = s_b[par][5];
            llo = s_b[par][2];
            lw = s_b[par][3] - llo;
            const int nwlo = b_wlo & ~63;
            if (b_whi - nwlo > TPB || b_jhi - b_jlo > EW) {
                if (tid == 0)
                    s_ovf = 1;
            } else if (nwlo > wlo) {
                wlo = nwlo;
                if (n < wlo) { /* (whole waves: wlo and n - tid are multiples of 64) */
                    const int steps = (wlo - n + TPB - 1) / TPB;
                    load_node(n + steps * TPB);
                    FLG[tid] = 0;
                    if (v)
                        SMAX[(par ^ 1) * TPB + (r_st & NM)] = FP_NO_EXIT;
                    load_scores(f + 1, o0, o1, o2);
                    load_scores(f + 2, q0, q1, q2);
                }
            }
        } else
            lw = 0; /* nothing is active: nothing can exit any more */
        return stop;
    };
    bool stop = false;
    for (int f = 0; f < T && !stop; f += 2) {
        stop = frame(f, nx0, nx1, nx2, ny0, ny1, ny2);
        if (f + 1 < T && !stop)
            stop = frame(f + 1, ny0, ny1, ny2, nx0, nx1, nx2);
    }
    __syncthreads();

    if (tid == 0) {
        auto at = [&](int k) -> size_t { /* banded as in first_pass_big_kernel<.., true> */
            const int fr = (k - 1) / NL, lo = (k - 1) % NL;
            return (size_t)(FBASE[fr] + lo - FLLO[fr]);
        };
        P.n_seg[u] = s_ovf ? -(1 << 30)
                           : fp_write_segments(hist, at, s_final_id, NL, P.leaf_wid + lb,
                                               P.seg + (size_t)u * P.max_seg, P.max_seg);
    }
}
