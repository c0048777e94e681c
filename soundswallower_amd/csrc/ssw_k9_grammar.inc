/* ssw_k9_grammar.inc -- device: grammar_search_kernel, grammar_search_big_kernel.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */
/* ---------------------------------------------------------------------------------- */
/* K9: recognition against a word FSG (decoder_set_fsg)                                 */
/*   fsg_search_start             src/fsg_search.c:747-798                               */
/*   fsg_search_step and its parts  :331-402, 404-435, 437-490, 498-541, 598-662, 665-739 */
/*   fsg_search_null_prop         :543-591                                               */
/*   fsg_search_find_exit (final), fsg_seg_bp2itor, fsg_search_seg_iter                   */
/*                                :854-924, 1033-1055, 1085-1142                         */
/* The design of K5 (ssw_k5_firstpass.inc): one workgroup per utterance, one thread per    */
/* phone-tree HMM with its state in registers, a frame in three phases with two LDS-only   */
/* barriers.  What a grammar adds to the linear text:                                      */
/*   - any start and final state;                                                         */
/*   - null transitions.  The grammar holds their transitive closure, so a word exit into  */
/*     state s reaches, in the same frame, exactly the states one null hop from s, and the */
/*     set of hops per state is static.  The host folds them into the states' entering     */
/*     lists: a list entry (SLOT) is a word-final HMM that leads into the state, or a pair  */
/*     (word-final HMM into s, null s -> state) with the null's log probability.  In phase  */
/*     B a word-final HMM writes its exit score into every one of its slots (plus the       */
/*     penalty, kept only if >= best + wbeam, as fsg_search_null_prop keeps it); phase C    */
/*     is K5's: a word-initial HMM takes the best compatible slot of its state's list.      */
/*     No extra barrier, no extra LDS round trip in phase C.                               */
/*   - history: entry id = 1 + (frame + 1) * NE + slot (NE slots per grammar, row 0 is      */
/*     frame -1: the null transitions out of the start state); a null slot's entry has the  */
/*     word exit's entry of the same frame as its predecessor, as in the reference.         */
/* Ties.  A word-initial HMM takes the first strictly better entry in history order        */
/* (fsg_search_word_trans); fsg_search_find_exit takes the oldest of the best entries into  */
/* the final state.  The reference files a frame's word exits by (state, left context) and  */
/* adds the null entries after them; the lists here are in that order -- word exits by      */
/* (left-context phone, ordinal), then null hops by the same key -- and both scans take the  */
/* first of equals.  Alternates pronounced alike follow K5's twin records.                  */
/* The default configuration (compallsen = no; ssw_recognize_batch_active, host half in           */
/* ssw_host_grammar.inc).  grammar_search_kernel<.., EXPORT> writes, for every frame f, one bit per */
/* phone-tree HMM: set iff the HMM is in the reference's pnode_active when fsg_search_step(f)       */
/* starts (hmm_frame == f) -- the list fsg_search_sen_active walks before the frame is scored       */
/* (src/fsg_search.c:310-325, :676-679).  Frame 0's set is what fsg_search_start leaves: the roots   */
/* of the start state and of the states its null transitions reach (:775-787).  Here that is act[]  */
/* as the frame begins.  HMM n = tid + k TPB is bit (tid & 63) of word (tid >> 6) + k (TPB / 64) of  */
/* the frame's row, that is bit n of the row: one wave ballot per k writes a whole word, with any    */
/* number of HMMs per thread.                                                                        */
/* The proof in the header of ssw_k7_fpactive.inc never looks at the shape of the grammar.  It needs */
/* (a) that a frame's search reads only the scores of the senones of the HMMs active as it starts,   */
/* and (b) that the sets of frame f + 1 are a function of those scores and the state after frame f.  */
/* Both hold for any word FSG, nulls and loops included: phase A evaluates the active HMMs alone,    */
/* and everything phases B and C decide follows from phase A's results and the static tables.  So    */
/* an utterance whose exported sets equal the assumed ones frame for frame has been searched on the  */
/* reference's scores, and any other is right up to and including the set of its first differing     */
/* frame.                                                                                            */
/* ---------------------------------------------------------------------------------- */
struct GrammarParams {
    const int16_t *senscr; /* [n_frames][n_sen] */
    const int *utt_off;    /* [n_utts + 1] */
    const int *fsg_of_utt; /* [n_utts] or NULL: grammar 0 */
    const int *node_off, *leaf_off, *state_off; /* [n_fsgs + 1] */
    const uint16_t *senid; /* [n_nodes][4] */
    const int *pen, *parent;
    const uint32_t *info;
    const unsigned long long *ctxt;
    const int *leaf_ord, *leaf_wid, *leaf_node, *leaf_lscr;
    const int *slot_off; /* [n_states + 1] */
    const int *slot_leaf, *slot_pen, *slot_null, *slot_state;
    const int *ls_off, *ls_slot;
    const int *g_start, *g_final, *sn_off, *sn_to, *sn_pen;
    const int *tw, *tw_off, *twin_ref, *tw_rk;
    const uint32_t *tp; /* [n_tmat][3] rows of 4 uint8 */
    int2 *hist;               /* (predecessor entry, score) of every (frame + 1, slot) */
    const long long *hist_off; /* [n_utts] */
    int *n_seg, *score;       /* [n_utts]: segments (-1 no match, -2 no entry at all, -(3 + k): k
                                 segments do not fit), hypothesis score */
    ssw_fsg_seg_t *seg;       /* [n_utts][max_seg] */
    int n_sen, max_seg, beam, pbeam, wbeam, sil;
    /* the EXPORT instances (grammar_search_kernel, grammar_search_big_kernel) only: */
    const int *only;              /* NULL, or the utterances this launch searches (one workgroup
                                     each): the ones a round has not proven yet */
    unsigned long long *act_mask; /* [n_frames_u][(N + 63) / 64] words at act_off[u]; cleared
                                     before a launch of grammar_search_kernel (fpa_clear_kernel),
                                     written whole by grammar_search_big_kernel */
    const long long *act_off;     /* [n_utts] */
};

/* what a phase needs of a node's constants: in registers with one HMM per thread, read again
 * from HBM (L2-resident) every frame with more */
struct GrNodeA {
    uint32_t sen01, sen2t, tpa, tpb, tpc;
};
struct GrNodeB {
    int leaf, ls0, ls1, twin;
};
struct GrNodeC {
    int parent, pen, j0, j1;
    uint32_t info;
    unsigned long long ctxt;
};

/* with several HMMs per thread: keeps the compiler from fetching the constants of all of them
 * ahead of the first one's work (their constants beside their state would not fit a lane's
 * registers) */
#define GR_ONE_AT_A_TIME() asm volatile("" ::: "memory")

template <int NPT, int TPB, bool EXPORT = false> /* HMMs per thread, threads, the sets of active HMMs written out */
__global__ void __launch_bounds__(TPB)
grammar_search_kernel(GrammarParams P)
{
    extern __shared__ int gr_lds[];
    const int u = (EXPORT && P.only != NULL) ? P.only[blockIdx.x] : (int)blockIdx.x, tid = threadIdx.x;
    const int gi = P.fsg_of_utt != NULL ? P.fsg_of_utt[u] : 0;
    const int nb = P.node_off[gi], N = P.node_off[gi + 1] - nb;
    const int lb = P.leaf_off[gi];
    const int sb = P.state_off[gi], NS = P.state_off[gi + 1] - sb;
    const int f0 = P.utt_off[u], T = P.utt_off[u + 1] - f0;
    const int W = SSW_WORST_SCORE;
    const int *slot_off = P.slot_off + sb;
    const int j_base = slot_off[0], NE = slot_off[NS] - j_base;
    const int snb = P.sn_off[gi], NSN = P.sn_off[gi + 1] - snb;
    const int ROW = NE > NSN ? (NE > 0 ? NE : 1) : NSN; /* history entries per frame */
    const int start = P.g_start[gi], fin = P.g_final[gi];
    /* LDS: XS / XH the exit a node offers its successors; FLG how it came through the frame
     * (twins); EXJ the frame's entries by slot; IL three ints per slot (left-context phone shown |
     * "any right context", right-context set); LS two ints per (leaf, slot): slot | state << 16,
     * penalty; TW / RK the twin records; SMAX best entry into each state, by frame parity */
    const int NTW = P.tw_off[gi + 1] - P.tw_off[gi], NRK = P.tw_rk[gi];
    int *XS = gr_lds, *XH = XS + N, *FLG = XH + N, *EXJ = FLG + N, *IL = EXJ + NE;
    int *LS = IL + 3 * NE, *TW = LS + 2 * NE, *RK = TW + NTW, *SMAX = RK + NRK;
    __shared__ int s_red[TPB / 64], s_any[2], s_final_id, s_final_score, s_have;
    const uint16_t *senid = P.senid + (size_t)nb * 4;
    const int *pen = P.pen + nb, *parent = P.parent + nb, *leaf_ord = P.leaf_ord + nb;
    const uint32_t *info = P.info + nb;
    const unsigned long long *ctxt = P.ctxt + nb;
    const int *leaf_node = P.leaf_node + lb;
    const int *ls_off = P.ls_off + lb;
    const int ls_base = ls_off[0];
    int2 *hist = P.hist + P.hist_off[u];

    for (int j = tid; j < NE; j += TPB) {
        const int lo = P.slot_leaf[j_base + j], ln = leaf_node[lo];
        il_pack(IL, j, 0u, info[ln], ctxt[ln]);
        EXJ[j] = FP_NO_EXIT;
        /* (a leaf's slots are ls_slot[ls_off[leaf] ..): NE of them in all */
        const int sj = P.ls_slot[ls_base + j];
        LS[2 * j] = sj | (P.slot_state[j_base + sj] << 16);
        LS[2 * j + 1] = P.slot_pen[j_base + sj];
    }
    for (int i = tid; i < NTW; i += TPB)
        TW[i] = P.tw[P.tw_off[gi] + i];
    for (int i = tid; i < NRK; i += TPB)
        RK[i] = FP_RANK_NONE;
    for (int i = tid; i < 2 * NS; i += TPB)
        SMAX[i] = FP_NO_EXIT;
    if (tid == 0) {
        /* fsg_search_start: the null transitions out of the start state are history entries of
         * frame -1 (kept under 0 + wbeam), row 0 of the table; the best of them into the final
         * state is what find_exit returns when no word ever exits */
        int be = INT_MIN, bid = -1, have = 0;
        for (int k = 0; k < NSN; ++k) {
            const int sc = P.sn_pen[snb + k];
            hist[k] = make_int2(0, sc);
            if (sc >= P.wbeam) {
                have = 1;
                if (P.sn_to[snb + k] == fin && sc > be) {
                    be = sc;
                    bid = 1 + k;
                }
            }
        }
        s_final_id = bid;
        s_final_score = be;
        s_have = have;
        s_any[0] = s_any[1] = 0;
    }
    if (tid < TPB / 64)
        s_red[tid] = W; /* waves that leave below never write their slot */

    auto node_a = [&](int n) {
        const uint16_t *sn = senid + (size_t)n * 4;
        const uint32_t *tp = P.tp + (size_t)sn[3] * 3;
        return GrNodeA{ (uint32_t)sn[0] | ((uint32_t)sn[1] << 16),
                        (uint32_t)sn[2] | ((uint32_t)sn[3] << 16), tp[0], tp[1], tp[2] };
    };
    auto node_b = [&](int n) {
        const int lf = leaf_ord[n];
        const int l = lf >= 0 ? lf : 0;
        return GrNodeB{ lf, ls_off[l] - ls_base, ls_off[l + 1] - ls_base, P.twin_ref[nb + n] };
    };
    auto node_c = [&](int n) {
        const uint32_t inf = info[n];
        const int d = (int)(inf >> 16);
        const bool root = (inf & FP_ROOT) != 0;
        return GrNodeC{ parent[n], pen[n], root ? slot_off[d] - j_base : 0,
                        root ? slot_off[d + 1] - j_base : 0, inf, ctxt[n] };
    };

    int s0[NPT], s1[NPT], s2[NPT], h0[NPT], h1[NPT], h2[NPT], os[NPT], oh[NPT], bsc[NPT];
    bool act[NPT];
    /* one HMM per thread: its constants stay in registers, and so do the dwords that hold its
     * next two frames' scores (K5: frame f's are requested at the top of frame f - 2) */
    GrNodeA ra = {};
    GrNodeB rb = {};
    GrNodeC rc = {};
    uint32_t nx0 = 0, nx1 = 0, nx2 = 0, ny0 = 0, ny1 = 0, ny2 = 0;
    if (NPT == 1) {
        const int nn = tid < N ? tid : 0;
        ra = node_a(nn);
        rb = node_b(nn);
        rc = node_c(nn);
        if (tid >= N) {
            rb.leaf = -1;
            rb.twin = -1;
            rc.parent = -1;
            rc.info = 0u;
            rc.j0 = rc.j1 = 0;
        }
        if (T > 0) { /* (uniform) */
            scores_request(P.senscr, f0, 0, T, P.n_sen, ra.sen01, ra.sen2t, nx0, nx1, nx2);
            scores_request(P.senscr, f0, 1, T, P.n_sen, ra.sen01, ra.sen2t, ny0, ny1, ny2);
        }
    }
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        const int n = tid + k * TPB;
        const bool v = n < N;
        s0[k] = s1[k] = s2[k] = os[k] = bsc[k] = W;
        h0[k] = h1[k] = h2[k] = oh[k] = -1;
        act[k] = false;
        if (v) {
            const GrNodeC c = NPT == 1 ? rc : node_c(n);
            /* fsg_search_start: the dummy entry 0 (score 0, left context SIL, every right
             * context), then the entries null_prop made of it, enter the word-initial HMMs of
             * their states under beam alone; the first strictly better one stays */
            if ((c.info & FP_ROOT) && ((c.ctxt >> P.sil) & 1)) {
                const int d = (int)(c.info >> 16);
                if (d == start && c.pen > P.beam && c.pen > s0[k]) {
                    s0[k] = c.pen;
                    h0[k] = 0;
                    act[k] = true;
                }
                for (int q = 0; q < NSN; ++q) {
                    const int sc = P.sn_pen[snb + q];
                    if (P.sn_to[snb + q] == d && sc >= P.wbeam && sc + c.pen > P.beam
                        && sc + c.pen > s0[k]) {
                        s0[k] = sc + c.pen;
                        h0[k] = 1 + q;
                        act[k] = true;
                    }
                }
            }
            FLG[n] = act[k] ? (FP_F_NEXT | FP_F_ENTW) : 0;
        }
    }
    __syncthreads();
    /* waves without a single HMM of THIS grammar leave now (K5) */
    if ((tid & ~63) >= N && tid >= 64) /* (the first wave stays: it writes the result) */
        return;
    const int alive = N <= 64 ? 64 : ((N + 63) & ~63) < TPB ? ((N + 63) & ~63) : TPB; /* threads that stay */

    auto frame = [&](const int f, uint32_t &q0, uint32_t &q1, uint32_t &q2) {
        const ScoreRow rf = score_row(P.senscr, (size_t)(f0 + f) * P.n_sen);
        if (EXPORT) {
            /* the HMMs active as the frame starts: what fsg_search_sen_active hands acmod.  Every
             * wave is whole here (the lanes beyond N hold act = false) */
            const int MW = (N + 63) >> 6;
            unsigned long long *row = P.act_mask + P.act_off[u] + (long long)f * MW;
#pragma unroll
            for (int k = 0; k < NPT; ++k) {
                const unsigned long long bm = __ballot(act[k]);
                const int word = (tid >> 6) + k * (TPB / 64);
                if ((tid & 63) == 0 && word < MW)
                    row[word] = bm;
            }
        }
        /* A: hmm_vit_eval of the active nodes, best score of the frame */
        int bs = W;
        if (NPT == 1) {
            /* the empty asm pins the wait for this frame's loads HERE (K5) */
            uint32_t a = q0, b = q1, c = q2;
            asm volatile("" : "+v"(a), "+v"(b), "+v"(c));
            const int c0 = score_of(a, rf.lo, ra.sen01 & 0xffff);
            const int c1 = score_of(b, rf.lo, ra.sen01 >> 16);
            const int c2 = score_of(c, rf.lo, ra.sen2t & 0xffff);
            const int fn = f + 2 < T ? f + 2 : T - 1;
            const ScoreRow rn = score_row(P.senscr, (size_t)(f0 + fn) * P.n_sen);
            q0 = score_dword(rn, ra.sen01 & 0xffff);
            q1 = score_dword(rn, ra.sen01 >> 16);
            q2 = score_dword(rn, ra.sen2t & 0xffff);
            if (act[0]) {
                bsc[0] = vit_eval_3st(s0[0], s1[0], s2[0], h0[0], h1[0], h2[0], os[0], oh[0], -c0,
                                      -c1, -c2, ra.tpa, ra.tpb, ra.tpc);
                bs = bsc[0];
            }
        } else {
            /* several HMMs per thread: one after the other, the constants and the scores of the
             * active ones fetched as they come (registers for four HMMs' state, not for their
             * constants as well) */
#pragma unroll
            for (int k = 0; k < NPT; ++k) {
                if (act[k]) {
                    const GrNodeA na = node_a(tid + k * TPB);
                    const int c0 = score_of(score_dword(rf, na.sen01 & 0xffff), rf.lo, na.sen01 & 0xffff);
                    const int c1 = score_of(score_dword(rf, na.sen01 >> 16), rf.lo, na.sen01 >> 16);
                    const int c2 = score_of(score_dword(rf, na.sen2t & 0xffff), rf.lo, na.sen2t & 0xffff);
                    bsc[k] = vit_eval_3st(s0[k], s1[k], s2[k], h0[k], h1[k], h2[k], os[k], oh[k],
                                          -c0, -c1, -c2, na.tpa, na.tpb, na.tpc);
                    bs = bsc[k] > bs ? bsc[k] : bs;
                }
                GR_ONE_AT_A_TIME();
            }
        }
        bs = wave_max_dpp(bs);
        if ((tid & 63) == 0)
            s_red[tid >> 6] = bs;
        lds_barrier();
        int best = s_red[0];
#pragma unroll
        for (int k = 1; k < TPB / 64; ++k)
            best = s_red[k] > best ? s_red[k] : best;
        const int thresh = best + P.beam, pth = best + P.pbeam, wth = best + P.wbeam;

        /* B: every node offers its exit to its successors; a word-final HMM that passes the
         * word beam files a word exit, and from it one entry per null transition out of the
         * state it leads to (fsg_search_hmm_prune_prop, fsg_search_null_prop) */
        bool keep[NPT];
        int any = 0;
        const int hrow = (f + 1) * ROW;
        for (int i = tid; i < NS; i += alive) /* next frame's buffer */
            SMAX[((f + 1) & 1) * NS + i] = FP_NO_EXIT;
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const int n = tid + k * TPB;
            keep[k] = act[k] && bsc[k] >= thresh;
            if (n < N) {
                const GrNodeB b = NPT == 1 ? rb : node_b(n);
                XS[n] = (keep[k] && os[k] >= pth) ? os[k] : INT_MIN;
                XH[n] = oh[k];
                if (b.leaf >= 0) {
                    bool ex = keep[k] && os[k] >= wth;
                    if (b.twin >= 0)
                        ex = twin_first_in_list(TW + b.twin, RK, FLG, f) && ex;
                    int id0 = 0;
                    for (int i = b.ls0; i < b.ls1; ++i) {
                        const int w = LS[2 * i], j = w & 0xffff;
                        const int sc = os[k] + LS[2 * i + 1];
                        /* (the word exit's own slot comes first, with penalty 0) */
                        const bool in = ex && sc >= wth;
                        EXJ[j] = in ? sc : FP_NO_EXIT;
                        if (in) {
                            hist[(size_t)hrow + j] = make_int2(i == b.ls0 ? oh[k] : id0, sc);
                            atomicMax(&SMAX[(f & 1) * NS + (int)((uint32_t)w >> 16)], sc);
                        }
                        if (i == b.ls0)
                            id0 = 1 + hrow + j;
                    }
                    any |= ex ? 1 : 0;
                }
            }
            if (NPT > 1)
                GR_ONE_AT_A_TIME();
        }
        if (any)
            s_any[f & 1] = 1;
        lds_barrier();

        /* C: phone transition into every node from its one predecessor, cross-word transition
         * into every word-initial node from the entries into its state, then the node settles
         * whether it stays active */
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const int n = tid + k * TPB;
            if (n >= N)
                continue;
            if (NPT > 1)
                GR_ONE_AT_A_TIME();
            const GrNodeC c = NPT == 1 ? rc : node_c(n);
            bool entered = false, entered_p = false, entered_w = false;
            const int p = c.parent >= 0 ? c.parent : 0;
            const int xs = XS[p], xh = XH[p];
            if (c.parent >= 0 && xs != INT_MIN) {
                const int ns = xs + c.pen;
                if (ns > thresh && ns > s0[k]) {
                    s0[k] = ns; /* hmm_enter */
                    h0[k] = xh;
                    entered = entered_p = true;
                }
            }
            if (c.info & FP_ROOT) {
                const int mx = SMAX[(f & 1) * NS + (int)(c.info >> 16)];
                if (mx != FP_NO_EXIT && mx + c.pen > thresh && mx + c.pen > s0[k]) {
                    const int ci = (int)((c.info >> 8) & 0xff);
                    int be, bid;
                    best_entry<true>(EXJ, IL, c.j0, c.j1, c.ctxt, ci, be, bid);
                    if (bid >= 0) {
                        const int ns = be + c.pen;
                        if (ns > thresh && ns > s0[k]) {
                            s0[k] = ns;
                            h0[k] = 1 + hrow + bid;
                            entered = entered_w = true;
                        }
                    }
                }
            }
            const bool stay = keep[k] || entered;
            FLG[n] = (stay ? FP_F_NEXT : 0) | (keep[k] ? FP_F_KEEP : 0)
                | (entered_p ? FP_F_ENTP : 0) | (entered_w ? FP_F_ENTW : 0);
            if (act[k] && !stay) { /* fsg_psubtree_pnode_deactivate -> hmm_clear */
                s0[k] = s1[k] = s2[k] = os[k] = bsc[k] = W;
                h0[k] = h1[k] = h2[k] = oh[k] = -1;
            }
            act[k] = stay;
        }
        /* fsg_search_find_exit, final: the LAST frame that has any entry, the best entry into
         * the final state, null entries included; of equals the oldest (first in the list) */
        if (tid == 0) {
            if (s_any[f & 1]) {
                int be = INT_MIN, bid = -1;
                for (int j = slot_off[fin] - j_base; j < slot_off[fin + 1] - j_base; ++j)
                    if (EXJ[j] != FP_NO_EXIT && EXJ[j] > be) {
                        be = EXJ[j];
                        bid = j;
                    }
                s_final_id = bid >= 0 ? 1 + hrow + bid : -1;
                s_final_score = be;
                s_have = 1;
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
    __syncthreads(); /* the entries written to HBM during the loop are read back below */

    /* fsg_search_seg_iter + fsg_seg_bp2itor: walk the predecessors back, then write the entries
     * in order.  Entry id -> row (id - 1) / ROW = frame + 1, slot (id - 1) % ROW. */
    if (tid == 0) {
        int id = s_final_id, n = 0;
        ssw_fsg_seg_t *seg = P.seg + (size_t)u * P.max_seg;
        if (id < 0)
            n = s_have ? -1 : -2;
        else {
            for (int k = id; k > 0; k = hist[k - 1].x)
                ++n;
            if (n > P.max_seg)
                n = -(3 + n);
            else {
                int j = n - 1;
                for (int k = id; k > 0; k = hist[k - 1].x, --j) {
                    const int row = (k - 1) / ROW, sl = (k - 1) % ROW;
                    const int2 e = hist[k - 1];
                    const int pk = e.x;
                    const int pscore = pk > 0 ? hist[pk - 1].y : 0;
                    const int ef = row - 1;
                    int sf = pk > 0 ? (pk - 1) / ROW : 0; /* predecessor's frame + 1 */
                    sf = sf > ef ? ef : sf;
                    int wid = -1, lscr;
                    if (row == 0)
                        lscr = P.sn_pen[snb + sl];
                    else if (P.slot_null[j_base + sl])
                        lscr = P.slot_pen[j_base + sl];
                    else {
                        const int lo = P.slot_leaf[j_base + sl];
                        wid = P.leaf_wid[lb + lo];
                        lscr = P.leaf_lscr[lb + lo];
                    }
                    seg[j].wid = wid;
                    seg[j].sf = sf;
                    seg[j].ef = ef;
                    seg[j].lscr = lscr;
                    seg[j].ascr = e.y - pscore - lscr;
                }
            }
            P.score[u] = s_final_score;
        }
        P.n_seg[u] = n;
    }
}

/* K9 for grammars beyond what one workgroup holds in registers and LDS (more than 4096 phone-tree
 * HMMs, or exchange arrays beyond 160 KB; ssw_grammar_prepare_large): the same three phases per
 * frame, the same decisions in the same order, but every thread walks its nodes (n = tid, tid +
 * TPB, ...) and the node state and the exchange arrays live in a per-utterance HBM workspace
 * (L2-resident), as in first_pass_big_kernel.  The barriers are full __syncthreads(): they order
 * the workgroup's global traffic as well, and every thread reaches every one of them.
 * Layout of the workspace (ints): 13 arrays of N (s0 s1 s2 h0 h1 h2 os oh bsc act xs xh flg) |
 * IL[3 NE] | LS[3 NE] (slot, state, penalty: no 16-bit packing) | TW | RK | SMAX[2 NS] |
 * TWL[NTW / 4 + 1] | FL[3 NE].
 * A frame of such a grammar has hundreds of active HMMs among thousands and about ten history
 * entries among thousands of slots, and the work follows that:
 *   - the walks over all N nodes read act[] alone; constants, scores and state are fetched for
 *     active nodes only (phase C reads a node's parent and info as well: whether it is entered
 *     depends on them).  act bit 0: active; bit 1: kept by the beam (phase B -> C); bit 2: the
 *     node was deactivated with an exit on offer, which the next phase B withdraws -- an inactive
 *     node has XS = INT_MIN by that, and is not touched otherwise;
 *   - there is no EXJ: phase B appends every entry it files to the frame's list FL (slot, score,
 *     state; count in LDS, by frame parity), a word-initial HMM scans that list instead of its
 *     state's slots, and so does fsg_search_find_exit.  The list is in no order, so of equal
 *     scores the lowest slot wins explicitly: the first in the reference's history order, the one
 *     the dense scan meets first;
 *   - the rank buffers of a twin group need every member's call in every frame: the inactive
 *     members are called from TWL, the list of twin leaves made once, not found by a walk.
 * The default configuration (EXPORT; see the header of this file): phase A's walk is where the
 * frame begins, and ACT[n] & 1 as it finds it is the reference's pnode_active -- a node with bit 2
 * alone was deactivated in the frame before and is not in it; frame 0 finds what the start-up code
 * left.  With n = tid + k TPB a wave's 64 lanes hold the 64 consecutive nodes of one word of the
 * frame's row, so one ballot per trip is that word: no atomics.  The exporting walk makes the same
 * number of trips in every lane (the plain one leaves inactive lanes through `continue`, and a
 * ballot inside that divergence would see part of the wave); lanes at n >= N vote 0, so the tail
 * word is written whole.  The trips cover every word of the row and the frames every row: a
 * searched utterance's rows need no clearing first (grammar_search_kernel's do: its waves without
 * a node leave before the first frame). */
struct GrammarBigParams {
    GrammarParams g;
    int *ws;                 /* the workspaces of the launch's utterances */
    const long long *ws_off; /* [n_utts] offset (ints) of the utterance's part of ws */
    int u0;                  /* workgroup b searches utterance u0 + b: a call whose history exceeds
                                the budget is searched group by group.  EXPORT with g.only: utterance
                                g.only[u0 + b], the members of one group that a round searches */
};

template <int TPB, bool EXPORT = false> /* threads, the sets of active HMMs written out */
__global__ void __launch_bounds__(TPB)
grammar_search_big_kernel(GrammarBigParams B)
{
    const GrammarParams &P = B.g;
    const int tid = threadIdx.x;
    const int u = (EXPORT && P.only != NULL) ? P.only[B.u0 + (int)blockIdx.x] : B.u0 + (int)blockIdx.x;
    const int gi = P.fsg_of_utt != NULL ? P.fsg_of_utt[u] : 0;
    const int nb = P.node_off[gi], N = P.node_off[gi + 1] - nb;
    const int lb = P.leaf_off[gi];
    const int sb = P.state_off[gi], NS = P.state_off[gi + 1] - sb;
    const int f0 = P.utt_off[u], T = P.utt_off[u + 1] - f0;
    const int W = SSW_WORST_SCORE;
    const int *slot_off = P.slot_off + sb;
    const int j_base = slot_off[0], NE = slot_off[NS] - j_base;
    const int snb = P.sn_off[gi], NSN = P.sn_off[gi + 1] - snb;
    const int ROW = NE > NSN ? (NE > 0 ? NE : 1) : NSN; /* history entries per frame */
    const int start = P.g_start[gi], fin = P.g_final[gi];
    const int NTW = P.tw_off[gi + 1] - P.tw_off[gi], NRK = P.tw_rk[gi];
    const int NTWL = NTW / 4 + 1; /* (a twin record is 4 + L ints, L >= 2) */
    int *ws = B.ws + B.ws_off[u];
    int *S0 = ws, *S1 = S0 + N, *S2 = S1 + N, *H0 = S2 + N, *H1 = H0 + N, *H2 = H1 + N;
    int *OS = H2 + N, *OH = OS + N, *BSC = OH + N, *ACT = BSC + N;
    int *XS = ACT + N, *XH = XS + N, *FLG = XH + N;
    int *IL = FLG + N, *LS = IL + 3 * NE, *TW = LS + 3 * NE, *RK = TW + NTW, *SMAX = RK + NRK;
    int *TWL = SMAX + 2 * NS, *FL = TWL + NTWL;
    __shared__ int s_red[TPB / 64], s_cnt[2], s_ntwl, s_final_id, s_final_score, s_have;
    const uint16_t *senid = P.senid + (size_t)nb * 4;
    const int *pen = P.pen + nb, *parent = P.parent + nb, *leaf_ord = P.leaf_ord + nb;
    const uint32_t *info = P.info + nb;
    const unsigned long long *ctxt = P.ctxt + nb;
    const int *leaf_node = P.leaf_node + lb;
    const int *ls_off = P.ls_off + lb;
    const int *twin_ref = P.twin_ref + nb;
    const int ls_base = ls_off[0];
    int2 *hist = P.hist + P.hist_off[u];

    for (int j = tid; j < NE; j += TPB) {
        const int lo = P.slot_leaf[j_base + j], ln = leaf_node[lo];
        const uint32_t li = info[ln];
        IL[3 * j] = (int)((((li >> 8) & 0xff) << 16) | ((li & FP_ALLRC) ? 1u << 24 : 0u));
        IL[3 * j + 1] = (int)(uint32_t)(ctxt[ln] & 0xffffffffull);
        IL[3 * j + 2] = (int)(uint32_t)(ctxt[ln] >> 32);
        /* (a leaf's slots are ls_slot[ls_off[leaf] ..): NE of them in all */
        const int sj = P.ls_slot[ls_base + j];
        LS[3 * j] = sj;
        LS[3 * j + 1] = P.slot_state[j_base + sj];
        LS[3 * j + 2] = P.slot_pen[j_base + sj];
    }
    for (int i = tid; i < NTW; i += TPB)
        TW[i] = P.tw[P.tw_off[gi] + i];
    for (int i = tid; i < NRK; i += TPB)
        RK[i] = FP_RANK_NONE;
    for (int i = tid; i < 2 * NS; i += TPB)
        SMAX[i] = FP_NO_EXIT;
    if (tid == 0) {
        /* fsg_search_start, as in grammar_search_kernel */
        int be = INT_MIN, bid = -1, have = 0;
        for (int k = 0; k < NSN; ++k) {
            const int sc = P.sn_pen[snb + k];
            hist[k] = make_int2(0, sc);
            if (sc >= P.wbeam) {
                have = 1;
                if (P.sn_to[snb + k] == fin && sc > be) {
                    be = sc;
                    bid = 1 + k;
                }
            }
        }
        s_final_id = bid;
        s_final_score = be;
        s_have = have;
        s_cnt[0] = s_cnt[1] = 0;
        s_ntwl = 0;
    }
    __syncthreads();
    for (int n = tid; n < N; n += TPB) {
        int s0 = W, h0 = -1, a = 0;
        const uint32_t inf = info[n];
        const int pn = pen[n];
        if ((inf & FP_ROOT) && ((ctxt[n] >> P.sil) & 1)) {
            const int d = (int)(inf >> 16);
            if (d == start && pn > P.beam && pn > s0) {
                s0 = pn;
                h0 = 0;
                a = 1;
            }
            for (int q = 0; q < NSN; ++q) {
                const int sc = P.sn_pen[snb + q];
                if (P.sn_to[snb + q] == d && sc >= P.wbeam && sc + pn > P.beam && sc + pn > s0) {
                    s0 = sc + pn;
                    h0 = 1 + q;
                    a = 1;
                }
            }
        }
        S0[n] = s0;
        S1[n] = S2[n] = OS[n] = BSC[n] = W;
        H0[n] = h0;
        H1[n] = H2[n] = OH[n] = -1;
        ACT[n] = a;
        XS[n] = INT_MIN;
        XH[n] = -1;
        FLG[n] = a ? (FP_F_NEXT | FP_F_ENTW) : 0;
        if (leaf_ord[n] >= 0 && twin_ref[n] >= 0) {
            const int i = atomicAdd(&s_ntwl, 1);
            if (i < NTWL)
                TWL[i] = n;
        }
    }
    __syncthreads();
    const int ntwl = s_ntwl < NTWL ? s_ntwl : NTWL;

    for (int f = 0; f < T; ++f) { /* (T is the same in every thread of the group: barriers) */
        /* A: hmm_vit_eval of the active nodes, best score of the frame */
        const uint16_t *urow =
            reinterpret_cast<const uint16_t *>(P.senscr + (size_t)(f0 + f) * P.n_sen);
        int bs = W;
        auto eval = [&](const int n) {
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
        };
        if (EXPORT) {
            /* the HMMs active as the frame starts: what fsg_search_sen_active hands acmod */
            const int MW = (N + 63) >> 6;
            unsigned long long *row = P.act_mask + P.act_off[u] + (long long)f * MW;
            for (int n0 = 0; n0 < N; n0 += TPB) { /* (the same trips in every lane) */
                const int n = n0 + tid;
                const bool on = n < N && (ACT[n] & 1);
                const unsigned long long bm = __ballot(on);
                if ((tid & 63) == 0 && (n >> 6) < MW)
                    row[n >> 6] = bm;
                if (on)
                    eval(n);
            }
        } else {
            for (int n = tid; n < N; n += TPB) {
                if (!(ACT[n] & 1))
                    continue;
                eval(n);
            }
        }
        bs = wave_max_dpp(bs);
        if ((tid & 63) == 0)
            s_red[tid >> 6] = bs;
        __syncthreads();
        int best = s_red[0];
#pragma unroll
        for (int k = 1; k < TPB / 64; ++k)
            best = s_red[k] > best ? s_red[k] : best;
        const int thresh = best + P.beam, pth = best + P.pbeam, wth = best + P.wbeam;

        /* B: the active nodes offer their exits; a word-final HMM that passes the word beam files
         * a word exit and one entry per null transition out of the state it leads to, each into
         * the history table, the state's maximum and the frame's list */
        const int hrow = (f + 1) * ROW;
        for (int i = tid; i < NS; i += TPB) /* next frame's buffer */
            SMAX[((f + 1) & 1) * NS + i] = FP_NO_EXIT;
        for (int n = tid; n < N; n += TPB) {
            const int a = ACT[n];
            if (!(a & 1)) {
                if (a & 4) { /* deactivated last frame: its offer is withdrawn */
                    XS[n] = INT_MIN;
                    ACT[n] = 0;
                }
                continue;
            }
            const int os = OS[n], oh = OH[n];
            const bool keep = BSC[n] >= thresh;
            ACT[n] = 1 | (keep ? 2 : 0);
            XS[n] = (keep && os >= pth) ? os : INT_MIN;
            XH[n] = oh;
            const int lf = leaf_ord[n];
            if (lf < 0)
                continue;
            bool ex = keep && os >= wth;
            const int tw = twin_ref[n];
            if (tw >= 0)
                ex = twin_first_in_list(TW + tw, RK, FLG, f) && ex;
            if (!ex)
                continue;
            const int ls0 = ls_off[lf] - ls_base, ls1 = ls_off[lf + 1] - ls_base;
            int id0 = 0;
            for (int i = ls0; i < ls1; ++i) {
                const int j = LS[3 * i], st = LS[3 * i + 1], sc = os + LS[3 * i + 2];
                /* (the word exit's own slot comes first, with penalty 0) */
                if (sc >= wth) {
                    hist[(size_t)hrow + j] = make_int2(i == ls0 ? oh : id0, sc);
                    atomicMax(&SMAX[(f & 1) * NS + st], sc);
                    const int q = atomicAdd(&s_cnt[f & 1], 1);
                    if (q < NE) { /* (a slot is filed at most once per frame) */
                        FL[3 * q] = j;
                        FL[3 * q + 1] = sc;
                        FL[3 * q + 2] = st;
                    }
                }
                if (i == ls0)
                    id0 = 1 + hrow + j;
            }
        }
        for (int i = tid; i < ntwl; i += TPB) { /* every member keeps its group's order up to date */
            const int n = TWL[i];
            if (!(ACT[n] & 1)) /* (bit 0 does not change in this phase) */
                (void)twin_first_in_list(TW + twin_ref[n], RK, FLG, f);
        }
        __syncthreads();

        /* C: phone transitions, cross-word transitions out of the frame's list, activity */
        const int cnt = s_cnt[f & 1] < NE ? s_cnt[f & 1] : NE;
        for (int n = tid; n < N; n += TPB) {
            const int actf = ACT[n];
            const bool act = actf & 1, keep = (actf & 2) != 0;
            const int par = parent[n];
            const uint32_t inf = info[n];
            int xs = INT_MIN, xh = -1;
            if (par >= 0) {
                xs = XS[par];
                xh = XH[par];
            }
            int mx = FP_NO_EXIT;
            if ((inf & FP_ROOT) && cnt > 0)
                mx = SMAX[(f & 1) * NS + (int)(inf >> 16)];
            if (!act && xs == INT_MIN && mx == FP_NO_EXIT)
                continue; /* (FLG is 0 and XS is INT_MIN already: it was not active) */
            const int pn = pen[n];
            int s0 = S0[n], h0 = H0[n];
            bool entered = false, entered_p = false, entered_w = false;
            if (par >= 0 && xs != INT_MIN) {
                const int ns = xs + pn;
                if (ns > thresh && ns > s0) {
                    s0 = ns; /* hmm_enter */
                    h0 = xh;
                    entered = entered_p = true;
                }
            }
            if ((inf & FP_ROOT) && mx != FP_NO_EXIT && mx + pn > thresh && mx + pn > s0) {
                const int ci = (int)((inf >> 8) & 0xff), d = (int)(inf >> 16);
                const unsigned long long cx = ctxt[n];
                int be = FP_NO_EXIT, bid = -1;
                for (int q = 0; q < cnt; ++q) {
                    if (FL[3 * q + 2] != d)
                        continue;
                    const int j = FL[3 * q], ex = FL[3 * q + 1];
                    if (ex < be || (ex == be && j > bid))
                        continue;
                    const uint32_t w = (uint32_t)IL[3 * j];
                    if (!((cx >> ((w >> 16) & 0xff)) & 1))
                        continue;
                    const unsigned long long rcs = (unsigned long long)(uint32_t)IL[3 * j + 1]
                        | ((unsigned long long)(uint32_t)IL[3 * j + 2] << 32);
                    if (!((w >> 24) & 1) && !((rcs >> ci) & 1))
                        continue;
                    be = ex;
                    bid = j;
                }
                if (bid >= 0) {
                    const int ns = be + pn;
                    if (ns > thresh && ns > s0) {
                        s0 = ns;
                        h0 = 1 + hrow + bid;
                        entered = entered_w = true;
                    }
                }
            }
            const bool stay = keep || entered;
            FLG[n] = (stay ? FP_F_NEXT : 0) | (keep ? FP_F_KEEP : 0) | (entered_p ? FP_F_ENTP : 0)
                | (entered_w ? FP_F_ENTW : 0);
            if (entered) {
                S0[n] = s0;
                H0[n] = h0;
            }
            if (act && !stay) { /* fsg_psubtree_pnode_deactivate -> hmm_clear */
                S0[n] = S1[n] = S2[n] = OS[n] = BSC[n] = W;
                H0[n] = H1[n] = H2[n] = OH[n] = -1;
            }
            ACT[n] = stay ? 1 : (act ? 4 : 0);
        }
        /* fsg_search_find_exit, final: the LAST frame that has any entry, the best entry into the
         * final state, null entries included; of equals the oldest (the lowest slot) */
        if (tid == 0) {
            if (cnt > 0) {
                int be = INT_MIN, bid = -1;
                for (int q = 0; q < cnt; ++q) {
                    if (FL[3 * q + 2] != fin)
                        continue;
                    const int j = FL[3 * q], ex = FL[3 * q + 1];
                    if (ex > be || (ex == be && j < bid)) {
                        be = ex;
                        bid = j;
                    }
                }
                s_final_id = bid >= 0 ? 1 + hrow + bid : -1;
                s_final_score = be;
                s_have = 1;
            }
            s_cnt[(f + 1) & 1] = 0;
        }
        /* no barrier here: the next frame's phase A touches a thread's own nodes only; XS, FL and
         * the counts are written after its barrier, which every reader above has to reach first */
    }
    __syncthreads(); /* the entries written during the loop are read back below */

    /* fsg_search_seg_iter + fsg_seg_bp2itor, as in grammar_search_kernel */
    if (tid == 0) {
        int id = s_final_id, n = 0;
        ssw_fsg_seg_t *seg = P.seg + (size_t)u * P.max_seg;
        if (id < 0)
            n = s_have ? -1 : -2;
        else {
            for (int k = id; k > 0; k = hist[k - 1].x)
                ++n;
            if (n > P.max_seg)
                n = -(3 + n);
            else {
                int j = n - 1;
                for (int k = id; k > 0; k = hist[k - 1].x, --j) {
                    const int row = (k - 1) / ROW, sl = (k - 1) % ROW;
                    const int2 e = hist[k - 1];
                    const int pk = e.x;
                    const int pscore = pk > 0 ? hist[pk - 1].y : 0;
                    const int ef = row - 1;
                    int sf = pk > 0 ? (pk - 1) / ROW : 0; /* predecessor's frame + 1 */
                    sf = sf > ef ? ef : sf;
                    int wid = -1, lscr;
                    if (row == 0)
                        lscr = P.sn_pen[snb + sl];
                    else if (P.slot_null[j_base + sl])
                        lscr = P.slot_pen[j_base + sl];
                    else {
                        const int lo = P.slot_leaf[j_base + sl];
                        wid = P.leaf_wid[lb + lo];
                        lscr = P.leaf_lscr[lb + lo];
                    }
                    seg[j].wid = wid;
                    seg[j].sf = sf;
                    seg[j].ef = ef;
                    seg[j].lscr = lscr;
                    seg[j].ascr = e.y - pscore - lscr;
                }
            }
            P.score[u] = s_final_score;
        }
        P.n_seg[u] = n;
    }
}
