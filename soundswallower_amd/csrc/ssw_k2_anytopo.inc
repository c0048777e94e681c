/* ssw_k2_anytopo.inc -- K2 for the topologies no shipped model has: state alignment over HMMs of
 * 1, 2, 4 or 5 emitting states (hmm_vit_eval's other two branches, src/hmm.c:741-759:
 * hmm_vit_eval_5st_lr :166-304 and hmm_vit_eval_anytopo :671-739; HMM_MAX_NSTATE = 5,
 * include/soundswallower/hmm.h).  Part of the single translation unit ssw_kernels.hip.
 *
 * One plain kernel, built to be read against the reference rather than for speed: one wave per
 * utterance, lane = phone (64-phone words in turn), the HMMs' state in a per-utterance HBM
 * workspace, the reference's full tokens.  The search around the evaluator is the 3-state
 * kernels' (state_align_search.c:57-213, viterbi_align_kernel above) with the state count a
 * run-time value. */

/* hmm_vit_eval_5st_lr, src/hmm.c:166-304 (non-mpx).  n[] are the NEGATED senone scores, tp the
 * matrix's 5 x 6 bytes (negated on use).  Blocks that the reference skips leave the stored
 * score of their state as it was, while the LOCAL value (score + senone score) goes on into the
 * blocks below, exactly as there. */
__device__ int
vit_eval_5st(int (&s)[5], int (&h)[5], int &os, int &oh, const int (&n)[5], const uint8_t *tp)
{
#define TP5(i, j) (-(int)tp[(i) * 6 + (j)])
    const int W = SSW_WORST_SCORE;
    int best = W, t0, t1, t2;
    int s4 = s[4] + n[4], s3 = s[3] + n[3];
    if (s3 > W) { /* into the exit state */
        t1 = s4 + TP5(4, 5);
        t2 = s3 + TP5(3, 5);
        int s5;
        if (t1 > t2) {
            s5 = t1;
            oh = h[4];
        } else {
            s5 = t2;
            oh = h[3];
        }
        s5 = s5 < W ? W : s5;
        os = s5;
        best = s5;
    }
    int s2 = s[2] + n[2];
    if (s2 > W) { /* into state 4 */
        t0 = s4 + TP5(4, 4);
        t1 = s3 + TP5(3, 4);
        t2 = s2 + TP5(2, 4);
        if (t0 > t1) {
            if (t2 > t0) {
                s4 = t2;
                h[4] = h[2];
            } else
                s4 = t0;
        } else if (t2 > t1) {
            s4 = t2;
            h[4] = h[2];
        } else {
            s4 = t1;
            h[4] = h[3];
        }
        s4 = s4 < W ? W : s4;
        best = s4 > best ? s4 : best;
        s[4] = s4;
    }
    int s1 = s[1] + n[1];
    if (s1 > W) { /* into state 3 */
        t0 = s3 + TP5(3, 3);
        t1 = s2 + TP5(2, 3);
        t2 = s1 + TP5(1, 3);
        if (t0 > t1) {
            if (t2 > t0) {
                s3 = t2;
                h[3] = h[1];
            } else
                s3 = t0;
        } else if (t2 > t1) {
            s3 = t2;
            h[3] = h[1];
        } else {
            s3 = t1;
            h[3] = h[2];
        }
        s3 = s3 < W ? W : s3;
        best = s3 > best ? s3 : best;
        s[3] = s3;
    }
    int s0 = s[0] + n[0];
    /* into state 2 (state 0 is always live) */
    t0 = s2 + TP5(2, 2);
    t1 = s1 + TP5(1, 2);
    t2 = s0 + TP5(0, 2);
    if (t0 > t1) {
        if (t2 > t0) {
            s2 = t2;
            h[2] = h[0];
        } else
            s2 = t0;
    } else if (t2 > t1) {
        s2 = t2;
        h[2] = h[0];
    } else {
        s2 = t1;
        h[2] = h[1];
    }
    s2 = s2 < W ? W : s2;
    best = s2 > best ? s2 : best;
    s[2] = s2;
    /* into state 1 */
    t0 = s1 + TP5(1, 1);
    t1 = s0 + TP5(0, 1);
    if (t0 > t1)
        s1 = t0;
    else {
        s1 = t1;
        h[1] = h[0];
    }
    s1 = s1 < W ? W : s1;
    best = s1 > best ? s1 : best;
    s[1] = s1;
    /* state 0 */
    s0 += TP5(0, 0);
    s0 = s0 < W ? W : s0;
    best = s0 > best ? s0 : best;
    s[0] = s0;
#undef TP5
    return best;
}

/* hmm_vit_eval_anytopo, src/hmm.c:671-739 (non-mpx): every arc that exists (tp > -255), targets
 * from the exit state down, sources from the nearest state down; the first source reaching a
 * score stays (strict >).  st[0] is NOT clamped and no new score is (as there).  Loops fully
 * unrolled with `< ne` guards: the arrays stay in registers. */
__device__ int
vit_eval_anytopo(int ne, int (&s)[5], int (&h)[5], int &os, int &oh, const int (&n)[5],
                 const uint8_t *tp)
{
    const int W = SSW_WORST_SCORE;
    const int nc = ne + 1;
    int st[5], hold[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        st[i] = i < ne ? s[i] + n[i] : W;
        if (i >= 1 && st[i] < W)
            st[i] = W;
        hold[i] = h[i];
    }
    /* (the reference overwrites history[to] while sources below `to` are still to be read for
     * lower targets; a source is always BELOW its target, so those reads see values this call
     * has not touched: reading from a copy is the same thing) */
    int scr = W, bestfrom = -1;
#pragma unroll
    for (int from = 4; from >= 0; --from)
        if (from < ne) {
            const int a = -(int)tp[from * nc + ne];
            if (a > -255 && st[from] + a > scr) {
                scr = st[from] + a;
                bestfrom = from;
            }
        }
    os = scr;
#pragma unroll
    for (int from = 0; from < 5; ++from)
        if (from == bestfrom)
            oh = hold[from];
    int best = scr;
#pragma unroll
    for (int to = 4; to >= 0; --to)
        if (to < ne) {
            const int self = -(int)tp[to * nc + to];
            scr = self > -255 ? st[to] + self : W;
            bestfrom = -1;
#pragma unroll
            for (int from = 3; from >= 0; --from)
                if (from < to) {
                    const int a = -(int)tp[from * nc + to];
                    if (a > -255 && st[from] + a > scr) {
                        scr = st[from] + a;
                        bestfrom = from;
                    }
                }
            s[to] = scr;
#pragma unroll
            for (int from = 0; from < 4; ++from)
                if (from == bestfrom)
                    h[to] = hold[from];
            best = best < scr ? scr : best;
        }
    return best;
}

/* per-phone arrays of the workspace: [G_COUNT][max_phones + 1] ints per utterance */
enum { G_OS, G_OH, G_FR, G_SF, G_EF, G_S, G_H = G_S + 5, G_COUNT = G_H + 5 };

__global__ void __launch_bounds__(64)
viterbi_align_any_kernel(AlignParams P, int ne)
{
    const int u = blockIdx.x;
    const int lane = threadIdx.x;
    const AlignUtt U = P.utts[u];
    const int NP = U.n_phones;
    const int PP = P.max_phones + 1; /* slot NP: a never-active sentinel neighbour */
    const int W = (NP + 63) >> 6;
    const int n_states = NP * ne;
    int *ws = P.big_ws + U.ws_off;
    auto sync_lanes = [] {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
    };
#define G(arr, p) ws[(arr)*PP + (p)]
    for (int p = lane; p <= NP; p += 64) {
        for (int j = 0; j < 5; ++j) { /* hmm_clear, src/hmm.c:124-140 */
            G(G_S + j, p) = SSW_WORST_SCORE;
            G(G_H + j, p) = -1;
        }
        G(G_OS, p) = SSW_WORST_SCORE;
        G(G_OH, p) = -1;
        G(G_FR, p) = -1;
        G(G_SF, p) = p < NP ? P.sf[U.phone_off + p] : INT_MAX;
        G(G_EF, p) = p < NP ? P.ef[U.phone_off + p] : INT_MAX;
    }
    sync_lanes();
    if (lane == 0) { /* state_align_search_start: hmm_enter(hmms, 0, 0, 0) */
        G(G_S, 0) = 0;
        G(G_H, 0) = 0;
        G(G_FR, 0) = 0;
    }
    sync_lanes();

    int2 *tok = P.tokens + U.tok_off;
    int best_score = 0;
    for (int t = 0; t < U.n_frames; ++t) {
        const int16_t *row = P.senscr + U.scr_off + (long long)t * U.scr_stride;
        const int nf = t + 1;
        const bool renorm = align_renorm_due(best_score);
        int bs = SSW_WORST_SCORE;
        /* renormalize_hmms + evaluate_hmms + prune_hmms (state_align_search.c:57-106) */
        for (int w = 0; w < W; ++w) {
            const int p = w * 64 + lane;
            if (p < NP) {
                const int gp = U.phone_off + p;
                int s[5], os = G(G_OS, p);
#pragma unroll
                for (int j = 0; j < 5; ++j)
                    s[j] = G(G_S + j, p);
                if (renorm) { /* hmm_normalize, src/hmm.c:150-161 */
#pragma unroll
                    for (int j = 0; j < 5; ++j)
                        if (j < ne && s[j] > SSW_WORST_SCORE)
                            s[j] -= best_score;
                    if (os > SSW_WORST_SCORE)
                        os -= best_score;
                }
                if (G(G_FR, p) >= t) {
                    int h[5], n[5], oh = G(G_OH, p);
#pragma unroll
                    for (int j = 0; j < 5; ++j) {
                        h[j] = G(G_H + j, p);
                        n[j] = j < ne ? -(int)row[P.senid[(size_t)gp * ne + j]] : 0;
                    }
                    const uint8_t *tp = P.tp + (size_t)P.tmatid[gp] * ne * (ne + 1);
                    const int b = ne == 5 ? vit_eval_5st(s, h, os, oh, n, tp)
                                          : vit_eval_anytopo(ne, s, h, os, oh, n, tp);
                    bs = b > bs ? b : bs;
#pragma unroll
                    for (int j = 0; j < 5; ++j)
                        G(G_H + j, p) = h[j];
                    G(G_OH, p) = oh;
                    if (nf <= G(G_EF, p))
                        G(G_FR, p) = nf;
                }
#pragma unroll
                for (int j = 0; j < 5; ++j)
                    G(G_S + j, p) = s[j];
                G(G_OS, p) = os;
            }
        }
        best_score = wave_max_i32(bs);
        sync_lanes();

        /* phone_transition (state_align_search.c:108-133) as a carry chain over the 64-phone
         * words, then record_transitions (:149-175): as viterbi_align_kernel */
        unsigned long long cin = 0;
        int2 *tkrow = tok + (size_t)t * n_states;
        for (int w = 0; w < W; ++w) {
            const int p = w * 64 + lane;
            const bool valid = p < NP;
            int fr = valid ? G(G_FR, p) : -1;
            const bool a_bit = valid && fr == nf;
            bool c_bit = false;
            if (valid && p + 1 < NP) {
                const int nfr = G(G_FR, p + 1);
                c_bit = (nf >= G(G_SF, p + 1)) && (nfr < t || G(G_OS, p) > G(G_S, p + 1));
            }
            const unsigned long long A = __ballot(a_bit), Cm = __ballot(c_bit);
            const unsigned long long X = Cm, Y = A & Cm;
            const unsigned long long S = X + Y + cin;
            const unsigned long long E = S ^ X ^ Y; /* bit i: phone w * 64 + i is entered */
            const unsigned long long cout = ((X & Y) | ((X | Y) & ~S)) >> 63;
            const bool entered = (E >> lane) & 1ull;
            int src_os = 0, src_oh = 0;
            if (valid && entered) { /* p >= 1 whenever entered */
                src_os = G(G_OS, p - 1);
                src_oh = G(G_OH, p - 1);
            }
            sync_lanes(); /* all reads of neighbours done before this word's writes */
            if (valid) {
                if (entered) { /* hmm_enter, src/hmm.c:142-148 */
                    G(G_S, p) = src_os;
                    G(G_H, p) = src_oh;
                    G(G_FR, p) = nf;
                    fr = nf;
                }
                for (int j = 0; j < ne; ++j) {
                    int2 k = make_int2(-1, -1);
                    if (fr >= t) {
                        k = make_int2(G(G_H + j, p), G(G_S + j, p));
                        G(G_H + j, p) = p * ne + j;
                    }
                    tkrow[p * ne + j] = k;
                }
            }
            cin = cout;
            sync_lanes();
        }
    }
    /* state_align_search_finish (state_align_search.c:215-268) */
    __syncthreads();
    if (lane == 0)
        align_backtrace(P, U, u, tok, n_states, G(G_OH, NP - 1), G(G_OS, NP - 1), nullptr, nullptr, ne);
#undef G
}
