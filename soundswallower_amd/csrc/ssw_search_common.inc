/* ssw_search_common.inc -- device: what the grammar search kernels share.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */
/* ---------------------------------------------------------------------------------- */
/* first_pass_kernel, first_pass_big_kernel and first_pass_win_kernel (ssw_k5_firstpass.inc)   */
/* differ in where the state of the search lives; every decision they take of the reference's  */
/* fsg_search is here, once, and a K5 kernel holds its storage, its walk over the nodes, its   */
/* barriers and calls into this file.  grammar_search_kernel (ssw_k9_grammar.inc) uses the     */
/* flags, twin_first_in_list, il_pack and best_entry; grammar_search_big_kernel the flags and  */
/* twin_first_in_list; K9's other blocks are their own text (profiles/README.md, search_common).*/
/* A kernel that indexes an LDS ring passes the ring's mask (-1: none), as twin_first_in_list  */
/* takes flg_mask.                                                                            */
/* ---------------------------------------------------------------------------------- */
#define FP_ROOT 1u
#define FP_LEAF 2u
#define FP_ALLRC 4u
#define FP_TWIN 8u
#define FP_TWIN_FIRST 16u
#define FP_TWIN_LAST 32u
#define FP_NO_EXIT INT_MIN
#define FP_RANK_NONE (1 << 20)
enum { FP_F_NEXT = 1, FP_F_KEEP = 2, FP_F_ENTP = 4, FP_F_ENTW = 8 };

/* Alternates pronounced alike ("twins") exit together with equal scores, and the reference's
 * history table keeps the exit that is entered first (src/fsg_history.c:164-170): the twin that
 * stands first in the active list.  That list is rebuilt every frame by prepending
 * (src/fsg_search.c:498-541): a surviving node at its own turn, a node its predecessor
 * transitions into at the predecessor's turn (children in chain order), word-initial nodes
 * entered by cross-word transitions after all of those.  The relative order of a twin group and
 * its ancestors depends on nothing but their own turns and flags, so every member follows it:
 * rec = [L, n_anc, own index, rank-buffer offset, L nodes (root .. predecessor, members in chain
 * order)], two rank buffers of L (list positions among these L nodes in this frame's list /
 * the previous one's).  Called once per frame by every member; returns whether the member is
 * the first of its group in this frame's list. */
__device__ __forceinline__ bool
twin_first_in_list(const int *rec, int *RK, const int *FLG, int f, int flg_mask = -1)
{
    const int L = rec[0], n_anc = rec[1], me = rec[2];
    const int *prev = RK + rec[3] + ((f + 1) & 1) * L;
    int *cur = RK + rec[3] + (f & 1) * L, *key = RK + rec[3] + 2 * L;
    /* when was element i put on this frame's list, in the previous frame's processing order?
     * own turn: 128 * its position; by its predecessor: 128 * the predecessor's position + 1 +
     * chain index; by a cross-word transition: after everything */
    for (int i = 0; i < L; ++i) {
        const int flg = FLG[rec[4 + i] & flg_mask];
        const int par = i < n_anc ? i - 1 : n_anc - 1;
        const int cidx = i < n_anc ? 0 : i - n_anc;
        int k = INT_MAX;
        if (flg & FP_F_NEXT) {
            if (flg & FP_F_KEEP)
                k = prev[i] * 128;
            if ((flg & FP_F_ENTP) && par >= 0) {
                const int k2 = prev[par] * 128 + 1 + cidx;
                k = k2 < k ? k2 : k;
            }
            if (flg & FP_F_ENTW) {
                const int k3 = (1 << 28) + cidx;
                k = k3 < k ? k3 : k;
            }
        }
        key[i] = k;
    }
    /* the list is the reverse of that order: position = number of elements put on it later */
    int best = FP_RANK_NONE;
    for (int i = 0; i < L; ++i) {
        const int ki = key[i];
        int r = FP_RANK_NONE;
        if (ki != INT_MAX) {
            r = 0;
            for (int j = 0; j < L; ++j) {
                const int kj = key[j];
                r += (kj != INT_MAX && kj > ki) ? 1 : 0;
            }
        }
        cur[i] = r;
        if (i >= n_anc)
            best = r < best ? r : best;
    }
    return cur[me] != FP_RANK_NONE && cur[me] == best;
}

/* IL: three ints per entry of a state's entering list, made of the word-final HMM behind it:
 * id (K5: its leaf ordinal; K9 names an entry by its slot: 0) | the phone it shows to the left
 * context test << 16 | "any right context" << 24, then its right-context set. */
__device__ __forceinline__ void
il_pack(int *IL, int j, uint32_t id, uint32_t leaf_info, unsigned long long leaf_ctxt)
{
    IL[3 * j] = (int)(id | (((leaf_info >> 8) & 0xff) << 16) | ((leaf_info & FP_ALLRC) ? 1u << 24 : 0u));
    IL[3 * j + 1] = (int)(uint32_t)(leaf_ctxt & 0xffffffffull);
    IL[3 * j + 2] = (int)(uint32_t)(leaf_ctxt >> 32);
}
/* may entry j enter a word-initial HMM with left-context set lctxt and phone ci?
 * (fsg_search_word_trans, src/fsg_search.c:630-650); w: the entry's first word */
__device__ __forceinline__ bool
il_compatible(const int *IL, int j, unsigned long long lctxt, int ci, uint32_t &w)
{
    w = (uint32_t)IL[3 * j];
    if (!((lctxt >> ((w >> 16) & 0xff)) & 1))
        return false;
    const unsigned long long rcs =
        (unsigned long long)(uint32_t)IL[3 * j + 1] | ((unsigned long long)(uint32_t)IL[3 * j + 2] << 32);
    return ((w >> 24) & 1) || ((rcs >> ci) & 1);
}

/* TW the twin records, RK their rank buffers, SMAX the best entry into each state (n_smax ints) */
template <int TPB>
__device__ __forceinline__ void
search_tables_init(int *TW, const int *tw, int n_tw, int *RK, int n_rk, int *SMAX, int n_smax, int tid)
{
    for (int i = tid; i < n_tw; i += TPB)
        TW[i] = tw[i];
    for (int i = tid; i < n_rk; i += TPB)
        RK[i] = FP_RANK_NONE;
    for (int i = tid; i < n_smax; i += TPB)
        SMAX[i] = FP_NO_EXIT;
}

/* fsg_search_start (src/fsg_search.c:747-802) of a linear text: the dummy entry 0 (score 0, left
 * context SIL, every right context) enters the word-initial HMMs of state 0 under beam alone.
 * (K9's rule, with the start state's null transitions, stays in its kernels: see the head of
 * this file.) */
__device__ __forceinline__ bool
search_start_text(uint32_t info, unsigned long long ctxt, int pen, int sil, int beam, int &s0, int &h0)
{
    if ((info & FP_ROOT) && (info >> 16) == 0 && ((ctxt >> sil) & 1) && pen > beam
        && pen > SSW_WORST_SCORE) {
        s0 = pen;
        h0 = 0;
        return true;
    }
    return false;
}

/* The frame's best score and the three beams off it (fsg_search_hmm_eval, :331-402).  A wave
 * publishes its maximum, the kernel's barrier follows, then every thread reads the beams. */
struct FrameBeams {
    int thresh, pth, wth;
};
__device__ __forceinline__ void
beams_publish(int *s_red, int bs, int tid)
{
    bs = wave_max_dpp(bs); /* (DPP: six dependent LDS-crossbar shuffles were ~400 clocks of a frame) */
    if ((tid & 63) == 0)
        s_red[tid >> 6] = bs;
}
template <int TPB>
__device__ __forceinline__ FrameBeams
beams_read(const int *s_red, int beam, int pbeam, int wbeam)
{
    int best = s_red[0];
#pragma unroll
    for (int k = 1; k < TPB / 64; ++k)
        best = s_red[k] > best ? s_red[k] : best;
    return FrameBeams{ best + beam, best + pbeam, best + wbeam };
}

/* The best compatible entry of the list slots [j0, j1) of a state (fsg_search_word_trans,
 * :598-662): first of equals.  The winner is named by its slot (K9) or by the leaf ordinal IL
 * holds (K5). */
template <bool SLOT_ID>
__device__ __forceinline__ void
best_entry(const int *EXJ, const int *IL, int j0, int j1, unsigned long long lctxt, int ci, int &be,
           int &bid, int exj_mask = -1)
{
    be = FP_NO_EXIT;
    bid = -1;
    for (int j = j0; j < j1; ++j) {
        const int ex = EXJ[j & exj_mask];
        if (ex == FP_NO_EXIT || ex <= be)
            continue;
        uint32_t w;
        if (!il_compatible(IL, j, lctxt, ci, w))
            continue;
        be = ex;
        bid = SLOT_ID ? j : (int)(w & 0xffff);
    }
}

/* hmm_enter under the beam, if strictly better than what state 0 holds */
__device__ __forceinline__ bool
hmm_enter_better(int score, int history, int pen, int thresh, int &s0, int &h0)
{
    const int ns = score + pen;
    if (ns > thresh && ns > s0) {
        s0 = ns;
        h0 = history;
        return true;
    }
    return false;
}
/* Phase C of a node: the phone transition from its one predecessor (exit xs / xh, INT_MIN: none;
 * fsg_search_pnode_trans, :404-435), then, for a word-initial node whose state's best entry mx
 * (FP_NO_EXIT: none, or not word-initial) could still enter, the cross-word transition from the
 * best compatible entry scan(be, bid) finds; its history id is id_base + bid.  Returns the
 * FP_F_ENTP / FP_F_ENTW bits. */
template <class Scan>
__device__ __forceinline__ int
node_enter(bool has_pred, int xs, int xh, int mx, int pen, int thresh, int id_base, int &s0, int &h0,
           Scan scan)
{
    bool entered_p = false, entered_w = false;
    if (has_pred && xs != INT_MIN)
        entered_p = hmm_enter_better(xs, xh, pen, thresh, s0, h0);
    if (mx != FP_NO_EXIT && mx + pen > thresh && mx + pen > s0) {
        int be, bid;
        scan(be, bid);
        if (bid >= 0)
            entered_w = hmm_enter_better(be, id_base + bid, pen, thresh, s0, h0);
    }
    return (entered_p ? FP_F_ENTP : 0) | (entered_w ? FP_F_ENTW : 0);
}

/* Does the node stay on the active list (fsg_search_hmm_prune_prop, :498-541), and how it came
 * through the frame: the word FLG holds for the twins' order. */
__device__ __forceinline__ bool
settle(bool keep, int entered, int &flg)
{
    const bool stay = keep || entered != 0;
    flg = (stay ? FP_F_NEXT : 0) | (keep ? FP_F_KEEP : 0) | entered;
    return stay;
}
/* ... with the HMM in registers: fsg_psubtree_pnode_deactivate -> hmm_clear */
__device__ __forceinline__ void
settle_regs(bool &act, bool keep, int entered, int &flg, int &s0, int &s1, int &s2, int &h0, int &h1,
            int &h2, int &os, int &oh, int &bsc)
{
    const bool stay = settle(keep, entered, flg);
    if (act && !stay) {
        s0 = s1 = s2 = os = bsc = SSW_WORST_SCORE;
        h0 = h1 = h2 = oh = -1;
    }
    act = stay;
}

/* fsg_search_find_exit (:854-925) over the final state's list slots [j0, j1): the best entry,
 * first of equals; -1 when there is none.  Named as in best_entry. */
template <bool SLOT_ID>
__device__ __forceinline__ int
final_exit(const int *EXJ, const int *IL, int j0, int j1, int &be, int exj_mask = -1)
{
    int bid = -1;
    be = INT_MIN;
    for (int j = j0; j < j1; ++j) {
        const int ex = EXJ[j & exj_mask];
        if (ex != FP_NO_EXIT && ex > be) {
            be = ex;
            bid = SLOT_ID ? j : IL[3 * j] & 0xffff;
        }
    }
    return bid;
}

/* fsg_search_seg_iter (:1085-1143) for K5: walk the predecessors back from entry id (< 0: no
 * match), then write the words in order.  Entry id = 1 + frame * NL + leaf; at(id) is its slot
 * in hist.  Returns the number of segments, -1, or -(2 + n) when the n segments do not fit (room
 * is needed: not a search failure). */
template <class At>
__device__ __forceinline__ int
fp_write_segments(const int2 *hist, At at, int id, int NL, const int *leaf_wid, ssw_word_seg_t *seg,
                  int max_seg)
{
    if (id < 0)
        return -1;
    int n = 0;
    for (int k = id; k > 0; k = hist[at(k)].x)
        ++n;
    if (n > max_seg)
        return -(2 + n);
    int j = n - 1;
    for (int k = id; k > 0; k = hist[at(k)].x, --j) {
        const int fr = (k - 1) / NL, lo = (k - 1) % NL;
        const int pk = hist[at(k)].x;
        int sf = pk > 0 ? (pk - 1) / NL + 1 : 0;
        sf = sf > fr ? fr : sf;
        seg[j].wid = leaf_wid[lo];
        seg[j].start = sf;
        seg[j].duration = fr - sf + 1;
        seg[j].score = hist[at(k)].y;
    }
    return n;
}

/* The senone scores of one HMM per thread, two frames ahead: two rotating sets of the three
 * dwords that hold the 16-bit scores (score_dword, ssw_dev_common.inc), extracted at use; frame
 * f's are requested at the top of frame f - 2 (one frame ahead, a frame of ~1.3 us was shorter
 * than a loaded DRAM round trip).  Beyond the end the last row again. */
__device__ __forceinline__ void
scores_request(const int16_t *senscr, int f0, int f, int T, int n_sen, uint32_t sen01, uint32_t sen2t,
               uint32_t &q0, uint32_t &q1, uint32_t &q2)
{
    const ScoreRow r = score_row(senscr, (size_t)(f0 + (f < T ? f : T - 1)) * n_sen);
    q0 = score_dword(r, sen01 & 0xffff);
    q1 = score_dword(r, sen01 >> 16);
    q2 = score_dword(r, sen2t & 0xffff);
}
/* frame f's scores out of the set, which is free again: frame f + 2's into it (unconditional, so
 * that the number of loads in flight is the same on every path) */
__device__ __forceinline__ void
scores_take(const int16_t *senscr, int f0, int f, int T, int n_sen, uint32_t sen01, uint32_t sen2t,
            uint32_t &q0, uint32_t &q1, uint32_t &q2, int &c0, int &c1, int &c2)
{
    /* the empty asm pins the wait for this frame's loads HERE and keeps the compiler from
     * pulling the sign extension (and with it the wait) up to the load */
    uint32_t a = q0, b = q1, c = q2;
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c));
    const uint32_t lo = score_row(senscr, (size_t)(f0 + f) * n_sen).lo;
    c0 = score_of(a, lo, sen01 & 0xffff);
    c1 = score_of(b, lo, sen01 >> 16);
    c2 = score_of(c, lo, sen2t & 0xffff);
    scores_request(senscr, f0, f + 2, T, n_sen, sen01, sen2t, q0, q1, q2);
}
