/* ssw_k2_align.inc -- K2: forced-alignment Viterbi kernels.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */
/* ---------------------------------------------------------------------------------- */
/* K2: forced-alignment Viterbi, one wave per utterance                                 */
/* ---------------------------------------------------------------------------------- */

struct AlignUtt {
    int frame_off, n_frames, phone_off, n_phones;
    long long tok_off; /* offset (in tokens) of this utterance's token stack */
    long long ws_off;  /* HBM-resident kernel: offset (ints) of its 16 x (max_phones + 1) state arrays */
    /* the utterance's score rows: frame t's row starts scr_off + t * scr_stride int16 elements
     * into AlignParams::senscr, and AlignParams::senid holds the index of each state's score IN
     * that row.  Full rows (acmod's [n_sen] layout): scr_off = frame_off * n_sen, scr_stride =
     * n_sen, index = the senone id.  Compact rows (round 5, ssw_score_batch_compact): only the
     * utterance's own states, scr_stride = 3 * n_phones rounded up to even, index = the first
     * state of the utterance with that senone */
    long long scr_off;
    int scr_stride, pad_;
};

struct AlignParams {
    const int16_t *senscr; /* [total_frames][n_sen] */
    const AlignUtt *utts;
    const uint16_t *senid; /* [total_phones][3]: index of the state's score in its row (AlignUtt) */
    const int16_t *tmatid; /* [total_phones] */
    const int32_t *sf, *ef;
    const uint8_t *tp; /* [n_tmat][12] */
    int2 *tokens;
    /* viterbi_align_mwb_kernel (round 5): byte tokens -- per utterance, at AlignUtt::tok_off BYTES:
     * [n_frames][64 n_words] one byte per phone and frame (three 2-bit back-pointers), then
     * [n_frames] int32 renormalisation amounts, then [n_frames + 1] uint16 states of the path */
    uint8_t *btok;
    ssw_align_entry_t *state_io; /* [total_phones*3] */
    int32_t *status;
    int n_sen, n_utts, max_phones;
    int *big_ws; /* viterbi_align_kernel<0, true>: per-utterance state arrays in HBM */
    /* the same kernel, round 3: a BANDED token table.  band_tokens > 0: frame t keeps tokens only
     * for the 64-phone words it walks (first active .. last active + 1), at TB[t] + id - TL[t];
     * the utterance's table holds n_frames * min(n_states, band_tokens) tokens and an utterance
     * whose bands outgrow that reports status -(1 << 30) (the host then takes the full table).
     * band_ws: per utterance TB[n_frames + 1] and TL[n_frames], at 2 * frame_off + 2 * u. */
    int band_tokens;
    int *band_ws;
};

/* state_align_search_finish (state_align_search.c:215-268): one lane walks the token stack
 * back from frame n_frames - 2. */
__device__ __forceinline__ void
align_backtrace(const AlignParams &P, const AlignUtt &U, int u, const int2 *tok, int n_states,
                int final_id, int final_score, const int *TB = nullptr, const int *TL = nullptr,
                int n_emit = 3)
{
    ssw_align_entry_t *st = P.state_io + (size_t)U.phone_off * n_emit;
    int last_id = final_id, cur_id = last_id;
    int last_score = final_score;
    int status = 0;
    if (last_id == -1) {
        status = -1;
    } else {
        int last_frame = U.n_frames;
        for (int cf = U.n_frames - 2; cf >= 0; --cf) {
            int2 cur;
            if (TB != nullptr) { /* banded table: outside the frame's band nothing was active */
                const int base = TB[cf], idx = cur_id - TL[cf];
                cur = (idx >= 0 && idx < TB[cf + 1] - base) ? tok[(size_t)base + idx]
                                                            : make_int2(-1, -1);
            } else
                cur = tok[(size_t)cf * n_states + cur_id];
            cur_id = cur.x;
            if (cur_id == -1) {
                status = -(2 + cf);
                break;
            }
            if (cur_id != last_id) {
                st[last_id].start = cf + 1;
                st[last_id].duration = last_frame - (cf + 1);
                st[last_id].score = last_score - cur.y;
                last_id = cur_id;
                last_score = cur.y;
                last_frame = cf + 1;
            }
        }
        if (status == 0) {
            st[0].start = 0;
            st[0].duration = last_frame;
        }
    }
    P.status[u] = status;
}

/* LDS layout: 16 int arrays of `P` (padded phone count) entries each. */
enum { A_S0, A_S1, A_S2, A_H0, A_H1, A_H2, A_OS, A_OH, A_FR, A_TPA, A_TPB, A_TPC, A_SEN01,
       A_SEN2, A_SF, A_EF, A_COUNT };

/* WMAX > 0: utterances of up to 64 * WMAX phones; every lane keeps the senone scores of its
 * phones for the current frame in registers and requests the next frame's at the top of each
 * frame, so the scattered 2-byte gathers from the score rows (DRAM latency: the rows were
 * written by another kernel long ago) are a whole frame step ahead of their use.  WMAX == 0:
 * any phone count, scores fetched where they are used. */
/* HBM = true (WMAX == 0 only): utterances beyond what LDS holds (2,560 phones, about 550 words
 * -- a 2,000-word page has ~9,000).  The 16 state arrays live in a per-utterance HBM workspace
 * (L2-resident), the lane-to-lane ordering points become workgroup-scope fences (global stores
 * complete before the neighbours' loads), and a frame only walks the 64-phone words between the
 * first and the last active phone (+ 1: the word a carry can enter) -- the search is left to
 * right, phones outside that range are inert until the range reaches them; when scores are
 * renormalised every phone is visited, as in the reference.  The token table is pre-set to -1
 * by the host and written for the walked words only. */
template <int WMAX, bool HBM = false>
__global__ void __launch_bounds__(64)
viterbi_align_kernel(AlignParams P)
{
    static_assert(!HBM || WMAX == 0, "the HBM-resident variant fetches scores where it uses them");
    extern __shared__ int lds_dyn[];
    const int u = blockIdx.x;
    const int lane = threadIdx.x;
    const AlignUtt U = P.utts[u];
    const int NP = U.n_phones;
    const int PP = P.max_phones + 1; /* +1: slot NP is a never-active sentinel neighbour */
    const int W = (NP + 63) >> 6;
    const int n_states = NP * 3;
    int *lds = HBM ? P.big_ws + U.ws_off : lds_dyn;
    auto sync_lanes = [] {
        if (HBM) {
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            __builtin_amdgcn_wave_barrier();
        } else
            wave_sync();
    };
    int wlo = 0, whi = 0; /* HBM: words holding an active phone (phone 0 at the start) */
    const bool BANDT = HBM && P.band_tokens > 0;
    int *TB = BANDT ? P.band_ws + 2 * (size_t)U.frame_off + 2 * (size_t)u : nullptr;
    int *TL = BANDT ? TB + U.n_frames + 1 : nullptr;
    long long tbase = 0;
    const long long tcap = BANDT
        ? (long long)U.n_frames * (n_states < P.band_tokens ? n_states : P.band_tokens) : 0;
    bool ovf = false;
#define L(arr, p) lds[(arr)*PP + (p)]

    for (int p = lane; p <= NP; p += 64) {
        bool real = p < NP;
        int gp = U.phone_off + p;
        L(A_S0, p) = SSW_WORST_SCORE; /* hmm_clear, src/hmm.c:124-140 */
        L(A_S1, p) = SSW_WORST_SCORE;
        L(A_S2, p) = SSW_WORST_SCORE;
        L(A_H0, p) = -1;
        L(A_H1, p) = -1;
        L(A_H2, p) = -1;
        L(A_OS, p) = SSW_WORST_SCORE;
        L(A_OH, p) = -1;
        L(A_FR, p) = -1;
        if (real) {
            const uint32_t *tp = reinterpret_cast<const uint32_t *>(P.tp)
                + (size_t)P.tmatid[gp] * 3;
            L(A_TPA, p) = (int)tp[0];
            L(A_TPB, p) = (int)tp[1];
            L(A_TPC, p) = (int)tp[2];
            L(A_SEN01, p) = (int)P.senid[gp * 3] | ((int)P.senid[gp * 3 + 1] << 16);
            L(A_SEN2, p) = (int)P.senid[gp * 3 + 2];
            L(A_SF, p) = P.sf[gp];
            L(A_EF, p) = P.ef[gp];
        } else {
            L(A_SF, p) = INT_MAX; /* nothing ever transitions into the sentinel */
            L(A_EF, p) = INT_MAX;
        }
    }
    sync_lanes();
    if (lane == 0) { /* state_align_search_start: hmm_enter(hmms, 0, 0, 0) */
        L(A_S0, 0) = 0;
        L(A_H0, 0) = 0;
        L(A_FR, 0) = 0;
    }
    sync_lanes();

    int2 *tok = P.tokens + U.tok_off;
    int best_score = 0;
    constexpr int WR = WMAX ? WMAX : 1;
    int sid01[WR], sid2[WR], cur01[WR], cur2[WR];
    if (WMAX) {
        const int16_t *row0 = P.senscr + U.scr_off;
#pragma unroll
        for (int w = 0; w < WR; ++w) {
            int p = w * 64 + lane;
            bool real = p < NP && U.n_frames > 0;
            sid01[w] = real ? L(A_SEN01, p) : 0;
            sid2[w] = real ? L(A_SEN2, p) : 0;
            cur01[w] = real ? ((int)(uint16_t)row0[sid01[w] & 0xffff]
                               | ((int)(uint16_t)row0[(sid01[w] >> 16) & 0xffff] << 16))
                            : 0;
            cur2[w] = real ? (int)row0[sid2[w]] : 0;
        }
    }
    for (int t = 0; t < U.n_frames; ++t) {
        const int16_t *row = P.senscr + U.scr_off + (long long)t * U.scr_stride;
        const int nf = t + 1;
        int nxt01[WR], nxt2[WR];
        if (WMAX) { /* next frame's scores (the last frame re-reads its own row) */
            const int16_t *rown = row + (nf < U.n_frames ? (size_t)U.scr_stride : 0);
#pragma unroll
            for (int w = 0; w < WR; ++w) {
                bool real = w * 64 + lane < NP;
                nxt01[w] = real ? ((int)(uint16_t)rown[sid01[w] & 0xffff]
                                   | ((int)(uint16_t)rown[(sid01[w] >> 16) & 0xffff] << 16))
                                : 0;
                nxt2[w] = real ? (int)rown[sid2[w]] : 0;
            }
        }
        const bool renorm = align_renorm_due(best_score);
        int bs = SSW_WORST_SCORE;

        /* renormalize_hmms + evaluate_hmms + prune_hmms (state_align_search.c:57-106) */
        const int w_first = (HBM && !renorm) ? wlo : 0;
        const int w_end = WMAX ? WMAX : ((HBM && !renorm) ? whi + 1 : W);
#pragma unroll
        for (int w = w_first; w < w_end; ++w) {
            int p = w * 64 + lane;
            if (p < NP) {
                int s0 = L(A_S0, p), s1 = L(A_S1, p), s2 = L(A_S2, p), os = L(A_OS, p);
                int fr = L(A_FR, p);
                if (renorm) { /* hmm_normalize, src/hmm.c:150-161 */
                    if (s0 > SSW_WORST_SCORE)
                        s0 -= best_score;
                    if (s1 > SSW_WORST_SCORE)
                        s1 -= best_score;
                    if (s2 > SSW_WORST_SCORE)
                        s2 -= best_score;
                    if (os > SSW_WORST_SCORE)
                        os -= best_score;
                }
                if (fr >= t) {
                    int h0 = L(A_H0, p), h1 = L(A_H1, p), h2 = L(A_H2, p), oh = L(A_OH, p);
                    int n0, n1, n2;
                    if (WMAX) {
                        n0 = -(int)(int16_t)(cur01[w < WR ? w : 0] & 0xffff);
                        n1 = -(cur01[w < WR ? w : 0] >> 16);
                        n2 = -cur2[w < WR ? w : 0];
                    } else {
                        int sen01 = L(A_SEN01, p), sen2 = L(A_SEN2, p);
                        n0 = -(int)row[sen01 & 0xffff];
                        n1 = -(int)row[(sen01 >> 16) & 0xffff];
                        n2 = -(int)row[sen2];
                    }
                    int b = vit_eval_3st(s0, s1, s2, h0, h1, h2, os, oh, n0, n1, n2,
                                         (uint32_t)L(A_TPA, p), (uint32_t)L(A_TPB, p),
                                         (uint32_t)L(A_TPC, p));
                    bs = b > bs ? b : bs;
                    L(A_H1, p) = h1;
                    L(A_H2, p) = h2;
                    L(A_OH, p) = oh;
                    if (nf <= L(A_EF, p))
                        L(A_FR, p) = nf;
                }
                L(A_S0, p) = s0;
                L(A_S1, p) = s1;
                L(A_S2, p) = s2;
                L(A_OS, p) = os;
            }
        }
        best_score = wave_max_i32(bs);
        sync_lanes();

        /* phone_transition (state_align_search.c:108-133) as a carry chain, then
         * record_transitions (:149-175).  entered(i+1) = C_i & (A_i | entered(i)) is the carry
         * recurrence of the binary sum X + Y with X = C, Y = A & C. */
        unsigned long long cin = 0;
        int2 *tkrow = tok + (size_t)t * n_states;
        const int w2_first = HBM ? wlo : 0;
        const int w2_end = HBM ? (whi + 2 < W ? whi + 2 : W) : W;
        if (BANDT) { /* this frame's row holds the walked words only */
            const int rw = (w2_end - w2_first) * 192;
            if (tbase + rw > tcap) { /* (wave-uniform) */
                ovf = true;
                break;
            }
            if (lane == 0) {
                TB[t] = (int)tbase;
                TB[t + 1] = (int)(tbase + rw);
                TL[t] = w2_first * 192;
            }
            tkrow = tok + (tbase - (long long)w2_first * 192);
            tbase += rw;
        }
        int nlo = INT_MAX, nhi = -1;
        for (int w = w2_first; w < w2_end; ++w) {
            int p = w * 64 + lane;
            bool valid = p < NP;
            int fr = valid ? L(A_FR, p) : -1;
            bool a_bit = valid && fr == nf;
            bool c_bit = false;
            if (valid && p + 1 < NP) {
                int nfr = L(A_FR, p + 1);
                c_bit = (nf >= L(A_SF, p + 1)) && (nfr < t || L(A_OS, p) > L(A_S0, p + 1));
            }
            unsigned long long A = __ballot(a_bit), Cm = __ballot(c_bit);
            unsigned long long X = Cm, Y = A & Cm;
            unsigned long long S = X + Y + cin;
            unsigned long long E = S ^ X ^ Y; /* bit i: phone (w*64+i) is entered */
            unsigned long long cout = ((X & Y) | ((X | Y) & ~S)) >> 63;
            bool entered = (E >> lane) & 1ull;
            int src_os = 0, src_oh = 0;
            if (valid && entered) { /* p >= 1 whenever entered */
                src_os = L(A_OS, p - 1);
                src_oh = L(A_OH, p - 1);
            }
            sync_lanes(); /* all reads of neighbours done before this word's writes */
            if (valid) {
                if (entered) { /* hmm_enter, src/hmm.c:142-148 */
                    L(A_S0, p) = src_os;
                    L(A_H0, p) = src_oh;
                    L(A_FR, p) = nf;
                    fr = nf;
                }
                int2 k0 = make_int2(-1, -1), k1 = k0, k2 = k0;
                if (fr >= t) {
                    k0 = make_int2(L(A_H0, p), L(A_S0, p));
                    k1 = make_int2(L(A_H1, p), L(A_S1, p));
                    k2 = make_int2(L(A_H2, p), L(A_S2, p));
                    L(A_H0, p) = p * 3;
                    L(A_H1, p) = p * 3 + 1;
                    L(A_H2, p) = p * 3 + 2;
                }
                tkrow[p * 3] = k0;
                tkrow[p * 3 + 1] = k1;
                tkrow[p * 3 + 2] = k2;
            }
            if (HBM && __ballot(valid && fr >= nf) != 0ull) { /* still active next frame */
                nlo = w < nlo ? w : nlo;
                nhi = w;
            }
            cin = cout;
            sync_lanes();
        }
        if (HBM && nhi >= 0) { /* (nothing active: the search has failed, the range stays) */
            wlo = nlo;
            whi = nhi;
        }
        if (WMAX) {
#pragma unroll
            for (int w = 0; w < WR; ++w) {
                cur01[w] = nxt01[w];
                cur2[w] = nxt2[w];
            }
        }
    }

    /* state_align_search_finish (state_align_search.c:215-268) */
    /* the token stack is read back by this workgroup only: workgroup-scope ordering (an
     * agent-scope fence would write back and invalidate the XCD's L2 under the other
     * utterances) */
    __syncthreads();
    if (lane == 0) {
        if (ovf)
            P.status[u] = -(1 << 30); /* the banded table is full: the host takes the full one */
        else
            align_backtrace(P, U, u, tok, n_states, L(A_OH, NP - 1), L(A_OS, NP - 1), TB, TL);
    }
#undef L
}

/* The same search with every phone's HMM in registers (lane = phone, WMAX words of 64 phones):
 * nothing of the frame step goes through LDS; the steps are ssw_align_common.inc's, word by word.
 * All of phone_transition's reads see the state left by evaluate/prune (as in the reference's
 * loop, where hmm i+1 is examined before it is entered); the enters are applied afterwards. */
template <int WMAX>
__global__ void __launch_bounds__(64)
viterbi_align_reg_kernel(AlignParams P)
{
    const int u = blockIdx.x;
    const int lane = threadIdx.x;
    const AlignUtt U = P.utts[u];
    const int NP = U.n_phones;
    const int n_states = NP * 3;

    AlignHmm hm[WMAX];
    AlignPhone phn[WMAX];
    int cur01[WMAX], cur2[WMAX];
    const int16_t *row0 = P.senscr + U.scr_off;
#pragma unroll
    for (int w = 0; w < WMAX; ++w) {
        phn[w] = align_phone_load(w * 64 + lane, NP, U.phone_off, P.tp, P.tmatid, P.senid, P.sf, P.ef);
        hmm_clear(hm[w]);
        const bool have = phn[w].real && U.n_frames > 0;
        cur01[w] = have ? ((int)(uint16_t)row0[phn[w].sid01 & 0xffff]
                           | ((int)(uint16_t)row0[(phn[w].sid01 >> 16) & 0xffff] << 16))
                        : 0;
        cur2[w] = have ? (int)row0[phn[w].sid2] : 0;
    }
    align_search_start(hm[0], phn[0].p);

    int2 *tok = P.tokens + U.tok_off;
    int best_score = 0;
    for (int t = 0; t < U.n_frames; ++t) {
        const int nf = t + 1;
        const int16_t *rown
            = P.senscr + U.scr_off + (long long)(nf < U.n_frames ? nf : t) * U.scr_stride;
        int nxt01[WMAX], nxt2[WMAX];
#pragma unroll
        for (int w = 0; w < WMAX; ++w) {
            nxt01[w] = phn[w].real ? ((int)(uint16_t)rown[phn[w].sid01 & 0xffff]
                                     | ((int)(uint16_t)rown[(phn[w].sid01 >> 16) & 0xffff] << 16))
                                  : 0;
            nxt2[w] = phn[w].real ? (int)rown[phn[w].sid2] : 0;
        }
        int bs = SSW_WORST_SCORE;
        /* (evaluated under a branch, a word at a time: as one block of selects the words'
         * evaluations are interleaved and <4> needs 159 registers instead of 126) */
#pragma unroll
        for (int w = 0; w < WMAX; ++w) {
            AlignHmm &h = hm[w];
            renormalize_hmm(h, best_score);
            if (h.fr >= t) {
                const int b = vit_eval_3st(h.s0, h.s1, h.s2, h.h0, h.h1, h.h2, h.os, h.oh,
                                           -(int)(int16_t)(cur01[w] & 0xffff), -(cur01[w] >> 16),
                                           -cur2[w], phn[w].tpa, phn[w].tpb, phn[w].tpc);
                bs = b > bs ? b : bs;
                if (nf <= phn[w].ef)
                    h.fr = nf;
            }
        }
        best_score = wave_max_i32(bs);

        AlignCarry k[WMAX];
#pragma unroll
        for (int w = 0; w < WMAX; ++w) {
            /* frame and entry score of phone p + 1 */
            const int efr = (w + 1 < WMAX) ? __builtin_amdgcn_readlane(hm[w + 1 < WMAX ? w + 1 : w].fr, 0) : -1;
            const int es0 = (w + 1 < WMAX) ? __builtin_amdgcn_readlane(hm[w + 1 < WMAX ? w + 1 : w].s0, 0) : 0;
            k[w] = phone_transition(hm[w], phn[w], NP, efr, es0, t);
        }
        int cin = 0;
        int2 *tkrow = tok + (size_t)t * n_states;
        int prev_os = 0, prev_oh = 0; /* exit score/history of the last phone of the previous word */
#pragma unroll
        for (int w = 0; w < WMAX; ++w) {
            const int p = phn[w].p;
            int c_out;
            const bool e_bit = phone_entered(k[w], cin, lane, &c_out);
            cin = c_out;
            hmm_enter(hm[w], phn[w].real && e_bit, nf, prev_os, prev_oh);
            prev_os = __builtin_amdgcn_readlane(hm[w].os, 63); /* (an enter leaves the exit alone) */
            prev_oh = __builtin_amdgcn_readlane(hm[w].oh, 63);
            int2 k0, k1, k2;
            record_transitions(hm[w], p, t, k0, k1, k2);
            if (phn[w].real) {
                tkrow[p * 3] = k0;
                tkrow[p * 3 + 1] = k1;
                tkrow[p * 3 + 2] = k2;
            }
        }
#pragma unroll
        for (int w = 0; w < WMAX; ++w) {
            cur01[w] = nxt01[w];
            cur2[w] = nxt2[w];
        }
    }

    /* state_align_search_finish (state_align_search.c:215-268) */
    const int lw = (NP - 1) >> 6, ll = (NP - 1) & 63;
    int fin_oh = -1, fin_os = SSW_WORST_SCORE;
#pragma unroll
    for (int w = 0; w < WMAX; ++w)
        if (w == lw) {
            fin_oh = __shfl(hm[w].oh, ll, WAVE);
            fin_os = __shfl(hm[w].os, ll, WAVE);
        }
    /* the token stack is read back by this workgroup only: workgroup-scope ordering (an
     * agent-scope fence would write back and invalidate the XCD's L2 under the other
     * utterances) */
    __syncthreads();
    if (lane == 0)
        align_backtrace(P, U, u, tok, n_states, fin_oh, fin_os);
}

/* One wave per 64-phone word of the utterance (workgroup = n_words waves, up to 16): the frame
 * step of every word runs in parallel, HMMs in registers as above, the waves meeting twice per
 * frame at the exchange slots (ssw_align_common.inc).  This kernel adds the reference's tokens:
 * three {history, score} per phone and frame, [n_frames][n_states]. */
__global__ void __launch_bounds__(64 * SSW_ALIGN_MAX_WAVES)
viterbi_align_mw_kernel(AlignParams P)
{
    __shared__ AlignExchange x;
    __shared__ int x_fin[2];
    const int u = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    const AlignUtt U = P.utts[u];
    const int NP = U.n_phones;
    const int n_states = NP * 3;
    const AlignPhone phn =
        align_phone_load(w * 64 + lane, NP, U.phone_off, P.tp, P.tmatid, P.senid, P.sf, P.ef);
    const ScoreAhead sa = {P.senscr, U.scr_off, U.scr_stride, U.n_frames - 1};
    AlignHmm hm;
    hmm_clear(hm);
    uint32_t a0 = 0, a1 = 0, a2 = 0, b0 = 0, b1 = 0, b2 = 0, c0 = 0, c1 = 0, c2 = 0;
    if (U.n_frames > 0) { /* (uniform) an empty utterance has no row to read */
        score_fetch(sa, phn, 0, a0, a1, a2);
        score_fetch(sa, phn, 1, b0, b1, b2);
    }
    align_search_start(hm, phn.p);
    exchange_init(x);
    __syncthreads();
    int2 *tok = P.tokens + U.tok_off;
    int best_score = 0;
    int2 *tkrow = tok + (phn.real ? phn.p * 3 : 0);
    auto frame = [&](const int t, uint32_t raw0, uint32_t raw1, uint32_t raw2, uint32_t &fut0,
                     uint32_t &fut1, uint32_t &fut2) {
        const int nf = t + 1, par = t & 1;
        int n0, n1, n2;
        score_step(sa, phn, t, raw0, raw1, raw2, fut0, fut1, fut2, n0, n1, n2);
        renormalize_hmm(hm, best_score);
        const int b = evaluate_hmm(hm, phn, t, n0, n1, n2);
        exchange_publish(x, par, w, lane, b, hm);
        lds_barrier();
        /* everything the barrier published, requested at once: the 16 best-score slots and the
         * next word's boundary */
        const bool has_next = w + 1 < nw;
        const int wnx = has_next ? w + 1 : w;
        const int efr = x.fr0[par][wnx], es0 = x.s00[par][wnx];
        best_score = exchange_best_score(x, par);
        const AlignCarry k = phone_transition(hm, phn, NP, has_next ? efr : -1, es0, t);
        if (lane == 0)
            x.gp[par][w] = k.code;
        lds_barrier();
        const int wpv = w > 0 ? w - 1 : 0;
        const int code = x.gp[par][lane & (SSW_ALIGN_MAX_WAVES - 1)];
        const int pos = x.os63[par][wpv], poh = x.oh63[par][wpv];
        const int cin = carry_into_word(code, w, SSW_ALIGN_MAX_WAVES);
        hmm_enter(hm, phn.real && phone_entered(k, cin, lane), nf, pos, poh);
        int2 k0, k1, k2;
        record_transitions(hm, phn.p, t, k0, k1, k2);
        if (phn.real) {
            tkrow[0] = k0;
            tkrow[1] = k1;
            tkrow[2] = k2;
        }
        tkrow += n_states;
    };
    for (int t = 0; t < U.n_frames; t += 3) { /* the same trip count in every wave: barriers */
        frame(t, a0, a1, a2, c0, c1, c2);
        if (t + 1 < U.n_frames)
            frame(t + 1, b0, b1, b2, a0, a1, a2);
        if (t + 2 < U.n_frames)
            frame(t + 2, c0, c1, c2, b0, b1, b2);
    }

    /* state_align_search_finish (state_align_search.c:215-268) */
    if (phn.p == NP - 1) {
        x_fin[0] = hm.oh;
        x_fin[1] = hm.os;
    }
    /* the token stack is read back by this workgroup only: workgroup-scope ordering (an
     * agent-scope fence would write back and invalidate the XCD's L2 under the other
     * utterances) */
    __syncthreads();
    if (threadIdx.x == 0)
        align_backtrace(P, U, u, tok, n_states, x_fin[0], x_fin[1]);
}

/* Round 5: the wave-per-word kernel with BYTE TOKENS.
 *
 * The reference records a token {history, score} per state and frame (src/state_align_search.c:
 * 149-175): 8 bytes x 450 states x 1000 frames = 3.6 MB per utterance, and at 2048 utterances
 * the kernel above is bound by writing them (profiles/r05_align_pmc_2048.json: 7.4 GB written,
 * 3.4 ms of the call even with compact score rows).  The backtrace (:215-268) reads ONE token per
 * frame, and what it reads is redundant:
 *   - history.  Before a frame is evaluated every active HMM's histories are its own state ids
 *     (record_transitions resets them, :168-172), so what hmm_vit_eval_3st_lr leaves in state j
 *     is the id of state j, j - 1 or j - 2 of the same phone, or -- state 0 of an entered phone
 *     -- state 2 or 1 of the phone before (hmm_out_history): own id minus 0, 1 or 2, or -1.
 *     Two bits per state, ONE BYTE per phone and frame: 150 B instead of 3,600 B per frame.
 *   - score.  Only the scores at the path's state changes enter the result (score of a segment =
 *     path score at its end - at its start), and a path score is the sum along the path of
 *     -senone score + transition, clamped at WORST, minus the renormalisations: once the path is
 *     known it is REPLAYED -- one score gather per frame instead of 450 token writes.
 * The replay equals the token scores as long as every score on the path was derived, in its
 * frame, from its predecessor's score of that frame.  The reference's quirks that break this are
 * detected in the forward pass and end the utterance with status -(1 << 30), upon which the host
 * runs it through the kernel above (full tokens), it alone:
 *   (1) an HMM entered with an exit score that was not computed in this frame (the exit block
 *       only runs when state 1 is alive, src/hmm.c:504-517; the cascade of phone_transition
 *       enters a phone from one that was itself only just entered) -- unless that score's
 *       history is -1, which ends any path through it;
 *   (2) an inactive HMM entered again while its states 1 / 2 still hold scores (hmm_enter only
 *       sets state 0, src/hmm.c:142-148);
 *   (3) state 2 taking the exit block's t2 when the model has no 0 -> 2 arc (the un-reset t2 of
 *       :496-520: state 1's score under state 0's history).
 * And whatever else might: the replayed score of the final state must EQUAL the forward pass's,
 * checked before any result is written; a backtrace that runs into a missing token also goes to
 * the other kernel (the reference's partial results in that case need the token scores).
 * Neither shipped model has skip arcs, and alignment_populate's windows never re-enter a phone:
 * on the round's soaks no utterance took the fall-back (profiles/r05_*_soak_align*.json). */
__global__ void __launch_bounds__(64 * SSW_ALIGN_MAX_WAVES)
viterbi_align_mwb_kernel(AlignParams P)
{
    __shared__ AlignExchange x;
    /* beside os63 / oh63: was that exit score computed in this frame? */
    __shared__ int x_fresh63[2][SSW_ALIGN_MAX_WAVES];
    __shared__ int x_fin[2], x_irr;
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[64 * 128]; /* backtrace: 64 frames x 128 phones */
    const int u = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    const AlignUtt U = P.utts[u];
    const int NP = U.n_phones;
    const int W = SSW_WORST_SCORE;
    const int n_frames = U.n_frames;
    /* the utterance's byte tokens, renormalisation amounts and path (AlignParams::btok) */
    const int tstride = nw * 64;
    uint8_t *tb = P.btok + U.tok_off;
    int *norm_a = reinterpret_cast<int *>(tb + (((size_t)n_frames * tstride + 255) & ~(size_t)255));
    uint16_t *qpath = reinterpret_cast<uint16_t *>(norm_a + n_frames);

    const AlignPhone phn =
        align_phone_load(w * 64 + lane, NP, U.phone_off, P.tp, P.tmatid, P.senid, P.sf, P.ef);
    const ScoreAhead sa = {P.senscr, U.scr_off, U.scr_stride, n_frames - 1};
    AlignHmm hm;
    hmm_clear(hm);
    uint32_t a0 = 0, a1 = 0, a2 = 0, b0 = 0, b1 = 0, b2 = 0, c0 = 0, c1 = 0, c2 = 0;
    if (n_frames > 0) {
        score_fetch(sa, phn, 0, a0, a1, a2);
        score_fetch(sa, phn, 1, b0, b1, b2);
    }
    align_search_start(hm, phn.p);
    exchange_init(x);
    if (threadIdx.x == 0)
        x_irr = 0;
    __syncthreads();
    int best_score = 0;
    bool irr = false; /* this lane saw something the replay cannot follow */
    uint8_t *tkrow = tb + phn.p; /* p < tstride always: lanes without a phone write "no token" */
    auto frame = [&](const int t, uint32_t raw0, uint32_t raw1, uint32_t raw2, uint32_t &fut0,
                     uint32_t &fut1, uint32_t &fut2) {
        const int nf = t + 1, par = t & 1;
        int n0, n1, n2;
        score_step(sa, phn, t, raw0, raw1, raw2, fut0, fut1, fut2, n0, n1, n2);
        /* the amount goes on record */
        const int amount = renormalize_hmm(hm, best_score);
        if (threadIdx.x == 0)
            norm_a[t] = amount;
        const bool active = hm.fr >= t;
        bool a1_live, quirk;
        const int b = evaluate_hmm(hm, phn, t, n0, n1, n2, &a1_live, &quirk);
        irr = irr || (active && quirk);                         /* (3) */
        const bool fresh = active && a1_live; /* this frame's exit score is this frame's */
        exchange_publish(x, par, w, lane, b, hm);
        if (lane == 63)
            x_fresh63[par][w] = fresh ? 1 : 0;
        lds_barrier();
        const bool has_next = w + 1 < nw;
        const int wnx = has_next ? w + 1 : w;
        const int efr = x.fr0[par][wnx], es0 = x.s00[par][wnx];
        best_score = exchange_best_score(x, par);
        const AlignCarry k = phone_transition(hm, phn, NP, has_next ? efr : -1, es0, t);
        if (lane == 0)
            x.gp[par][w] = k.code;
        lds_barrier();
        const int wpv = w > 0 ? w - 1 : 0;
        const int code = x.gp[par][lane & (SSW_ALIGN_MAX_WAVES - 1)];
        const int pos = x.os63[par][wpv], poh = x.oh63[par][wpv], pfr = x_fresh63[par][wpv];
        const int cin = carry_into_word(code, w, SSW_ALIGN_MAX_WAVES);
        const bool entered = phn.real && phone_entered(k, cin, lane);
        const int src_fresh = lane_from_prev(fresh ? 1 : 0, pfr);
        irr = irr || (entered && !active && (hm.s1 > W || hm.s2 > W)); /* (2) */
        hmm_enter(hm, entered, nf, pos, poh);
        /* (1); h0 is the history it entered with */
        irr = irr || (entered && src_fresh == 0 && hm.h0 != -1);
        uint8_t token;
        const bool two_bits = record_transitions_2bit(hm, phn.p, t, token);
        irr = irr || !two_bits;
        tkrow[0] = token;
        tkrow += tstride;
    };
    for (int t = 0; t < n_frames; t += 3) { /* the same trip count in every wave: barriers */
        frame(t, a0, a1, a2, c0, c1, c2);
        if (t + 1 < n_frames)
            frame(t + 1, b0, b1, b2, a0, a1, a2);
        if (t + 2 < n_frames)
            frame(t + 2, c0, c1, c2, b0, b1, b2);
    }

    /* state_align_search_finish (state_align_search.c:215-268) */
    if (phn.p == NP - 1) {
        x_fin[0] = hm.oh;
        x_fin[1] = hm.os;
    }
    if (__ballot(irr) != 0ull && lane == 0)
        atomicOr(&x_irr, 1);
    /* tokens are read back by this workgroup only: workgroup-scope ordering (as above) */
    __syncthreads();
    if (w != 0)
        return;
    if (x_irr != 0) {
        if (lane == 0)
            P.status[u] = -(1 << 30);
        return;
    }
    const int final_id = x_fin[0], fin_os = x_fin[1];
    if (final_id == -1) { /* "Failed to reach final state" */
        if (lane == 0)
            P.status[u] = -1;
        return;
    }
    /* ---- the path: q[f] = state occupied in frame f, walked back through the byte tokens in
     * tiles of 64 frames x 128 phones (a frame moves the path by one phone at most) staged in LDS;
     * the walk itself is scalar code on one broadcast LDS read per frame ---- */
    int id = final_id;
    if (lane == 0)
        qpath[n_frames - 1] = (uint16_t)id;
    bool lost = false; /* (wave-uniform) */
    for (int hi = n_frames - 2; hi >= 0 && !lost; hi -= 64) {
        const int f = hi - 63 + lane; /* token row f gives q[f] from q[f + 1] */
        const int ph = id / 3;
        const int pb = ph >= 64 ? ((ph >> 6) - 1) << 6 : 0; /* window [pb, pb + 128) holds ph - 64 .. ph */
        {
            const uint4 *src = reinterpret_cast<const uint4 *>(tb + (size_t)(f < 0 ? 0 : f) * tstride + pb);
            const bool second = pb + 64 < tstride; /* the row may end after the window's first half */
            uint4 v[8];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                v[k] = src[k];
#pragma unroll
            for (int k = 4; k < 8; ++k)
                v[k] = second ? src[k] : make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
            uint4 *dst = reinterpret_cast<uint4 *>(s_tile + lane * 128);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                dst[k] = v[k];
        }
        wave_sync();
        int qv = 0;
        for (int l = 63; l >= 0; --l) {
            if (hi - 63 + l < 0)
                break;
            const int pp = id / 3, j = id - pp * 3;
            const int byte = __builtin_amdgcn_readfirstlane((int)s_tile[l * 128 + (pp - pb)]);
            const int d = (byte >> (2 * j)) & 3;
            if (d == 3) { /* "Alignment failed in frame": the reference's partial results need
                           * the token scores -> the other kernel */
                lost = true;
                break;
            }
            id -= d;
            qv = lane == l ? id : qv; /* (no v_writelane builtin in this compiler) */
        }
        if (!lost && f >= 0)
            qpath[f] = (uint16_t)qv;
        wave_sync();
    }
    if (lost) {
        if (lane == 0)
            P.status[u] = -(1 << 30);
        return;
    }
    /* ---- the replay: pass 0 only checks that the path's score arrives at the forward pass's
     * final score, pass 1 writes the entries.  64 frames at a time: every lane prepares its
     * frame's increment (one score gather + the transition), the running score is scalar code
     * over v_readlane, and a lane whose frame ends a segment (the state changes, or the
     * utterance ends) writes that state's entry: start, duration, score at the end - at the
     * start, the start taken from the nearest segment end below it ---- */
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); /* qpath: written by other lanes */
    ssw_align_entry_t *st = P.state_io + (size_t)U.phone_off * 3;
    for (int pass = 0; pass < 2; ++pass) {
        int y = 0, seg_a = 0, seg_ya = 0; /* running score; start (frame, score) of the open segment */
        for (int f0 = 0; f0 < n_frames; f0 += 64) {
            const int f = f0 + lane;
            const bool valid = f < n_frames;
            const int fc = valid ? f : n_frames - 1;
            const int q = (int)__hip_atomic_load(qpath + fc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int qn = fc + 1 < n_frames
                ? (int)__hip_atomic_load(qpath + fc + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                : -2; /* the exit out of the last phone */
            const int pp = q / 3, j = q - pp * 3;
            const int gq = U.phone_off + pp;
            const uint32_t tpw = (reinterpret_cast<const uint32_t *>(P.tp) + (size_t)P.tmatid[gq] * 3)[j];
            const int col = (qn >= 0 && qn / 3 == pp) ? qn - pp * 3 : 3; /* 3: the exit arc */
            const int tpv = -(int)((tpw >> (8 * col)) & 0xffu);
            const int sc = (int)P.senscr[U.scr_off + (long long)fc * U.scr_stride + P.senid[gq * 3 + j]];
            const int inc = valid ? tpv - sc : 0;
            const int R = valid ? norm_a[fc] : 0;
            const bool bnd = valid && qn != q;
            int yv = 0;
            const int cnt = n_frames - f0 < 64 ? n_frames - f0 : 64;
            for (int i = 0; i < cnt; ++i) {
                const int r = __builtin_amdgcn_readlane(R, i);
                if (r != 0 && y > W)
                    y -= r; /* hmm_normalize at the top of the frame */
                y += __builtin_amdgcn_readlane(inc, i);
                y = y < W ? W : y;
                yv = lane == i ? y : yv;
            }
            const unsigned long long bm = __ballot(bnd);
            if (pass == 1 && bnd) {
                const unsigned long long lower = bm & ((1ull << lane) - 1ull);
                const int pl = lower != 0ull ? 63 - __builtin_clzll(lower) : 0;
                const int a_in = f0 + pl + 1, ya_in = __shfl(yv, pl, WAVE);
                const int a = lower != 0ull ? a_in : seg_a;
                const int ya = lower != 0ull ? ya_in : seg_ya;
                if (a == 0) { /* the first segment: the reference sets start and duration only */
                    st[0].start = 0;
                    st[0].duration = f + 1;
                } else {
                    st[q].start = a;
                    st[q].duration = f + 1 - a;
                    st[q].score = yv - ya;
                }
            }
            if (bm != 0ull) {
                const int ll = 63 - __builtin_clzll(bm);
                seg_a = f0 + ll + 1;
                seg_ya = __builtin_amdgcn_readlane(yv, ll);
            }
        }
        if (pass == 0 && y != fin_os) { /* the replay does not follow this path: the other kernel */
            if (lane == 0)
                P.status[u] = -(1 << 30);
            return;
        }
    }
    if (lane == 0)
        P.status[u] = 0;
}

/* Round 3: utterances of ANY length with the HMMs in registers -- the wave-per-word kernel above
 * on a SLIDING WINDOW of nw 64-phone blocks (a page of 2,000 words is 13 K phones = 209 blocks,
 * of which a frame has one or two active when the phones carry the first pass's windows).
 * Wave w holds block g with g = w (mod nw), g in [glo, glo + nw): when every phone of the
 * window's first blocks has gone inactive for good (the search is left to right: nothing below
 * the lowest active phone can be entered again) those waves take the blocks that follow the
 * window's end -- per-phone constants reloaded, HMMs cleared, the two score sets in flight
 * requested again.  Exchange slots stay indexed by wave; block b's neighbours are the waves of
 * b - 1 and b + 1; the carry-lookahead reads the slots in window order.
 * Tokens go to the banded table of viterbi_align_kernel<0, true> (TB / TL per frame, band =
 * the blocks from the lowest active one to the one after the highest: the block a transition
 * can enter).  Anything the window or the band cannot hold -- an active range beyond nw - 1
 * blocks, a transition cascade that crosses a whole block in one frame, the token budget -- ends
 * the utterance with status -(1 << 30) and the host runs the batch through the kernels that
 * keep their state in LDS / HBM. */
__global__ void __launch_bounds__(64 * SSW_ALIGN_MAX_WAVES)
viterbi_align_win_kernel(AlignParams P)
{
    __shared__ AlignExchange x;
    /* beside bs: has the wave's block an active phone? */
    __shared__ int x_act[2][SSW_ALIGN_MAX_WAVES];
    __shared__ int x_fin[2], x_ovf[2];
    const int u = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6, nwm = nw - 1; /* nw is a power of two (host) */
    const AlignUtt U = P.utts[u];
    const int NP = U.n_phones;
    const int n_states = NP * 3;
    const int NB = (NP + 63) >> 6;
    const int W = SSW_WORST_SCORE;
    int g = w, glo = 0; /* this wave's block; the window's first block */
    AlignPhone phn;
    AlignHmm hm;
    auto load_block = [&](int gb) { /* the block's phones: constants in, hmm_clear */
        phn = align_phone_load(gb * 64 + lane, NP, U.phone_off, P.tp, P.tmatid, P.senid, P.sf, P.ef);
        hmm_clear(hm);
    };
    load_block(g);
    const ScoreAhead sa = {P.senscr, U.scr_off, U.scr_stride, U.n_frames - 1};
    uint32_t a0 = 0, a1 = 0, a2 = 0, b0 = 0, b1 = 0, b2 = 0, c0 = 0, c1 = 0, c2 = 0;
    if (U.n_frames > 0) {
        score_fetch(sa, phn, 0, a0, a1, a2);
        score_fetch(sa, phn, 1, b0, b1, b2);
    }
    align_search_start(hm, phn.p);
    if (threadIdx.x == 0) {
        x_fin[0] = -1;
        x_fin[1] = W;
        x_ovf[0] = x_ovf[1] = 0;
    }
    exchange_init(x);
    int2 *tok = P.tokens + U.tok_off;
    int *TB = P.band_ws + 2 * (size_t)U.frame_off + 2 * (size_t)u;
    int *TL = TB + U.n_frames + 1;
    long long tbase = 0;
    const long long tcap =
        (long long)U.n_frames * (n_states < P.band_tokens ? n_states : P.band_tokens);
    int best_score = 0;
    bool ovf = false;
    __syncthreads();

    auto frame = [&](const int t, uint32_t raw0, uint32_t raw1, uint32_t raw2, uint32_t &nx0,
                     uint32_t &nx1, uint32_t &nx2, uint32_t &fut0, uint32_t &fut1, uint32_t &fut2) {
        const int nf = t + 1, par = t & 1;
        int n0, n1, n2;
        score_step(sa, phn, t, raw0, raw1, raw2, fut0, fut1, fut2, n0, n1, n2);
        renormalize_hmm(hm, best_score);
        const bool any_active = __ballot(hm.fr >= t) != 0ull;
        const int b = evaluate_hmm(hm, phn, t, n0, n1, n2);
        exchange_publish(x, par, w, lane, b, hm);
        if (lane == 0)
            x_act[par][w] = any_active ? 1 : 0;
        lds_barrier();
        /* window order: position k is block glo + k, held by wave (k + r) % nw.  Everything the
         * barrier published is requested at once */
        const int r = glo & nwm;
        const int wk = (lane + r) & nwm;
        const int wn = (w + 1) & nwm, wp = (w - 1) & nwm;
        const int act_ = x_act[par][wk];
        const int efr = x.fr0[par][wn], es0 = x.s00[par][wn];
        best_score = exchange_best_score(x, par);
        const unsigned long long M = __ballot(act_ != 0) & ((1ull << nw) - 1ull);
        const int kpos = (w - r) & nwm;
        const int kmin = M ? __builtin_ctzll(M) : 0;
        const int kmax = M ? 63 - __builtin_clzll(M) : -1;
        /* the band of this frame's tokens: the active blocks and the one a transition can enter */
        int kend = kmax + 1;
        if (kend > nw - 1) { /* the block after the highest active one must be in the window */
            if (glo + kend < NB)
                ovf = true;
            kend = nw - 1;
        }
        kend = glo + kend > NB - 1 ? NB - 1 - glo : kend;
        const int nblk = M ? kend - kmin + 1 : 0;
        if (tbase + (long long)nblk * 192 > tcap)
            ovf = true;

        const bool has_next = kpos + 1 < nw; /* else: a block beyond the window, never entered */
        const AlignCarry k = phone_transition(hm, phn, NP, has_next ? efr : -1, es0, t);
        if (lane == 0)
            x.gp[par][w] = k.code;
        lds_barrier();
        const int code = x.gp[par][wk];
        const int pos = x.os63[par][wp], poh = x.oh63[par][wp];
        const int cin = carry_into_word(code, kpos, nw);
        int c_out;
        const bool e_bit = phone_entered(k, cin, lane, &c_out);
        const bool entered = phn.real && e_bit;
        /* a transition out of the window's last block, or into a block beyond the token band */
        if ((kpos == nw - 1 && c_out && g + 1 < NB) || (kpos > kend && __ballot(entered) != 0ull))
            ovf = true;
        hmm_enter(hm, entered, nf, pos, poh);
        int2 k0, k1, k2;
        record_transitions(hm, phn.p, t, k0, k1, k2);
        const bool in_band = M != 0ull && kpos >= kmin && kpos <= kend;
        if (phn.real && in_band && !ovf) {
            int2 *tkrow = tok + tbase + (long long)(kpos - kmin) * 192 + lane * 3;
            tkrow[0] = k0;
            tkrow[1] = k1;
            tkrow[2] = k2;
        }
        if (threadIdx.x == 0 && !ovf) {
            TB[t] = (int)tbase;
            TL[t] = (glo + kmin) * 192;
        }
        tbase += (long long)nblk * 192;
        if (ovf && lane == 0)
            x_ovf[par] = 1; /* read by every wave after the NEXT frame's first barrier */
        /* slide: the blocks below the lowest active one are done */
        if (M != 0ull && kmin > 0) {
            glo += kmin;
            if (kpos < kmin) {
                g += nw;
                load_block(g);
                score_fetch(sa, phn, t + 1, nx0, nx1, nx2);
                score_fetch(sa, phn, t + 2, fut0, fut1, fut2);
            }
        }
    };
    /* the same trip count in every wave (barriers); an overflow seen by one wave reaches the
     * others through x_ovf one barrier later, and all leave together at the end of a triple */
    int t = 0;
    for (; t < U.n_frames; t += 3) {
        frame(t, a0, a1, a2, b0, b1, b2, c0, c1, c2);
        if (t + 1 < U.n_frames)
            frame(t + 1, b0, b1, b2, c0, c1, c2, a0, a1, a2);
        if (t + 2 < U.n_frames)
            frame(t + 2, c0, c1, c2, a0, a1, a2, b0, b1, b2);
        lds_barrier(); /* (LDS only: the token stores in flight are not waited for) */
        if (x_ovf[0] | x_ovf[1])
            break;
    }
    if (g == NB - 1 && lane == ((NP - 1) & 63)) {
        x_fin[0] = hm.oh;
        x_fin[1] = hm.os;
    }
    if (threadIdx.x == 0)
        TB[U.n_frames] = (int)tbase; /* end of the last frame's row (a global store, read back by
                                      * this thread below) */
    __syncthreads();
    if (threadIdx.x == 0) {
        if (x_ovf[0] | x_ovf[1])
            P.status[u] = -(1 << 30);
        else
            align_backtrace(P, U, u, tok, n_states, x_fin[0], x_fin[1], TB, TL);
    }
}
