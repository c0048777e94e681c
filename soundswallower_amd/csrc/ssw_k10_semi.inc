/* ssw_k10_semi.inc -- K10: the s2_semi scorer of single-codebook (semi-continuous) models.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order).
 *
 * Restates s2_semi_mgau_frame_eval (src/s2_semi_mgau.c:829-875) for batches, in three kernels:
 *   semi_density_kernel  parallel over frames: every density of every stream exactly (unfused
 *                        float32, dimensions in index order, :126-142); per (frame, stream) it
 *                        leaves every density's truncated score and tie bit, and the frame's
 *                        CANDIDATES: the densities at or above the frame's topn-th best truncated
 *                        score, in index order.  Where those are exactly topn densities of topn
 *                        different scores (ds = 1) the frame's list is settled here: it does not
 *                        depend on the history
 *   semi_chain_kernel    one wave per (utterance, stream): the only sequential part.  Applies
 *                        eval_topn (:68-108) and eval_cb (:110-169) to the candidates and hands the
 *                        codeword order on, through the reference's ring of two history slots
 *                        (:845-855).  With ds = 1 and a reset at every utterance it visits only the
 *                        frames with a tie, each from its predecessor's stored order; with ds > 1
 *                        or the history carried over utterance boundaries, every frame in order
 *   semi_senone_kernel   parallel over frames: mgau_norm (:184-202, topn_beam = 0) and
 *                        get_scores_8b_feat_all (:425-443)
 *
 * Why the candidates are enough.  Call S the topn-th largest truncated score of a frame and
 * stream.  eval_cb inserts a density whose truncated score s is above the list's worst score w
 * whatever the history was (semi_accepts below), and the list's worst score never falls; so once
 * eval_cb has passed the last density, the list holds topn entries >= S, and every entry below S
 * -- a carried codeword, or a density below S that was let in early -- has been pushed out
 * without ever standing before an entry >= S.  What such an entry scored exactly therefore does
 * not matter: the chain looks a carried codeword up among the candidates and takes INT_MIN for
 * one it does not find.  That needs every density at or above S among the candidates; a frame
 * with more than 64 of them (ties, or a NaN row whose densities all truncate to INT_MIN) is marked
 * and walked from the whole row instead.  On a frame that down-sampling skips (frame % ds != 0:
 * eval_topn only, :176-178) the carried codewords keep their places, and their scores are read
 * from the whole row.
 *
 * Equality with the reference is claimed for finite features: then the partial sums of a density
 * never increase (the scaled variances are positive), which is what turns eval_cb's test before
 * every dimension into one test of the sum before the last (semi_tie_bit).  A NaN or infinite
 * feature gives a deterministic row -- everything is a function of the stored scores -- and no
 * fault: every index is bounded by construction, not by the data. */

struct SemiParams {
    const float *rec;            /* [n_feat][SSW_SC_ROWS][SSW_SC_MAX_DENSITY], ssw_model.c */
    const float *feats;          /* [n_frames][featdim] */
    const int *utt_off;          /* [n_utts + 1] */
    const uint32_t *carry_pk;    /* optional [n_utts][n_feat] packed codeword order to start from */
    int *row_dint;               /* [n_frames][n_feat][SSW_SC_MAX_DENSITY] truncated scores */
    unsigned long long *row_tie; /* [n_frames][n_feat][4] tie bits, a word per 64 densities */
    int2 *cand;                  /* [n_frames][n_feat][64]: .x score, .y codeword | SEMI_* bits */
    uint8_t *hard;               /* [n_feat][n_frames]: 1 = the frame's list depends on the history */
    uint32_t *topn_cw;           /* [n_frames][n_feat] topn codewords packed, best first */
    int4 *topn_sc;               /* [n_frames][n_feat] their raw scores (INT_MIN beyond topn) */
    const uint8_t *mixw;         /* [n_feat][n_density][sc_stride] */
    const uint8_t *logadd8;      /* [256] */
    int16_t *out;                /* [n_frames][n_sen] */
    int n_utts, n_frames, n_feat, n_density, featdim, ds, frame_base, chain_utts, topn, n_sen,
        sc_stride;
    int featoff[SSW_MAX_FEAT], veclen[SSW_MAX_FEAT];
};

constexpr int SEMI_TIE = 1 << 8;    /* cand.y: the density's tie bit */
constexpr int SEMI_VALID = 1 << 9;  /* the slot holds a candidate */
constexpr int SEMI_WHOLE = 1 << 10; /* more than 64 candidates: walk the whole row */
constexpr int SEMI_FR = 4;          /* frames a wave of the density kernel evaluates per record read */

/* ---------------------------------------------------------------------------------- */
/* eval_cb's accept rule (src/s2_semi_mgau.c:136-154), once                             */
/* ---------------------------------------------------------------------------------- */
/* The reference walks a density's dimensions while d >= (float)worst.score, tested BEFORE every
 * dimension and not after the last, then rejects on the integer: (int32)d < worst.score.  For
 * finite features the partial sums never increase, so the walk's tests come down to the sum
 * before the last dimension, `pre`.  With s = (int32)d and w = worst.score -- itself a truncated
 * float or INT_MIN, so (float)w is exact:
 *   s > w   d > s - 1 >= w (d < 0: s = ceil d; d >= 0: s <= d), and pre >= d: always inserted
 *   s == w  the integer test passes; the walk's test is pre >= (float)s, one bit per density
 *           (PTM's d >= thresh rejects a d in (w - 1, w); this rule accepts it)
 *   s < w   rejected */
__device__ __forceinline__ bool
semi_tie_bit(float pre, int s)
{
    return pre >= (float)s; /* (false for a NaN) */
}

__device__ __forceinline__ bool
semi_accepts(int s, bool tie_bit, int w)
{
    return s > w || (s == w && tie_bit);
}

/* ---------------------------------------------------------------------------------- */
/* densities                                                                           */
/* ---------------------------------------------------------------------------------- */
/* One wave per (group of SEMI_FR frames, stream); lane l holds densities l, 64 + l, 128 + l and
 * 192 + l of the stream.  grid: ceil(n_frames / SEMI_FR) * n_feat waves, four to a workgroup. */
__global__ void __launch_bounds__(256)
semi_density_kernel(SemiParams P)
{
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int groups = (P.n_frames + SEMI_FR - 1) / SEMI_FR;
    if (w >= groups * P.n_feat)
        return;
    const int f = w % P.n_feat, t0 = (w / P.n_feat) * SEMI_FR;
    const int vl = P.veclen[f];
    const float *rec = P.rec + (size_t)f * SSW_SC_ROWS * SSW_SC_MAX_DENSITY;
    const float *xrow[SEMI_FR];
    float d[SEMI_FR][4], pre[SEMI_FR][4];
#pragma unroll
    for (int r = 0; r < SEMI_FR; ++r) {
        /* (a group's frames beyond the batch re-read its last frame; nothing of them is stored) */
        const int t = t0 + r < P.n_frames ? t0 + r : P.n_frames - 1;
        xrow[r] = P.feats + (size_t)t * P.featdim + P.featoff[f];
#pragma unroll
        for (int h = 0; h < 4; ++h)
            pre[r][h] = d[r][h]
                = rec[(size_t)(2 * SSW_SC_MAX_VECLEN) * SSW_SC_MAX_DENSITY + h * 64 + lane];
    }
    for (int j = 0; j < vl; ++j) {
        float mean[4], scale[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            mean[h] = rec[(size_t)j * SSW_SC_MAX_DENSITY + h * 64 + lane];
            scale[h] = rec[(size_t)(SSW_SC_MAX_VECLEN + j) * SSW_SC_MAX_DENSITY + h * 64 + lane];
        }
#pragma unroll
        for (int r = 0; r < SEMI_FR; ++r) {
            const float x = xrow[r][j];
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                pre[r][h] = d[r][h]; /* (after the loop: the sum before the last dimension) */
                const float diff = x - mean[h];
                const float sq = diff * diff;
                const float c = sq * scale[h];
                d[r][h] = d[r][h] - c;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < SEMI_FR; ++r) {
        const int t = t0 + r;
        if (t >= P.n_frames)
            break;
        const size_t pair = (size_t)t * P.n_feat + f;
        int iv[4];
        bool valid[4], tie[4], elig[4];
        unsigned long long tiew[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            valid[h] = h * 64 + lane < P.n_density;
            iv[h] = valid[h] ? dens2int(d[r][h]) : INT_MIN;
            tie[h] = valid[h] && semi_tie_bit(pre[r][h], iv[h]);
            tiew[h] = __ballot(tie[h]);
            P.row_dint[pair * SSW_SC_MAX_DENSITY + h * 64 + lane] = iv[h];
            elig[h] = valid[h];
        }
        if (lane < 4)
            P.row_tie[pair * 4 + lane] = lane == 0 ? tiew[0] : lane == 1 ? tiew[1]
                : lane == 2                        ? tiew[2]
                                                   : tiew[3];
        /* S: the topn-th largest truncated score, counted with its repeats */
        int S = INT_MIN, total = 0;
        /* a frame whose topn best truncated scores all differ and leave no tie at the boundary is
         * EASY: its final list is those densities in score order whatever the history was (see
         * the head of this file) -- written here, and the chain never visits the frame */
        bool easy = P.ds == 1 && !P.chain_utts;
        int ecw[4] = { 0, 0, 0, 0 }, esc[4] = { INT_MIN, INT_MIN, INT_MIN, INT_MIN };
        for (int round = 0; round < P.topn; ++round) {
            int lm = INT_MIN;
            bool any = false;
#pragma unroll
            for (int h = 0; h < 4; ++h)
                if (elig[h]) {
                    lm = iv[h] > lm ? iv[h] : lm;
                    any = true;
                }
            if (__ballot(any) == 0ull) {
                easy = false;
                break;
            }
            S = wave_max_dpp(lm);
            int cnt = 0, who = 0;
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const bool eq = elig[h] && iv[h] == S;
                const unsigned long long m = __ballot(eq);
                cnt += __popcll(m);
                who = m != 0ull ? h * 64 + __builtin_ctzll(m) : who;
                elig[h] = elig[h] && !eq;
            }
            easy = easy && cnt == 1;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k == round) {
                    ecw[k] = who;
                    esc[k] = S;
                }
            total += cnt;
            if (total >= P.topn)
                break;
        }
        easy = easy && total == P.topn;
        if (lane == 0) {
            P.hard[(size_t)f * P.n_frames + t] = easy ? 0 : 1;
            if (easy) {
                P.topn_cw[pair] = (uint32_t)ecw[0] | (uint32_t)ecw[1] << 8 | (uint32_t)ecw[2] << 16
                    | (uint32_t)ecw[3] << 24;
                P.topn_sc[pair] = make_int4(esc[0], esc[1], esc[2], esc[3]);
            }
        }
        /* the candidates, compacted in index order */
        unsigned long long mk[4];
        int count = 0;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            mk[h] = __ballot(valid[h] && iv[h] >= S);
            count += __popcll(mk[h]);
        }
        int2 *cand = P.cand + pair * 64;
        if (count > 64) {
            cand[lane] = make_int2(INT_MIN, SEMI_WHOLE);
            continue;
        }
        if (lane >= count)
            cand[lane] = make_int2(INT_MIN, 0);
        int base = 0;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            if ((mk[h] >> lane) & 1ull) {
                const int pos = base + __popcll(mk[h] & ((1ull << lane) - 1ull));
                cand[pos] = make_int2(iv[h], (h * 64 + lane) | (tie[h] ? SEMI_TIE : 0) | SEMI_VALID);
            }
            base += __popcll(mk[h]);
        }
    }
}

/* ---------------------------------------------------------------------------------- */
/* the order chain                                                                     */
/* ---------------------------------------------------------------------------------- */
/* eval_topn's insertion (src/s2_semi_mgau.c:100-106): entry i with its new score s goes behind
 * every earlier entry that scores at least as much (strict >: an equal score stays behind) */
template <int TOPN>
__device__ __forceinline__ void
semi_place_rescored(int (&nc)[TOPN], int (&ns)[TOPN], int i, int c, int s)
{
    int pos = 0;
#pragma unroll
    for (int k = 0; k < TOPN; ++k)
        pos += (k < i && ns[k] >= s) ? 1 : 0;
#pragma unroll
    for (int k = TOPN - 1; k >= 1; --k)
        if (k <= i && k > pos) {
            ns[k] = ns[k - 1];
            nc[k] = nc[k - 1];
        }
#pragma unroll
    for (int k = 0; k < TOPN; ++k)
        if (k == pos) {
            ns[k] = s;
            nc[k] = c;
        }
}

/* eval_cb over up to 64 densities held one per lane, in lane order (cw ascending): `ok` marks
 * the lanes that hold one.  The walk is scalar code over a ballot of the densities that can
 * still be accepted; the list's worst score only rises, so the ballot is only ever narrowed. */
template <int TOPN>
__device__ __forceinline__ void
semi_walk(int cw, int s, bool tie_bit, bool ok, int (&Lc)[TOPN], int (&Ls)[TOPN])
{
    unsigned long long rel = __ballot(ok && s >= Ls[TOPN - 1]);
    const unsigned long long tiew = __ballot(tie_bit);
    while (rel != 0ull) {
        const int l = __builtin_ctzll(rel);
        rel &= rel - 1ull;
        const int c = __builtin_amdgcn_readlane(cw, l), sc = __builtin_amdgcn_readlane(s, l);
        const int w = Ls[TOPN - 1];
        bool present = false; /* already there: not inserted (:155-161) */
#pragma unroll
        for (int k = 0; k < TOPN; ++k)
            present = present || Lc[k] == c;
        if (present || !semi_accepts(sc, (tiew >> l) & 1ull, w))
            continue;
        /* before equal scores: d_int >= cur->score shifts (:163-164) */
        int pos = 0;
#pragma unroll
        for (int k = 0; k < TOPN - 1; ++k)
            pos += (Ls[k] > sc) ? 1 : 0;
#pragma unroll
        for (int k = TOPN - 1; k >= 1; --k)
            if (k > pos) {
                Ls[k] = Ls[k - 1];
                Lc[k] = Lc[k - 1];
            }
#pragma unroll
        for (int k = 0; k < TOPN; ++k)
            if (k == pos) {
                Ls[k] = sc;
                Lc[k] = c;
            }
        if (Ls[TOPN - 1] != w)
            rel &= __ballot(s >= Ls[TOPN - 1]);
    }
}

/* one frame of one stream: `r` is the lane's slot of the frame's candidates */
template <int TOPN>
__device__ __forceinline__ void
semi_frame(const SemiParams &P, size_t pair, int2 r, bool scan, int lane, int (&Lc)[TOPN],
           int (&Ls)[TOPN])
{
    const bool whole = !scan || __ballot((r.y & SEMI_WHOLE) != 0) != 0ull;
    const int *row = P.row_dint + pair * SSW_SC_MAX_DENSITY;
    const int ccw = r.y & 0xff;
    const bool cok = (r.y & SEMI_VALID) != 0;
    int nc[TOPN], ns[TOPN];
#pragma unroll
    for (int i = 0; i < TOPN; ++i) {
        const int c = Lc[i];
        int s;
        if (whole)
            s = row[c];
        else {
            const unsigned long long hit = __ballot(cok && ccw == c);
            const int found = __builtin_amdgcn_readlane(r.x, hit != 0ull ? __builtin_ctzll(hit) : 0);
            s = hit != 0ull ? found : INT_MIN;
        }
        semi_place_rescored<TOPN>(nc, ns, i, c, s);
    }
#pragma unroll
    for (int i = 0; i < TOPN; ++i) {
        Lc[i] = nc[i];
        Ls[i] = ns[i];
    }
    if (scan && !whole)
        semi_walk<TOPN>(ccw, r.x, (r.y & SEMI_TIE) != 0, cok, Lc, Ls);
    else if (scan) {
        for (int h = 0; h < (P.n_density + 63) / 64; ++h) {
            const int cw = h * 64 + lane;
            semi_walk<TOPN>(cw, row[cw], (P.row_tie[pair * 4 + h] >> lane) & 1ull,
                            cw < P.n_density, Lc, Ls);
        }
    }
    if (lane == 0) {
        uint32_t pk = 0;
        int sc[4] = { INT_MIN, INT_MIN, INT_MIN, INT_MIN };
#pragma unroll
        for (int k = 0; k < TOPN; ++k) {
            pk |= (uint32_t)(Lc[k] & 0xff) << (8 * k);
            sc[k] = Ls[k];
        }
        P.topn_cw[pair] = pk;
        P.topn_sc[pair] = make_int4(sc[0], sc[1], sc[2], sc[3]);
    }
}

/* One wave (a workgroup of 64) per (utterance, stream) chain; with chain_utts one per stream over
 * all the utterances, the history carried across their boundaries as the ring of two slots
 * carries it: frame numbers restart at 0 and frame 0 starts from slot 1, the last ODD-numbered
 * frame (an utterance of one frame leaves slot 1 as it found it).  The candidates of the next
 * four frames are fetched while four frames are walked: their addresses do not depend on the
 * history. */
template <int TOPN>
__global__ void __launch_bounds__(64)
semi_chain_kernel(SemiParams P)
{
    constexpr int PF = 4;
    const int lane = threadIdx.x;
    const int id = (int)blockIdx.x;
    if (id >= (P.chain_utts ? 1 : P.n_utts) * P.n_feat)
        return;
    const int u = id / P.n_feat, f = id - u * P.n_feat;
    int Lc[TOPN], Ls[TOPN];
    /* the reset state: codeword k, the worst score (src/s2_semi_mgau.c:993-1002) */
#pragma unroll
    for (int k = 0; k < TOPN; ++k) {
        Lc[k] = P.carry_pk != nullptr
            ? (int)((P.carry_pk[(size_t)u * P.n_feat + f] >> (8 * k)) & 0xffu)
            : k;
        /* (a carried codeword the codebook does not have: the host refuses it; bounded all the same) */
        Lc[k] = Lc[k] < P.n_density ? Lc[k] : k;
        Ls[k] = INT_MIN;
    }
    if (P.ds == 1 && !P.chain_utts) {
        /* the frames the density kernel could not settle (ties), 64 flags at a time; such a
         * frame starts from its predecessor's final order: in registers when the chain made it,
         * else what the density kernel stored for it */
        const int a = P.utt_off[u], b = P.utt_off[u + 1];
        int last = a - 1; /* the frame Lc belongs to (a - 1: the start order) */
        for (int t0 = a; t0 < b; t0 += 64) {
            const int tl = t0 + lane;
            unsigned long long todo
                = __ballot(tl < b && P.hard[(size_t)f * P.n_frames + (tl < b ? tl : a)] != 0);
            while (todo != 0ull) {
                const int t = t0 + __builtin_ctzll(todo);
                todo &= todo - 1ull;
                if (last != t - 1) {
                    const uint32_t pk = P.topn_cw[(size_t)(t - 1) * P.n_feat + f];
#pragma unroll
                    for (int k = 0; k < TOPN; ++k) {
                        Lc[k] = (int)((pk >> (8 * k)) & 0xffu);
                        Lc[k] = Lc[k] < P.n_density ? Lc[k] : k;
                    }
                }
                const size_t pair = (size_t)t * P.n_feat + f;
                semi_frame<TOPN>(P, pair, P.cand[pair * 64 + lane], true, lane, Lc, Ls);
                last = t;
            }
        }
        return;
    }
    const int u_end = P.chain_utts ? P.n_utts : u + 1;
    for (int uu = u; uu < u_end; ++uu) {
        const int a = P.utt_off[uu], b = P.utt_off[uu + 1];
        int2 nxt[PF];
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            const int t = a + i < P.n_frames ? a + i : P.n_frames - 1;
            nxt[i] = P.cand[((size_t)t * P.n_feat + f) * 64 + lane];
        }
        for (int t0 = a; t0 < b; t0 += PF) {
            int2 cur[PF];
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                cur[i] = nxt[i];
                const int t = t0 + PF + i < P.n_frames ? t0 + PF + i : P.n_frames - 1;
                nxt[i] = P.cand[((size_t)t * P.n_feat + f) * 64 + lane];
            }
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                const int t = t0 + i;
                if (t >= b)
                    break;
                const bool scan = ((t - a + P.frame_base) % P.ds) == 0; /* :176-178 */
                /* the last frame of an utterance of odd length writes slot 0, which the next
                 * utterance's frame 0 does not read: its result is stored, its order not carried */
                const bool off_chain = P.chain_utts && t == b - 1 && ((b - a) & 1);
                int Kc[TOPN];
#pragma unroll
                for (int k = 0; k < TOPN; ++k)
                    Kc[k] = Lc[k];
                semi_frame<TOPN>(P, (size_t)t * P.n_feat + f, cur[i], scan, lane, Lc, Ls);
                if (off_chain) {
#pragma unroll
                    for (int k = 0; k < TOPN; ++k)
                        Lc[k] = Kc[k];
                }
            }
        }
    }
}

/* ---------------------------------------------------------------------------------- */
/* senones                                                                             */
/* ---------------------------------------------------------------------------------- */
/* mgau_norm per stream (norm = top1 >> 10, each score min(96, -((s >> 10) - norm)), the count is
 * topn) and get_scores_8b_feat_all: the row starts at 0; per stream the first density's
 * weight + score, the others log-added in list order with the 8-bit table, the sum added as int16.
 * No subtraction of a minimum, no acoustic weight.  A thread takes 4 neighbouring senones: the
 * frame's n_feat x topn weight rows are read as dwords, lanes side by side.
 * grid: n_frames * ceil(n_sen / 1024) workgroups of 256. */
__global__ void __launch_bounds__(256)
semi_senone_kernel(SemiParams P)
{
    __shared__ uint8_t s_tab[SSW_LOGADD_LDS];
    for (int i = threadIdx.x; i < SSW_LOGADD_LDS; i += 256)
        s_tab[i] = i < 256 ? P.logadd8[i] : (uint8_t)0;
    __syncthreads();
    const int chunks = (P.n_sen + 1023) / 1024;
    const int t = (int)(blockIdx.x / (unsigned)chunks);
    const int s0 = ((int)(blockIdx.x % (unsigned)chunks) * 256 + (int)threadIdx.x) * 4;
    if (t >= P.n_frames || s0 >= P.n_sen)
        return;
    int acc[4] = { 0, 0, 0, 0 };
    for (int f = 0; f < P.n_feat; ++f) {
        const size_t pair = (size_t)t * P.n_feat + f;
        const uint32_t pk = P.topn_cw[pair];
        const int4 raw4 = P.topn_sc[pair];
        const int raw[4] = { raw4.x, raw4.y, raw4.z, raw4.w };
        const int norm = raw[0] >> SSW_SENSCR_SHIFT;
        int tmp[4] = { 0, 0, 0, 0 };
        for (int k = 0; k < P.topn; ++k) {
            int cw = (int)((pk >> (8 * k)) & 0xffu);
            cw = cw < P.n_density ? cw : 0;
            int sc = -((raw[k] >> SSW_SENSCR_SHIFT) - norm);
            sc = sc > SSW_MAX_NEG_ASCR ? SSW_MAX_NEG_ASCR : sc;
            sc = sc < 0 ? 0 : sc; /* (never for a sorted list: keeps the table index bounded) */
            const uint32_t w4 = *reinterpret_cast<const uint32_t *>(
                P.mixw + ((size_t)f * P.n_density + cw) * P.sc_stride + s0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int y = (int)((w4 >> (8 * q)) & 0xffu) + sc;
                if (k == 0)
                    tmp[q] = y;
                else {
                    /* fast_logmath_add: min - table[|difference|]; the difference stays below
                     * 255 + 96 + 3 table[0] < 512, the table is zero from its 256th entry on */
                    const int hi = tmp[q] > y ? tmp[q] : y, lo = tmp[q] < y ? tmp[q] : y;
                    const int dd = hi - lo < SSW_LOGADD_LDS - 1 ? hi - lo : SSW_LOGADD_LDS - 1;
                    tmp[q] = lo - (int)s_tab[dd];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            acc[q] = (int)(int16_t)(acc[q] + tmp[q]);
    }
    int16_t *o = P.out + (size_t)t * P.n_sen + s0;
    if ((reinterpret_cast<uintptr_t>(o) & 3) == 0 && s0 + 3 < P.n_sen) { /* two dword stores */
        uint32_t *o2 = reinterpret_cast<uint32_t *>(o);
        o2[0] = ((uint32_t)acc[0] & 0xffffu) | ((uint32_t)acc[1] << 16);
        o2[1] = ((uint32_t)acc[2] & 0xffffu) | ((uint32_t)acc[3] << 16);
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (s0 + q < P.n_sen)
            o[q] = (int16_t)acc[q];
}
