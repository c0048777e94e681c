/* ssw_k7_fpactive.inc -- device: the first pass in the reference's DEFAULT configuration
 * (compallsen = no) as a batch (round 6; host half: ssw_host_fpactive.inc).
 * Part of the single translation unit ssw_kernels.hip (included there, in this order).
 *
 * In that configuration frame t is scored only after frame t - 1 has been searched: acmod scores
 * the senones of the HMMs the search holds active (fsg_search_sen_active clears and rebuilds the
 * set every frame, src/fsg_search.c:310-325, :677-680), through the uint8 delta list of
 * acmod_flags2list (src/acmod.c:947-999: gaps above 255 list extra "bridge" senones), and the
 * PTM scorer scans the codebooks of the listed senones only, normalises over them and subtracts
 * the best LISTED score (src/ptm_mgau.c:264-403).  Served frame by frame that is two launches and
 * a search step per frame.  Here the dependency is broken by SPECULATION AND PROOF:
 *   1. a trajectory of active sets is assumed (first: the one the search takes on the
 *      compallsen = yes scores; first_pass_kernel<.., EXPORT> writes a bit per HMM and frame),
 *   2. fpa_plan_kernel turns each frame's HMM set into the listed senones (bridges included)
 *      and the codebooks they make active,
 *   3. the whole batch is scored with those per-frame sets (the scan with per-frame codebook
 *      masks; senone_listed_kernel below),
 *   4. the search runs again on THOSE scores and exports the sets it took,
 *   5. fpa_compare_kernel: an utterance whose sets equal the assumed ones frame for frame is
 *      PROVEN -- by induction over the frames its search read nothing but scores the reference
 *      would have computed, so it is the reference's search; any other utterance is right up
 *      to its first differing frame, INCLUDING that frame's set, and goes round again with the
 *      sets of step 4 as the assumption: the proven prefix grows by at least a frame per round.
 */

struct FpaPlanParams {
    const unsigned long long *act_mask; /* first_pass_kernel<.., EXPORT> */
    const long long *act_off;           /* [n_utts] */
    const int *utt_off;                 /* [n_utts + 1] */
    const int *node_base, *node_cnt;    /* [n_utts]: the utterance's phone-tree HMMs among senid's
                                           rows -- a text's own graph, or the grammar it is searched
                                           against (many utterances may share one) */
    const uint16_t *senid;              /* [n_nodes][4] */
    const uint8_t *sen2cb;              /* NULL (a continuous model): no codebook mask is made */
    uint32_t *listed;                   /* [n_frames][nw32] listed senones, bridges included */
    unsigned long long *cbmask;         /* [n_frames] */
    int32_t *iota;                      /* [n_frames] = t (the scan's segment table) */
    uint32_t *seed;                     /* NULL, or [n_utts][nw32]: the flags (no bridges) of every
                                           utterance's LAST frame: what acmod's vector holds when
                                           the second pass starts (src/state_align_search.c:186-189) */
    int32_t *n_listed;                  /* NULL, or [n_frames] (statistics) */
    int n_utts, n_frames, n_sen, nw32;
    int frame_lo, frame_hi;             /* the frames this launch plans */
};

/* One wave per frame, four frames per workgroup.  Per wave in LDS (FpaPlanCarve): the senone
 * bitmap [nw32 words], the ascending list of the flagged senones [cap uint16] and the two words
 * of the codebook mask. */
__global__ void __launch_bounds__(256)
fpa_plan_kernel(FpaPlanParams P, int cap)
{
    extern __shared__ __align__(16) unsigned char fpa_smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    /* The wave's block is FpaPlanCarve's (ssw_senone_lds.inc), from which fpa_shape takes the byte
     * count.  Within it the carve stays written out as typed-pointer steps: taken from the
     * struct's byte offsets the same addresses are computed by other instructions.
     * tests/harness/senone_lds_host.cpp holds these lines verbatim and compares them with the
     * struct region by region: change both together. */
    const size_t per_wave = FpaPlanCarve(P.nw32, cap).per_wave();
    uint32_t *bm = reinterpret_cast<uint32_t *>(fpa_smem + (size_t)w * per_wave);
    uint16_t *lst = reinterpret_cast<uint16_t *>(bm + P.nw32);
    uint32_t *cbm = reinterpret_cast<uint32_t *>(lst + cap); /* two words */
    const int t = P.frame_lo + (int)blockIdx.x * 4 + w;
    if (t >= P.frame_hi)
        return;
    /* the frame's utterance: the last u with utt_off[u] <= t (empty utterances own no frame) */
    int lo = 0, hi = P.n_utts - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (P.utt_off[mid] <= t)
            lo = mid;
        else
            hi = mid - 1;
    }
    const int u = lo;
    const int nb = P.node_base[u], N = P.node_cnt[u], MW = (N + 63) >> 6;
    const int f = t - P.utt_off[u];
    const unsigned long long *mask = P.act_mask + P.act_off[u] + (long long)f * MW;
    for (int i = lane; i < P.nw32; i += 64)
        bm[i] = 0u;
    if (lane < 2)
        cbm[lane] = 0u;
    wave_sync();
    /* acmod_activate_hmm of every active HMM (src/acmod.c:905-945).  A long text's row is
     * hundreds of words of which a handful are set: 64 words a step, the set ones visited */
    for (int k0 = 0; k0 < MW; k0 += 64) {
        const unsigned long long mine = k0 + lane < MW ? mask[k0 + lane] : 0ull;
        unsigned long long nz = __ballot(mine != 0ull);
        while (nz != 0ull) {
            const int j = __builtin_ctzll(nz);
            nz &= nz - 1ull;
            const unsigned long long word
                = (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine, j)
                | ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mine >> 32), j) << 32);
            if ((word >> lane) & 1ull) {
                const uint16_t *sn = P.senid + (size_t)(nb + 64 * (k0 + j) + lane) * 4;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const uint32_t s = sn[q];
                    atomicOr(&bm[s >> 5], 1u << (s & 31));
                }
            }
        }
    }
    wave_sync();
    if (P.seed != nullptr && t + 1 == P.utt_off[u + 1])
        for (int i = lane; i < P.nw32; i += 64)
            P.seed[(size_t)u * P.nw32 + i] = bm[i];
    /* the flagged senones in ascending order: lane l owns the words [l C, (l + 1) C) */
    const int C = (P.nw32 + 63) >> 6;
    int cnt = 0;
    for (int k = 0; k < C; ++k) {
        const int i = lane * C + k;
        cnt += i < P.nw32 ? __popc(bm[i]) : 0;
    }
    int incl = cnt; /* inclusive prefix sum over the lanes */
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        incl += lane >= d ? o : 0;
    }
    const int total = __builtin_amdgcn_readlane(incl, 63);
    int pos = incl - cnt;
    for (int k = 0; k < C; ++k) {
        const int i = lane * C + k;
        uint32_t word = i < P.nw32 ? bm[i] : 0u;
        while (word != 0u) {
            const int b = __builtin_ctz(word);
            word &= word - 1u;
            if (pos < cap)
                lst[pos] = (uint16_t)(32 * i + b);
            ++pos;
        }
    }
    wave_sync();
    /* acmod_flags2list (src/acmod.c:947-999): a gap of more than 255 to the senone listed
     * before (0 before the first) is bridged by listing senones 255 apart */
    const int n = total < cap ? total : cap; /* (cap = n_sen or 3 x the most HMMs: never short) */
    uint32_t mycb0 = 0u, mycb1 = 0u;
    int n_bridge = 0;
    for (int i = lane; i < n; i += 64) {
        const int sen = lst[i], prev = i > 0 ? (int)lst[i - 1] : 0;
        const int cb = P.sen2cb != nullptr ? (int)P.sen2cb[sen] : 64;
        mycb0 |= cb < 32 ? 1u << cb : 0u;
        mycb1 |= cb >= 32 && cb < 64 ? 1u << (cb - 32) : 0u;
        const int r = sen - prev;
        const int K = r > 0 ? (r - 1) / 255 : 0;
        for (int k = 1; k <= K; ++k) {
            const int b = prev + 255 * k;
            atomicOr(&bm[b >> 5], 1u << (b & 31));
            const int cbb = P.sen2cb != nullptr ? (int)P.sen2cb[b] : 64;
            mycb0 |= cbb < 32 ? 1u << cbb : 0u;
            mycb1 |= cbb >= 32 && cbb < 64 ? 1u << (cbb - 32) : 0u;
            ++n_bridge;
        }
    }
    if (mycb0)
        atomicOr(&cbm[0], mycb0);
    if (mycb1)
        atomicOr(&cbm[1], mycb1);
    wave_sync();
    uint32_t *out = P.listed + (size_t)t * P.nw32;
    for (int i = lane; i < P.nw32; i += 64)
        out[i] = bm[i];
    if (P.n_listed != nullptr) {
        int nbr = n_bridge;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            nbr += __shfl_xor(nbr, d, 64);
        if (lane == 0)
            P.n_listed[t] = total + nbr;
    }
    if (lane == 0) {
        P.cbmask[t] = (unsigned long long)cbm[0] | ((unsigned long long)cbm[1] << 32);
        P.iota[t] = t;
    }
}

/* The rows of the utterances a launch of the sliding-window or the HBM-resident search kernel
 * is about to export into (those kernels write only the words that hold an active HMM; the
 * register kernel writes every word), and of the ones grammar_search_kernel<.., EXPORT> is about
 * to search.  One workgroup per utterance. */
__global__ void __launch_bounds__(256)
fpa_clear_kernel(unsigned long long *__restrict__ mask, const long long *__restrict__ act_off,
                 const int *__restrict__ utt_off, const int *__restrict__ node_cnt,
                 const int *__restrict__ only)
{
    const int u = only != nullptr ? only[blockIdx.x] : (int)blockIdx.x;
    const int MW = (node_cnt[u] + 63) >> 6;
    const long long n = (long long)(utt_off[u + 1] - utt_off[u]) * MW;
    unsigned long long *p = mask + act_off[u];
    for (long long i = threadIdx.x; i < n; i += 256)
        p[i] = 0ull;
}

/* What decoder_alignment's second pass starts from in the default configuration (cfg->
 * two_pass_history): acmod_rewind keeps the scorer's top-N history, and frame 0 of the second
 * pass copies slot 1 of its two-slot ring -- the lists after the first pass's last ODD-numbered
 * frame (src/decoder.c:786-793, src/ptm_mgau.c:425-437) -- for EVERY codebook, the ones that
 * frame did not scan included (theirs were re-sorted by every frame since they were last
 * scanned: eval_topn runs for all, src/ptm_mgau.c:236-238).  Which is what
 * carried_order_masked derives from the features and the proven per-frame codebook masks.
 * One wave per (utterance, codebook x stream); the records straight from global memory (a few
 * frames' worth per wave).  rows [n_utts][n_cbf]: 4 codewords packed best first. */
__global__ void __launch_bounds__(64)
fpa_carry_rows_kernel(FramesParams P, const float *__restrict__ rec28, const float *__restrict__ feats,
                      const int *__restrict__ utt_off, uint32_t *__restrict__ rows)
{
    const int u = (int)blockIdx.x / P.n_cbf, cbf = (int)blockIdx.x % P.n_cbf, lane = threadIdx.x;
    const int t0 = utt_off[u], n = utt_off[u + 1] - t0;
    uint32_t pk = SSW_ORDER_RESET; /* an utterance of one frame never wrote slot 1: the reset order */
    if (n >= 2) {
        const int last_odd = t0 + ((n >> 1) << 1) - 1; /* T even: its last frame; T odd: T - 2 */
        const float *srow0 = rec28 + ((size_t)cbf * 128 + lane) * SSW_REC28_FLOATS;
        const float *srow1 = srow0 + 64 * SSW_REC28_FLOATS;
        int Lc[4];
        carried_order_masked<13, true>(P, cbf, feats, P.featoff[cbf % P.n_feat], last_odd, lane, srow0,
                                       srow1, 0, Lc);
        pk = order_pack(Lc);
    }
    if (lane == 0)
        rows[(size_t)u * P.n_cbf + cbf] = pk;
}

/* Per utterance: the first frame whose exported sets differ between two runs of the search
 * (FPA_NO_DIFF: none -- the utterance is proven).  gridDim.x utterances x gridDim.y slices of
 * each one's words (a 2,000-word page is 29 M words: one workgroup took 54 ms over them);
 * first_diff[] starts at FPA_NO_DIFF (a memset of 0x7f bytes). */
#define FPA_NO_DIFF 0x7f7f7f7f
__global__ void __launch_bounds__(256)
fpa_compare_kernel(const unsigned long long *__restrict__ a, const unsigned long long *__restrict__ b,
                   const long long *__restrict__ act_off, const int *__restrict__ utt_off,
                   const int *__restrict__ node_cnt, const int *__restrict__ only,
                   int32_t *__restrict__ first_diff)
{
    const int u = only != nullptr ? only[blockIdx.x] : (int)blockIdx.x;
    const int MW = (node_cnt[u] + 63) >> 6;
    const long long n = (long long)(utt_off[u + 1] - utt_off[u]) * MW, base = act_off[u];
    int mine = FPA_NO_DIFF;
    for (long long i = (long long)blockIdx.y * 256 + threadIdx.x; i < n; i += 256ll * gridDim.y)
        if (a[base + i] != b[base + i]) {
            mine = (int)(i / MW);
            break; /* (this thread's later words are later frames) */
        }
    if (mine != FPA_NO_DIFF)
        atomicMin(&first_diff[u], mine);
}

/* The compallsen = no half of ptm_mgau_frame_eval (src/ptm_mgau.c:264-403) -- and of
 * ms_cont_mgau_frame_eval (src/ms_mgau.c:322-365) -- for every frame of a batch, each frame with
 * a listed set of its own (a bitmap, bridges included).  One WAVE per frame, four frames per
 * workgroup, as senone_active2_kernel; the listed senones are taken from the bitmap.  Writes the
 * listed entries of the [n_sen] row (what a search that stays inside the set reads); with `full`
 * the rest of the row as acmod's buffer would hold it (PTM: 0 - best, src/ptm_mgau.c:333,
 * :392-400; ms: 0). */
struct SenoneListedParams {
    const uint32_t *topn_cw;
    const int4 *topn_sc;
    const uint8_t *mixw, *logadd8, *sen2cb;
    const uint16_t *sen_slot;
    const uint32_t *listed;           /* [..][nw32], indexed by batch frame */
    const unsigned long long *cbmask; /* [..] */
    int16_t *out;                     /* [..][n_sen] */
    int n_frames, frame_base;         /* this launch: frames frame_base .. + n_frames (topn_* start
                                         at frame_base, everything else is indexed by batch frame) */
    int n_cb, n_feat, n_density, n_sen, slot_stride, nw32;
    int zero, aw;
    int cap, full;
    /* full == 2 (rounds over the few utterances that are still unproven): the unlisted entries
     * become what their compallsen = yes scores (`yes`, rows laid out like `out`) suggest they
     * would be if they were listed -- yes score minus the yes score of the best listed senone.
     * Nothing the proof rests on: a search that leaves the assumed sets reads them, and the
     * closer they are, the better the NEXT assumption (a newly entered HMM judged on a stale
     * score costs a round per frame until its fate settles) */
    const int16_t *yes;
};

template <bool MS>
__global__ void __launch_bounds__(256)
senone_listed_kernel(SenoneListedParams P)
{
    __shared__ uint8_t s_tab[SSW_LOGADD_LDS];
    extern __shared__ __align__(16) unsigned char fpa_smem[];
    const int n_cbf = P.n_cb * P.n_feat;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    /* per wave: normalised scores and codewords of every (codebook, stream) | the list | its raw
     * scores | the entry counter */
    const ListedCarve carve(MS, n_cbf, P.cap);
    unsigned char *mine = fpa_smem + carve.wave(w);
    uint32_t *s_ns4 = reinterpret_cast<uint32_t *>(mine + carve.ns4());
    uint32_t *s_cw4 = reinterpret_cast<uint32_t *>(mine + carve.cw4());
    uint16_t *s_sen = reinterpret_cast<uint16_t *>(mine + carve.sen());
    int16_t *s_a = reinterpret_cast<int16_t *>(mine + carve.a());
    int *s_n = reinterpret_cast<int *>(mine + carve.count());
    logadd_table_to_lds(s_tab, P.logadd8, tid, 256);
    if (lane == 0)
        *s_n = 0;
    __syncthreads();
    const int t = P.frame_base + (int)blockIdx.x * 4 + w;
    if (t >= P.frame_base + P.n_frames)
        return;
    const uint32_t *cw = P.topn_cw + (size_t)(t - P.frame_base) * n_cbf;
    const int4 *sc = P.topn_sc + (size_t)(t - P.frame_base) * n_cbf;
    const uint32_t *bits = P.listed + (size_t)t * P.nw32;
    /* the listed senones, in any order */
    for (int i = lane; i < P.nw32; i += 64) {
        uint32_t word = bits[i];
        if (word != 0u) {
            int pos = atomicAdd(s_n, __popc(word));
            while (word != 0u) {
                const int b = __builtin_ctz(word);
                word &= word - 1u;
                if (pos < P.cap)
                    s_sen[pos] = (uint16_t)(32 * i + b);
                ++pos;
            }
        }
    }
    if (!MS)
        wave_codebook_norm(sc, cw, n_cbf, P.n_feat, P.cbmask[t], lane, s_ns4, s_cw4);
    wave_sync();
    const int n_all = *s_n;
    const int n_ent = n_all < P.cap ? n_all : P.cap; /* (cap = n_sen: never short) */
    int best = INT_MAX;
    for (int i = lane; i < n_ent; i += 64) {
        const int sen = s_sen[i];
        const int sl = P.sen_slot[sen], cb = P.sen2cb[sen];
        const int a = MS
            ? ms_slot_score(P.mixw + sl, P.n_feat, P.n_density, P.slot_stride, cw + cb * P.n_feat,
                            sc + cb * P.n_feat, P.zero, P.aw, s_tab)
            : ptm_slot_score(P.mixw + sl, P.n_feat, P.n_density, P.slot_stride,
                             s_cw4 + cb * P.n_feat, s_ns4 + cb * P.n_feat, s_tab);
        s_a[i] = (int16_t)a;
        best = a < best ? a : best;
    }
    best = wave_best_or_zero(best); /* 0: a frame the search has no HMM left in (it fails there) */
    wave_sync();
    int16_t *orow = P.out + (size_t)t * P.n_sen;
    if (P.full == 2) {
        const int16_t *yrow = P.yes + (size_t)t * P.n_sen;
        int delta = INT_MAX; /* the yes score of a best listed senone */
        for (int i = lane; i < n_ent; i += 64)
            if ((int)s_a[i] == best) {
                const int y = yrow[s_sen[i]];
                delta = y < delta ? y : delta;
            }
        delta = -wave_max_dpp(-delta);
        if (delta == INT_MAX)
            delta = 0;
        for (int sen = lane; sen < P.n_sen; sen += 64)
            if (!((bits[sen >> 5] >> (sen & 31)) & 1u)) {
                orow[sen] = (int16_t)clamp_i16((int)yrow[sen] - delta);
            }
    } else if (P.full) { /* the unlisted entries first: listed ones are skipped, no store is overwritten */
        const int16_t rest = MS ? (int16_t)0 : (int16_t)(0 - best);
        for (int sen = lane; sen < P.n_sen; sen += 64)
            if (!((bits[sen >> 5] >> (sen & 31)) & 1u))
                orow[sen] = rest;
    }
    for (int i = lane; i < n_ent; i += 64)
        orow[s_sen[i]] = final_score<MS>((int)s_a[i], best);
}
