/* ssw_align_common.inc -- device: what the 3-state forced-alignment kernels share.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */
/* ---------------------------------------------------------------------------------- */
/* viterbi_align_mw_kernel, _mwb_kernel and _win_kernel (ssw_k2_align.inc) run the same frame  */
/* step with a phone's HMM in the registers of a lane, one wave per 64-phone word; they differ */
/* in their tokens, mwb's replay and win's sliding window.  The step is here, once.            */
/* viterbi_align_reg_kernel (one wave, several words per lane) uses the lane's constants,      */
/* phone_transition, the enter and the record; viterbi_align_kernel and                        */
/* viterbi_align_any_kernel, whose state lives in LDS / HBM arrays, the renormalisation test.  */
/* The model tables are passed as pointers: AlignParams / AlignUtt are defined in              */
/* ssw_k2_align.inc, which follows.                                                            */
/* ---------------------------------------------------------------------------------- */

/* hmm_vit_eval_3st_lr, src/hmm.c:482-567.  n0..n2 are the NEGATED senone scores.  Written
 * with selects instead of the reference's nested ifs (a lone wave pays for every branch with
 * scalar exec-mask bookkeeping); the decision tree is the same, including the t2 that the state-2
 * block inherits from the exit block when it has no 0->2 arc of its own (:496,501-502,519-520):
 *   exit   only if s1 + n1 > WORST:  t1 = a2 + tp23, t2 = a1 + tp13 if that arc exists else
 *          INT_MIN;  take t1 iff t1 > t2 (history of state 2), else t2 (history of state 1)
 *   state2 t0 = a2 + tp22, t1 = a1 + tp12, t2 = a0 + tp02 if that arc exists, else the exit
 *          block's t2;  if t0 > t1: (t2 > t0 ? t2/h0 : t0/h2) else (t2 > t1 ? t2/h0 : t1/h1)
 *   state1 t0 = a1 + tp11, t1 = a0 + tp01;  t0 > t1 ? t0/h1 : t1/h0
 *   state0 a0 + tp00;  every new score clamped to WORST, best = max over them and the exit. */
/* a1_live / quirk (optional, for the byte-token kernel): whether the exit block ran, and whether
 * state 2 took the exit block's t2 -- a score that is state 1's with the history of state 0 */
__device__ __forceinline__ int
vit_eval_3st(int &s0, int &s1, int &s2, int &h0, int &h1, int &h2, int &os, int &oh, int n0,
             int n1, int n2, uint32_t tpa, uint32_t tpb, uint32_t tpc, bool *a1_live_out = nullptr,
             bool *quirk_out = nullptr)
{
#define TPQ(word, j) (-(int)(((word) >> (8 * (j))) & 0xffu))
    const int tp00 = TPQ(tpa, 0), tp01 = TPQ(tpa, 1), tp02 = TPQ(tpa, 2);
    const int tp11 = TPQ(tpb, 1), tp12 = TPQ(tpb, 2), tp13 = TPQ(tpb, 3);
    const int tp22 = TPQ(tpc, 2), tp23 = TPQ(tpc, 3);
#undef TPQ
    const int a2 = s2 + n2, a1 = s1 + n1, a0 = s0 + n0;
    const int W = SSW_WORST_SCORE;

    /* exit */
    const bool a1_live = a1 > W;
    const int e1 = a2 + tp23;
    const int e2 = (a1_live && tp13 > -255) ? a1 + tp13 : INT_MIN;
    const bool from2 = e1 > e2;
    int s3 = from2 ? e1 : e2;
    s3 = s3 < W ? W : s3;
    const int oh_new = from2 ? h2 : h1;
    os = a1_live ? s3 : os;
    oh = a1_live ? oh_new : oh;
    int best = a1_live ? s3 : W;

    /* state 2 (uses h1, h2 as they were) */
    const int t0 = a2 + tp22, t1 = a1 + tp12;
    const int t2 = (tp02 > -255) ? a0 + tp02 : e2;
    const bool self2 = t0 > t1;
    const int base2 = self2 ? t0 : t1;
    const int hb2 = self2 ? h2 : h1;
    const bool skip2 = t2 > base2;
    int ns2 = skip2 ? t2 : base2;
    h2 = skip2 ? h0 : hb2;
    if (a1_live_out != nullptr)
        *a1_live_out = a1_live;
    if (quirk_out != nullptr)
        *quirk_out = skip2 && !(tp02 > -255);
    ns2 = ns2 < W ? W : ns2;
    best = ns2 > best ? ns2 : best;

    /* state 1 */
    const int u0 = a1 + tp11, u1 = a0 + tp01;
    const bool self1 = u0 > u1;
    int ns1 = self1 ? u0 : u1;
    h1 = self1 ? h1 : h0;
    ns1 = ns1 < W ? W : ns1;
    best = ns1 > best ? ns1 : best;

    /* state 0 */
    int ns0 = a0 + tp00;
    ns0 = ns0 < W ? W : ns0;
    best = ns0 > best ? ns0 : best;
    s0 = ns0;
    s1 = ns1;
    s2 = ns2;
    return best;
}

/* Neighbour values move by one lane with DPP wave shifts, whose `old` operand supplies the value
 * that crosses a 64-phone word boundary. */
__device__ __forceinline__ int
lane_from_next(int v, int edge) /* lane i <- lane i+1, lane 63 <- edge */
{
    return __builtin_amdgcn_update_dpp(edge, v, 0x130, 0xf, 0xf, false);
}

__device__ __forceinline__ int
lane_from_prev(int v, int edge) /* lane i <- lane i-1, lane 0 <- edge */
{
    return __builtin_amdgcn_update_dpp(edge, v, 0x138, 0xf, 0xf, false);
}

/* v_max3_i32 */
__device__ __forceinline__ int
max3_i32(int a, int b, int c)
{
    const int m = a > b ? a : b;
    return m > c ? m : c;
}

/* ---- a lane's phone: its constants and its HMM ------------------------------------------ */

/* p: the phone's index in the utterance; a lane without a phone (!real) carries constants that
 * keep its HMM inert */
struct AlignPhone {
    int p;
    bool real;
    uint32_t tpa, tpb, tpc; /* the transition matrix's three rows */
    int sid01, sid2;        /* where the three states' scores stand in a score row (AlignUtt) */
    int ef, sf_next;        /* the phone's last frame; the first frame of the phone after it */
};

/* NP phones from phone_off on in tmatid / senid / sf / ef (AlignParams) */
__device__ __forceinline__ AlignPhone
align_phone_load(int p, int NP, int phone_off, const uint8_t *tp_tab, const int16_t *tmatid,
                 const uint16_t *senid, const int32_t *sf, const int32_t *ef)
{
    AlignPhone c;
    c.p = p;
    c.real = p < NP;
    const int gp = phone_off + (c.real ? p : 0);
    const uint32_t *tp = reinterpret_cast<const uint32_t *>(tp_tab) + (size_t)tmatid[gp] * 3;
    c.tpa = c.real ? tp[0] : 0u;
    c.tpb = c.real ? tp[1] : 0u;
    c.tpc = c.real ? tp[2] : 0u;
    c.sid01 = c.real ? ((int)senid[gp * 3] | ((int)senid[gp * 3 + 1] << 16)) : 0;
    c.sid2 = c.real ? (int)senid[gp * 3 + 2] : 0;
    c.ef = c.real ? ef[gp] : INT_MAX;
    c.sf_next = (p + 1 < NP) ? sf[gp + 1] : INT_MAX; /* nothing enters past the end */
    return c;
}

struct AlignHmm {
    int s0, s1, s2, os; /* state and exit scores */
    int h0, h1, h2, oh; /* their histories */
    int fr;             /* the last frame the HMM is active in */
};

/* hmm_clear, src/hmm.c:124-140 */
__device__ __forceinline__ void
hmm_clear(AlignHmm &h)
{
    h.s0 = h.s1 = h.s2 = h.os = SSW_WORST_SCORE;
    h.h0 = h.h1 = h.h2 = h.oh = -1;
    h.fr = -1;
}

/* state_align_search_start: hmm_enter(hmms, 0, 0, 0) */
__device__ __forceinline__ void
align_search_start(AlignHmm &h, int p)
{
    if (p == 0) {
        h.s0 = 0;
        h.h0 = 0;
        h.fr = 0;
    }
}

/* ---- score look-ahead -------------------------------------------------------------------- */

/* Senone scores of a lane's phone: three rotating register sets, so that the scattered 2-byte
 * gathers of frame t + 2 are requested at the top of frame t (a frame step is shorter than a DRAM
 * round trip).  The three scores stay in three registers until their frame -- packing two of
 * them at the load made every frame wait for the loads it had just issued.
 * Every lane loads (lanes without a phone read senone 0: their HMM is inert whatever the
 * score), and what is loaded is the ALIGNED DWORD that holds the 16-bit score: a 32-bit value
 * the compiler cannot narrow, so that the extraction -- and with it the wait for the load --
 * stays behind the asm pin at the top of the frame two frames later.  (As 16-bit loads the
 * extension was hoisted to the end of the previous frame, right behind that frame's token
 * stores, and `s_waitcnt vmcnt(0)` waits for stores as well.)  An aligned dword that holds a
 * valid half never leaves that half's page; the other half is discarded. */
struct ScoreAhead {
    const int16_t *senscr; /* AlignParams::senscr */
    long long scr_off;     /* AlignUtt's row layout */
    int scr_stride, last;  /* the utterance's last frame: later ones re-read its row */
};

/* the 4-byte aligned address at or below frame t's row; lo: what the row's own leaves modulo 4 */
__device__ __forceinline__ const char *
score_row(const ScoreAhead &a, int t, uint32_t &lo)
{
    const char *scr0 = reinterpret_cast<const char *>(a.senscr);
    const size_t ro = (size_t)(a.scr_off + (long long)(t < a.last ? t : a.last) * a.scr_stride) * 2;
    lo = ((uint32_t)(reinterpret_cast<uintptr_t>(scr0) & 3) + (uint32_t)ro) & 3u;
    return scr0 + ro - lo;
}

/* request the three scores of frame t */
__device__ __forceinline__ void
score_fetch(const ScoreAhead &a, const AlignPhone &c, int t, uint32_t &v0, uint32_t &v1, uint32_t &v2)
{
    uint32_t lo;
    const char *base = score_row(a, t, lo);
    v0 = *reinterpret_cast<const uint32_t *>(base + ((2u * (c.sid01 & 0xffff) + lo) & ~3u));
    v1 = *reinterpret_cast<const uint32_t *>(base + ((2u * ((c.sid01 >> 16) & 0xffff) + lo) & ~3u));
    v2 = *reinterpret_cast<const uint32_t *>(base + ((2u * (uint32_t)c.sid2 + lo) & ~3u));
}

/* the half of its dword a score sits in: bit offset 0 or 16 */
__device__ __forceinline__ uint32_t
score_half_of(const ScoreAhead &a, int t, int sid)
{
    uint32_t lo;
    score_row(a, t, lo);
    return ((2u * (uint32_t)sid + lo) & 2u) * 8u;
}

/* top of frame t: request frame t + 2 into fut*, then take frame t's NEGATED scores out of raw*,
 * requested two frames ago */
__device__ __forceinline__ void
score_step(const ScoreAhead &a, const AlignPhone &c, int t, uint32_t raw0, uint32_t raw1,
           uint32_t raw2, uint32_t &fut0, uint32_t &fut1, uint32_t &fut2, int &n0, int &n1, int &n2)
{
    score_fetch(a, c, t + 2, fut0, fut1, fut2);
    /* the empty asm pins the wait for the loads of two frames ago HERE */
    asm volatile("" : "+v"(raw0), "+v"(raw1), "+v"(raw2));
    n0 = -(int)(short)(raw0 >> score_half_of(a, t, c.sid01 & 0xffff));
    n1 = -(int)(short)(raw1 >> score_half_of(a, t, (c.sid01 >> 16) & 0xffff));
    n2 = -(int)(short)(raw2 >> score_half_of(a, t, c.sid2));
}

/* ---- renormalize_hmms, evaluate_hmms + prune_hmms (state_align_search.c:57-106) ---------- */

/* The frame step is written with selects rather than branches: a lone wave pays for every
 * divergent `if` with scalar exec-mask bookkeeping, and lanes without a phone hold an inert HMM
 * (scores WORST, frame -1) that the arithmetic leaves inert.  Only stores are masked. */

__device__ __forceinline__ bool
align_renorm_due(int best_score)
{
    return (best_score - 0x300000) < SSW_WORST_SCORE;
}

/* hmm_normalize (src/hmm.c:150-161) when it is due; returns the amount taken off (0: none) */
__device__ __forceinline__ int
renormalize_hmm(AlignHmm &h, int best_score)
{
    const int W = SSW_WORST_SCORE;
    const bool renorm = align_renorm_due(best_score);
    h.s0 = (renorm && h.s0 > W) ? h.s0 - best_score : h.s0;
    h.s1 = (renorm && h.s1 > W) ? h.s1 - best_score : h.s1;
    h.s2 = (renorm && h.s2 > W) ? h.s2 - best_score : h.s2;
    h.os = (renorm && h.os > W) ? h.os - best_score : h.os;
    return renorm ? best_score : 0;
}

/* Frame t with the negated scores n0..n2: evaluated for every lane, kept for the phones that are
 * active in this frame, which stay active while their window lasts.  Returns this frame's best
 * score of the HMM (WORST: not active); a1_live / quirk as vit_eval_3st gives them. */
__device__ __forceinline__ int
evaluate_hmm(AlignHmm &h, const AlignPhone &c, int t, int n0, int n1, int n2,
             bool *a1_live = nullptr, bool *quirk = nullptr)
{
    const bool active = h.fr >= t;
    int e0 = h.s0, e1 = h.s1, e2 = h.s2, g0 = h.h0, g1 = h.h1, g2 = h.h2, eos = h.os, eoh = h.oh;
    const int b = vit_eval_3st(e0, e1, e2, g0, g1, g2, eos, eoh, n0, n1, n2, c.tpa, c.tpb, c.tpc,
                               a1_live, quirk);
    h.s0 = active ? e0 : h.s0;
    h.s1 = active ? e1 : h.s1;
    h.s2 = active ? e2 : h.s2;
    h.h1 = active ? g1 : h.h1;
    h.h2 = active ? g2 : h.h2;
    h.os = active ? eos : h.os;
    h.oh = active ? eoh : h.oh;
    h.fr = (active && t + 1 <= c.ef) ? t + 1 : h.fr;
    return active ? b : SSW_WORST_SCORE;
}

/* ---- what the waves of a workgroup exchange ---------------------------------------------- */

/* One wave per 64-phone word (up to 16 waves).  Per frame the waves meet twice at an LDS-only
 * barrier (no drain of the outstanding token stores): once to publish their boundary values
 * (frame / entry score of their first phone, exit score / history of their last) and their best
 * score, once to publish their carry code of phone_transition, after which every wave folds the
 * carry chain up to its own word.  The slots are double-buffered by frame parity: a wave can be
 * at most one barrier ahead of the slowest one. */
#define SSW_ALIGN_MAX_WAVES 16

struct AlignExchange {
    /* bs / gp: all 16 slots are read by every wave (one round trip for everything a barrier
     * publishes, no exec-masked reads); the slots of waves that do not exist hold WORST / 0 */
    __attribute__((aligned(16))) int bs[2][SSW_ALIGN_MAX_WAVES];
    int fr0[2][SSW_ALIGN_MAX_WAVES], s00[2][SSW_ALIGN_MAX_WAVES];
    int os63[2][SSW_ALIGN_MAX_WAVES], oh63[2][SSW_ALIGN_MAX_WAVES];
    int gp[2][SSW_ALIGN_MAX_WAVES]; /* bit 0: carry generated, bit 1: carry passed on */
};

/* before the kernel's first __syncthreads() */
__device__ __forceinline__ void
exchange_init(AlignExchange &x)
{
    if (threadIdx.x < 2 * SSW_ALIGN_MAX_WAVES) { /* both parities */
        const int par = threadIdx.x / SSW_ALIGN_MAX_WAVES, slot = threadIdx.x % SSW_ALIGN_MAX_WAVES;
        x.bs[par][slot] = SSW_WORST_SCORE;
        x.gp[par][slot] = 0;
    }
}

/* wave w's best score of the frame (bs: this lane's) and its boundary values */
__device__ __forceinline__ void
exchange_publish(AlignExchange &x, int par, int w, int lane, int bs, const AlignHmm &h)
{
    bs = wave_max_dpp(bs);
    if (lane == 0) {
        x.bs[par][w] = bs;
        x.fr0[par][w] = h.fr;
        x.s00[par][w] = h.s0;
    }
    if (lane == 63) {
        x.os63[par][w] = h.os;
        x.oh63[par][w] = h.oh;
    }
}

/* the frame's best score over all waves: four 16-byte reads of one address, no cross-lane
 * reduction */
__device__ __forceinline__ int
exchange_best_score(const AlignExchange &x, int par)
{
    const int4 *bq = reinterpret_cast<const int4 *>(x.bs[par]);
    const int4 q0 = bq[0], q1 = bq[1], q2 = bq[2], q3 = bq[3];
    return max3_i32(max3_i32(max3_i32(q0.x, q0.y, q0.z), max3_i32(q0.w, q1.x, q1.y),
                             max3_i32(q1.z, q1.w, q2.x)),
                    max3_i32(max3_i32(q2.y, q2.z, q2.w), max3_i32(q3.x, q3.y, q3.z), q3.w),
                    SSW_WORST_SCORE);
}

/* ---- phone_transition (state_align_search.c:108-133) as a carry chain --------------------- */

/* Phone i + 1 is entered in frame t + 1 when phone i may hand on (C_i: the next phone's window
 * has begun, and it is inactive or its entry score is below i's exit score -- all read from the
 * state evaluate/prune left, as in the reference's loop, where hmm i + 1 is examined before it
 * is entered) and i is itself active (A_i) or was entered a moment ago:
 * entered(i+1) = C_i & (A_i | entered(i)) is the carry recurrence of the binary sum X + Y with
 * X = C, Y = A & C.  Across words it is a carry-lookahead: every word publishes whether it
 * generates a carry out (g) and whether it would pass one through (p). */
struct AlignCarry {
    unsigned long long X, Y; /* the word's summands */
    int code;                /* g | p << 1, for AlignExchange::gp */
};

__device__ __forceinline__ int
carry_out(unsigned long long X, unsigned long long Y, unsigned long long S)
{
    return (int)(((X & Y) | ((X | Y) & ~S)) >> 63);
}

/* nx_fr / nx_s0: frame and entry score of the phone after the word's last (the next word's
 * first).  Where the kernel has no next word in reach it passes frame -1 and any score: -1 < t
 * decides C before the score is looked at, and C's other terms decide whether anything is past
 * the word at all. */
__device__ __forceinline__ AlignCarry
phone_transition(const AlignHmm &h, const AlignPhone &c, int NP, int nx_fr, int nx_s0, int t)
{
    const int nfr = lane_from_next(h.fr, nx_fr);
    const int ns0 = lane_from_next(h.s0, nx_s0);
    const bool a_bit = h.fr == t + 1; /* lanes without a phone keep frame -1 */
    const bool c_bit = c.p + 1 < NP && t + 1 >= c.sf_next && (nfr < t || h.os > ns0);
    const unsigned long long Am = __ballot(a_bit), Cm = __ballot(c_bit);
    AlignCarry k;
    k.X = Cm;
    k.Y = Am & Cm;
    const unsigned long long S0 = k.X + k.Y, S1 = S0 + 1ull;
    const int g_out = carry_out(k.X, k.Y, S0), c1_out = carry_out(k.X, k.Y, S1);
    k.code = g_out | ((c1_out & ~g_out) << 1);
    return k;
}

/* The carry into the word at position pos of npos; code: lane i's read of the published code of
 * position i (lanes from npos on: of any position): bit pos of the carries of (G | P) + G, one
 * more add.  Position 0 needs no guard: nothing carries into bit 0 of a sum. */
__device__ __forceinline__ int
carry_into_word(int code, int pos, int npos)
{
    const unsigned long long lowm = (1ull << npos) - 1ull;
    const unsigned long long Gm = __ballot(code & 1) & lowm, Pm = __ballot(code & 2) & lowm;
    const unsigned long long XX = Gm | Pm;
    const unsigned long long carries = (XX + Gm) ^ XX ^ Gm;
    return (int)((carries >> pos) & 1ull);
}

/* is this lane's phone entered, given the carry into its word?  c_out: the carry out of it */
__device__ __forceinline__ bool
phone_entered(const AlignCarry &k, int cin, int lane, int *c_out = nullptr)
{
    const unsigned long long S = k.X + k.Y + (unsigned long long)cin;
    const unsigned long long E = S ^ k.X ^ k.Y; /* bit i: phone (w*64+i) is entered */
    if (c_out != nullptr)
        *c_out = carry_out(k.X, k.Y, S);
    return (E >> lane) & 1ull;
}

/* ---- hmm_enter (src/hmm.c:142-148), record_transitions (state_align_search.c:149-175) ---- */

/* Enter from the lane before; prev_os / prev_oh: exit score and history of the last phone of the
 * word before, for lane 0.  (A word with nothing before it may pass anything: its lane 0 is
 * entered by a carry into the word, and none comes.) */
__device__ __forceinline__ void
hmm_enter(AlignHmm &h, bool entered, int nf, int prev_os, int prev_oh)
{
    const int src_os = lane_from_prev(h.os, prev_os);
    const int src_oh = lane_from_prev(h.oh, prev_oh);
    h.s0 = entered ? src_os : h.s0;
    h.h0 = entered ? src_oh : h.h0;
    h.fr = entered ? nf : h.fr;
}

/* what both token forms end with: the histories of a recorded HMM become its own state ids */
__device__ __forceinline__ void
reset_histories(AlignHmm &h, int p, bool rec)
{
    h.h0 = rec ? p * 3 : h.h0;
    h.h1 = rec ? p * 3 + 1 : h.h1;
    h.h2 = rec ? p * 3 + 2 : h.h2;
}

/* the reference's tokens {history, score}, {-1, -1} for an HMM that is not active */
__device__ __forceinline__ void
record_transitions(AlignHmm &h, int p, int t, int2 &k0, int2 &k1, int2 &k2)
{
    const bool rec = h.fr >= t;
    k0 = make_int2(rec ? h.h0 : -1, rec ? h.s0 : -1);
    k1 = make_int2(rec ? h.h1 : -1, rec ? h.s1 : -1);
    k2 = make_int2(rec ? h.h2 : -1, rec ? h.s2 : -1);
    reset_histories(h, p, rec);
}

/* the same as three 2-bit back-pointers in one byte: own id - history (0, 1, 2), 3 = none.
 * Returns false when a history is further back than two bits can say. */
__device__ __forceinline__ bool
record_transitions_2bit(AlignHmm &h, int p, int t, uint8_t &tok)
{
    const bool rec = h.fr >= t;
    const int id0 = p * 3;
    const uint32_t d0 = (rec && h.h0 >= 0) ? (uint32_t)(id0 - h.h0) : 3u;
    const uint32_t d1 = (rec && h.h1 >= 0) ? (uint32_t)(id0 + 1 - h.h1) : 3u;
    const uint32_t d2 = (rec && h.h2 >= 0) ? (uint32_t)(id0 + 2 - h.h2) : 3u;
    const bool far = rec && ((h.h0 >= 0 && d0 > 2u) || (h.h1 >= 0 && d1 > 2u) || (h.h2 >= 0 && d2 > 2u));
    reset_histories(h, p, rec);
    tok = (uint8_t)((d0 & 3u) | (d1 & 3u) << 2 | (d2 & 3u) << 4);
    return !far;
}
