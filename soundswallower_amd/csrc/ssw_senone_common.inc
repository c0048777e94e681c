/* ssw_senone_common.inc -- the steps of the reference's senone scorers that several kernels must
 * do identically, each written once with its citation: ptm_senone_kernel, ptm_frame_kernel,
 * ms_senone_kernel, senone_active2_kernel (ssw_k1b_senone.inc), senone_listed_kernel
 * (ssw_k7_fpactive.inc) and the continuous-density kernels (ssw_k11_cont.inc) call them.
 * Part of the single translation unit ssw_kernels.hip (included there, in this order). */

static_assert(SSW_SENONE_NORM_W == SSW_MAX_FEAT, "SenoneCarve: a normaliser word per stream");

/* a score as acmod's int16 buffer holds it where the reference clamps (src/ms_senone.c:355-360,
 * src/ms_mgau.c:314-320); the one-frame ms vtable call applies it on the host as well */
__host__ __device__ __forceinline__ int
clamp_i16(int v)
{
    v = v > 32767 ? 32767 : v;
    v = v < -32768 ? -32768 : v;
    return v;
}

/* fast_logmath_add (tied_mgau_common.h:100-117): min(x, y) - table[|x - y|] */
__device__ __forceinline__ int
fast_logadd(int x, int y, const uint8_t *tab)
{
    /* x is the running value: it can dip up to 3 T below zero (two equal entries whose value is
     * below tab[0]), so |x - y| is taken on the full ints (a 16-bit SAD would see the sign
     * extension as a difference of 2^16).  d <= 351 + 3 T < SSW_LOGADD_LDS: the callers' tables
     * are padded with zeros to 512 entries, the value every entry from 29 up holds. */
    const int hi = x > y ? x : y;
    const int r = x < y ? x : y;
    return r - (int)tab[hi - r];
}

/* logmath_add on the shift-10 table (src/logmath.c:228-272): max(x, y) + table[|x - y|], with
 * the "zero" short-cuts; the table has exactly 256 entries for the bases the loader accepts. */
__device__ __forceinline__ int
ms_logadd(int x, int y, int zero, const uint8_t *tab)
{
    int d = x > y ? x - y : y - x;
    int r = x > y ? x : y;
    int add = d < 256 ? (int)tab[d < 256 ? d : 255] : 0;
    int v = r + add;
    v = (y <= zero) ? x : v;
    v = (x <= zero) ? y : v;
    return v;
}

/* the table fast_logadd indexes without a bound: the 256 entries, then zeros (what every entry
 * from 29 up holds) to SSW_LOGADD_LDS bytes; the caller's barrier follows */
__device__ __forceinline__ void
logadd_table_to_lds(uint8_t *s_tab, const uint8_t *logadd8, int tid, int nthr)
{
    for (int i = tid; i < SSW_LOGADD_LDS; i += nthr)
        s_tab[i] = i < 256 ? logadd8[i] : (uint8_t)0;
}

/* codebook_norm's inner step (src/ptm_mgau.c:284-290): s = min(96, -((s >> 10) - norm)) for the
 * four codewords of a (codebook, stream), a byte each; an inactive codebook's senones see 96 for
 * all of them (:353-364) */
__device__ __forceinline__ uint32_t
ptm_norm_pack4(int4 sc, int norm, bool active)
{
    const int v[4] = { sc.x, sc.y, sc.z, sc.w };
    uint32_t pk = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int q = -((v[k] >> SSW_SENSCR_SHIFT) - norm);
        q = q > SSW_MAX_NEG_ASCR ? SSW_MAX_NEG_ASCR : q;
        if (!active)
            q = SSW_MAX_NEG_ASCR;
        pk |= (uint32_t)(q & 0xff) << (8 * k);
    }
    return pk;
}

/* codebook_norm over an active set by ONE wave (src/ptm_mgau.c:271-290, :353-364): the per-stream
 * normalisers over the codebooks of `cbmask` as wave reductions, then the packed scores and the
 * codewords of every (codebook, stream) of frame rows sc / cw into the wave's s_ns4 / s_cw4.  The
 * caller's wave_sync follows. */
__device__ __forceinline__ void
wave_codebook_norm(const int4 *sc, const uint32_t *cw, int n_cbf, int n_feat,
                   unsigned long long cbmask, int lane, uint32_t *s_ns4, uint32_t *s_cw4)
{
    int nm[SSW_MAX_FEAT];
#pragma unroll
    for (int f = 0; f < SSW_MAX_FEAT; ++f)
        nm[f] = SSW_WORST_SCORE;
    for (int i = lane; i < n_cbf; i += 64)
        if ((cbmask >> (i / n_feat)) & 1ull) {
            const int v = sc[i].x >> SSW_SENSCR_SHIFT;
            const int f = i % n_feat;
#pragma unroll
            for (int k = 0; k < SSW_MAX_FEAT; ++k)
                nm[k] = (k == f && v > nm[k]) ? v : nm[k];
        }
#pragma unroll
    for (int f = 0; f < SSW_MAX_FEAT; ++f)
        nm[f] = f < n_feat ? wave_max_dpp(nm[f]) : 0;
    for (int i = lane; i < n_cbf; i += 64) {
        const int f = i % n_feat;
        int norm = nm[0];
#pragma unroll
        for (int k = 1; k < SSW_MAX_FEAT; ++k)
            norm = k == f ? nm[k] : norm;
        s_ns4[i] = ptm_norm_pack4(sc[i], norm, (cbmask >> (i / n_feat)) & 1ull);
        s_cw4[i] = cw[i];
    }
}

/* One slot's PTM score with the reference's own arithmetic (src/ptm_mgau.c:342-395): per stream
 * the log-add of weight + normalised score over the four codewords, summed over the streams.
 * cw4 / ns4 = the packed codewords and normalised scores of the slot's codebook, [n_feat];
 * mixw_sl = the slot's column of the mixture weights (byte gathers). */
__device__ __forceinline__ int
ptm_slot_score(const uint8_t *mixw_sl, int n_feat, int n_density, int slot_stride,
               const uint32_t *cw4s, const uint32_t *ns4s, const uint8_t *tab)
{
    int a = 0;
    for (int f = 0; f < n_feat; ++f) {
        const uint32_t cw4 = cw4s[f], ns4 = ns4s[f];
        const uint8_t *mw = mixw_sl + (size_t)f * n_density * slot_stride;
        int fden = (int)mw[(size_t)(cw4 & 0xffu) * slot_stride] + (int)(ns4 & 0xffu);
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const int y = (int)mw[(size_t)((cw4 >> (8 * k)) & 0xffu) * slot_stride]
                + (int)((ns4 >> (8 * k)) & 0xffu);
            fden = fast_logadd(fden, y, tab);
        }
        a += fden;
    }
    return a;
}

/* what senone_eval does with a slot's sum (src/ms_senone.c:351-360): / aw (C division truncates
 * toward zero; 1 is the default), then the clamp */
__device__ __forceinline__ int
ms_finish(int sum, int aw)
{
    if (aw != 1)
        sum = sum / aw;
    return clamp_i16(sum);
}

/* One slot's ms score (senone_eval, src/ms_senone.c:314-362): per stream logmath_add over
 * fden - pdf of the four codewords, negated and summed, / aw, clamped.  cw4s / fds = the top-N
 * block's rows of the slot's codebook, [n_feat]; byte gathers from the slot's column. */
__device__ __forceinline__ int
ms_slot_score(const uint8_t *pdf_sl, int n_feat, int n_density, int slot_stride,
              const uint32_t *cw4s, const int4 *fds, int zero, int aw, const uint8_t *tab)
{
    int a = 0;
    for (int f = 0; f < n_feat; ++f) {
        const uint32_t cw4 = cw4s[f];
        const int4 fd4 = fds[f];
        const int fd[4] = { fd4.x, fd4.y, fd4.z, fd4.w };
        const uint8_t *mw = pdf_sl + (size_t)f * n_density * slot_stride;
        int fscr = fd[0] - (int)mw[(size_t)(cw4 & 0xffu) * slot_stride];
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const int fw = fd[k] - (int)mw[(size_t)((cw4 >> (8 * k)) & 0xffu) * slot_stride];
            fscr = ms_logadd(fscr, fw, zero, tab);
        }
        a -= fscr;
    }
    return ms_finish(a, aw);
}

/* The same sum for the four slots of a quad, stream f's term: v[j] -= the stream's score of slot
 * j, from the four codewords' dword rows (a byte per slot) at mq = the quad's first column.  The
 * callers loop over the streams (one with a compile-time count) and finish with ms_finish. */
__device__ __forceinline__ void
ms_quad_scores(const uint8_t *mq, int f, int n_density, int slot_stride, uint32_t cw4, int4 fd4,
               int zero, const uint8_t *tab, int (&v)[4])
{
    const int fd[4] = { fd4.x, fd4.y, fd4.z, fd4.w };
    uint32_t mw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t cw = (cw4 >> (8 * k)) & 0xffu;
        mw[k] = *reinterpret_cast<const uint32_t *>(mq + ((size_t)f * n_density + cw) * slot_stride);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int fscr = fd[0] - (int)((mw[0] >> (8 * j)) & 0xffu);
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            int fw = fd[k] - (int)((mw[k] >> (8 * j)) & 0xffu);
            fscr = ms_logadd(fscr, fw, zero, tab);
        }
        v[j] -= fscr;
    }
}

/* what acmod's buffer holds for a scored entry: PTM `senone_scores[i] -= bestscore` in int16,
 * which wraps (src/ptm_mgau.c:399); ms (score - best) with the clamp (src/ms_mgau.c:314-320) */
template <bool MS>
__device__ __forceinline__ int16_t
final_score(int raw, int best)
{
    return MS ? (int16_t)clamp_i16(raw - best) : (int16_t)(raw - best);
}

/* a wave's best (smallest) score; 0 where no lane had one (best = INT_MAX in all of them) */
__device__ __forceinline__ int
wave_best_or_zero(int best)
{
    best = -wave_max_dpp(-(best == INT_MAX ? INT_MAX - 1 : best));
    return best == INT_MAX - 1 ? 0 : best;
}

/* the count of the scans' exact in-wave pass, moved from its running word [0] to [1] (= the last
 * batch's; acc: added to it instead); one thread of the launch calls this */
__device__ __forceinline__ void
move_exact_count(unsigned long long *nfixed, int acc)
{
    nfixed[1] = (acc ? nfixed[1] : 0ull) + nfixed[0];
    nfixed[0] = 0ull;
}
